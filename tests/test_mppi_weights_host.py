"""CPU checks of the importance-weight fold (no GPU): the float64 emulation of the three-level fold of csrc/nlc_mppi_dev.h
against the plain one-level formula in np.longdouble, on every case tests/test_gpu_mppi_weights.py runs through the kernels,
within the bound derived in tests/mppi_weight_cases.py -- which also shows that the reference side alone meets every condition
the GPU file asserts -- and the Python restatements of the shard merge (sharding.py, oracle/mppi.py) on +inf shards."""

import numpy as np
import pytest
import torch

import mppi_weight_cases as mw


def _mp(mpmath, v):
    """np.longdouble -> mpmath, exactly (the mantissa in two float64 pieces, then the exponent)."""
    m, e = np.frexp(np.longdouble(v))
    hi = float(m)
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(float(m - np.longdouble(hi))), int(e))


def test_longdouble_reference_against_mpmath_50_digits():
    """The K = 1000 wide-spread case: the np.longdouble reference agrees with 50-digit arithmetic far inside the bound (its own
    error: a 64-bit mantissa, argument error 2^-64 x, one exp, 1000 additions)."""
    import mpmath

    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not wider than float64 here"
    case = mw.wide_spread(1000, 3, 1, 0.7, -1e6)
    ref, hi = mw.reference(case), mw.reference_mpmath(case)
    x = ref["x"].astype(np.float64)
    dUb = mw.bounds(case, ref)[2].reshape(-1)
    with mpmath.workdps(50):
        for k in range(case.K):
            assert abs(_mp(mpmath, ref["omega"][k]) - hi["omega"][k]) <= (x[k] + 1100) * 2.0 ** -63 * hi["omega"][k]
        for i in range(case.T * case.nu):
            assert abs(_mp(mpmath, ref["dU"].reshape(-1)[i]) - hi["dU"][i]) <= 1e-3 * float(dUb[i])


def test_emulated_fold_within_derived_bound(record_property):
    """Every finite-result case (a - e, g): the emulation of the three-level fold stays inside the derived bound."""
    worst, where = 0.0, None
    for case in mw.all_finite_result_cases():
        ref = mw.reference(case)
        em = mw.emulate_fold(case)
        r = mw.check(case, ref, em["w"], em["omega"], em["dU"], "emulation")
        if r > worst:
            worst, where = r, case.name
    print(f"largest emulation error / bound: {worst:.4f} at {where}")
    record_property("worst_ratio", worst)
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("K", [1000, 4097])
def test_emulated_ties_are_exact(K):
    case = mw.ties(K)
    em = mw.emulate_fold(case)
    assert np.all(em["w"] == 1.0) and np.all(em["omega"] == 1.0 / K) and em["eta"] == float(K)
    mw.check(case, mw.reference(case), em["w"], em["omega"], em["dU"])


@pytest.mark.parametrize("K,kstar", mw.SURVIVORS)
def test_emulated_one_survivor_is_one_hot(K, kstar):
    case = mw.one_survivor(K, kstar)
    em = mw.emulate_fold(case)
    hot = np.zeros(K)
    hot[kstar] = 1.0
    assert np.array_equal(em["omega"], hot) and em["w"][kstar] == 1.0 and np.array_equal(em["dU"], case.noise[kstar])
    ref = mw.reference(case)
    assert np.array_equal(ref["omega"].astype(np.float64), hot)


@pytest.mark.parametrize("sign", [1, -1])
def test_emulated_padding_lanes_do_not_reach_the_minimum(sign):
    for K in (1000, 17):
        case = mw.padding(K, sign)
        em = mw.emulate_fold(case)
        assert em["w"][np.argmin(case.cost)] == 1.0 and em["beta"] == case.cost.min()


def test_inf_tile_is_nan_without_the_rule_and_absent_with_it():
    """The divergence the rule closes: an all-+inf tile gives eta_b = NaN, and 0 * NaN reaches eta.  With the rule the result
    equals the population without those samples."""
    case = mw.inf_cases()[0]
    assert np.isnan(mw.emulate_fold(case, inf_rule=False)["eta"])
    em = mw.emulate_fold(case)
    keep = np.isfinite(case.cost)
    sub = mw.Case("without", case.cost[keep], case.noise[keep], case.lam)
    em_sub = mw.emulate_fold(sub)
    assert np.isfinite(em["eta"]) and np.all(em["omega"][~keep] == 0.0)
    np.testing.assert_allclose(em["dU"], em_sub["dU"], rtol=0, atol=float(np.max(mw.bounds(sub, mw.reference(sub))[2])) * 2)
    assert np.allclose(mw.reference(case)["dU"].astype(np.float64), mw.reference(sub)["dU"].astype(np.float64), rtol=1e-15, atol=0)


@pytest.mark.parametrize("case", mw.poisoned_cases(), ids=repr)
def test_poisoned_costs_stay_nan(case):
    """NaN, -inf and all-+inf costs: the reference's dU is NaN, and so is the fold's (with the +inf rule in place)."""
    assert np.all(np.isnan(mw.reference(case)["dU"].astype(np.float64)))
    assert np.all(np.isnan(mw.emulate_fold(case)["dU"]))


def test_finite_costs_do_not_see_the_rule():
    """The rule is a select on `== +inf`: no bit of a finite-cost result depends on it."""
    for case in (mw.wide_spread(1000, 3, 1, 0.7, 0.0), mw.wide_spread(4097, 40, 2, 1e-3, 1e9), mw.ties(1000)):
        a, b = mw.emulate_fold(case, inf_rule=True), mw.emulate_fold(case, inf_rule=False)
        for k in ("w", "omega", "dU"):
            assert np.array_equal(a[k], b[k])


# ------------------------------------------------------------------ the Python restatements of the shard merge
def _one_level(case):
    ref = mw.reference(case)
    return ref, mw.bounds(case, ref)


@pytest.mark.parametrize("G,case", mw.shard_cases(), ids=lambda v: repr(v))
def test_emulated_shard_merge_equals_one_level(G, case):
    ref = mw.reference(case)
    em = mw.emulate_fold(case, G=G)
    mw.check(case, ref, em["w"], em["omega"], em["dU"], f"G={G}")


@pytest.mark.parametrize("G,case", mw.shard_cases(), ids=lambda v: repr(v))
def test_oracle_shard_partials_and_merge_equal_one_level(G, case):
    from oracle import mppi as omppi

    cost, eps = torch.from_numpy(case.cost), torch.from_numpy(case.noise)
    Kl = case.K // G
    parts = torch.stack([omppi.shard_partials(cost[g * Kl:(g + 1) * Kl], eps[g * Kl:(g + 1) * Kl], case.lam) for g in range(G)])
    beta, eta, dU = omppi.merge_partials(parts, case.lam)
    ref, (rel, cap, dUb) = _one_level(case)
    assert float(beta) == float(ref["beta"])
    assert abs(np.longdouble(float(eta)) - ref["eta"]) <= ref["eta"] * 256 * mw.EPS
    err = np.abs(dU.numpy().reshape(case.T, case.nu).astype(np.longdouble) - ref["dU"])
    assert np.all(err <= dUb), float(np.max(err / dUb))


@pytest.mark.parametrize("G,case", mw.shard_cases(), ids=lambda v: repr(v))
def test_torch_shard_partials_and_merge_equal_one_level(G, case):
    """sharding.shard_partials_torch (the shard branch of MPPIDelay._torch_command) + sharding.merge_partials_torch."""
    from neurallaplacecontrol_amd.sharding import merge_partials_torch, shard_partials_torch

    cost, eps = torch.from_numpy(case.cost), torch.from_numpy(case.noise)
    Kl = case.K // G
    parts = torch.stack([shard_partials_torch(cost[g * Kl:(g + 1) * Kl], eps[g * Kl:(g + 1) * Kl], case.lam) for g in range(G)])
    assert bool(torch.isfinite(parts[:, 1:]).all())
    beta, eta, S = merge_partials_torch(parts, case.lam)
    ref, (rel, cap, dUb) = _one_level(case)
    assert float(beta) == float(ref["beta"])
    err = np.abs((S / eta).numpy().reshape(case.T, case.nu).astype(np.longdouble) - ref["dU"])
    assert np.all(err <= dUb), float(np.max(err / dUb))
    # what _torch_command derives from the merge: cost_total_non_zero and omega
    w = torch.exp(-(cost - beta) / case.lam)
    mw.check(case, ref, w.numpy(), (w / eta).numpy(), (S / eta).numpy(), "torch shard merge")


def test_torch_and_oracle_merges_keep_poisoned_shards_nan():
    from neurallaplacecontrol_amd.sharding import merge_partials_torch, shard_partials_torch
    from oracle import mppi as omppi

    for case in mw.poisoned_cases():
        if case.K % 2:
            continue
        cost, eps = torch.from_numpy(case.cost), torch.from_numpy(case.noise)
        Kl = case.K // 2
        for sp, mg in ((omppi.shard_partials, omppi.merge_partials), (shard_partials_torch, merge_partials_torch)):
            parts = torch.stack([sp(cost[g * Kl:(g + 1) * Kl], eps[g * Kl:(g + 1) * Kl], case.lam) for g in range(2)])
            out = mg(parts, case.lam)
            dU = out[2] if mg is omppi.merge_partials else out[2] / out[1]
            assert bool(torch.isnan(dU).all()), case
