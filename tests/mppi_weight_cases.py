"""Inputs, reference and error bound shared by the importance-weight tests (tests/test_mppi_weights_host.py on the CPU,
tests/test_gpu_mppi_weights.py on the GPU).

Reference: the planner's plain ONE-level formula (planners/mppi_delay.py:210-216) in np.longdouble,
    beta = min c,  w = exp(-(c - beta)/lambda),  eta = sum w,  omega = w/eta,  dU = sum_k omega_k noise_k.
Under test: the three-level fold of csrc/nlc_mppi_dev.h (16-sample tiles, 64-tile chunks + rank fold, shard merge), on the
GPU by the kernels and here by `emulate_fold`, a float64 numpy restatement of their operation order.

Bound (derived, not tuned).  With x_k = (c_k - beta)/lambda: every level rounds 1/lambda, the difference and their product,
an argument error of at most 3 * 2^-53 * |x| per level, and one exp adds about an ulp; the three levels' arguments add up to
x_k.  The summation depth of the fold is 4 butterfly levels + 16 tiles + 3 waves + nch <= 17 chunks + the shards.  Hence
    |omega_k - omega_ref,k|  <=  omega_ref,k * (4 x_k + 256) * 2^-53                                  (x_k <= 690)
    0 <= omega_k <= e^-680 / eta_ref                                                                  (x_k >  690: denormal or 0)
    |dU_i - dU_ref,i|        <=  sum_k omega_ref,k |noise_k,i| (4 x_k + 256) * 2^-53  (+ e^-680/eta_ref |noise_k,i| where x_k > 690)
and cost_total_non_zero (w) is held to the same relative bound as omega.
"""

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
TILE, CHUNK = 16, 64
X_DENORMAL = 690.0

K_EDGES = (1, 15, 16, 17, 1000, 4096, 4097, 16384, 16400)
TN_EDGES = ((3, 1), (63, 1), (32, 2), (40, 2))
# every K at (3, 1), every (T, nu) at K = 1000 and 4097
SHAPES = [(K, 3, 1) for K in K_EDGES] + [(K, T, nu) for K in (1000, 4097) for (T, nu) in TN_EDGES[1:]]
LAMBDAS = (1e-3, 0.7, 50.0)
C0S = (0.0, -1e6, 1e9)


class Case:
    def __init__(self, name, cost, noise, lam):
        self.name, self.lam = name, float(lam)
        self.cost = np.ascontiguousarray(cost, dtype=np.float64)
        self.noise = np.ascontiguousarray(noise, dtype=np.float64)
        self.K, self.T, self.nu = self.noise.shape

    def __repr__(self):
        return self.name


def _noise(rng, K, T, nu):
    return rng.standard_normal((K, T, nu))


def _seed(K, T, nu, extra=0):
    return np.random.default_rng([K, T, nu, extra])


# ------------------------------------------------------------------ the cases of the issue
def wide_spread(K, T, nu, lam, c0, extra=0):
    """a: c_k = c0 + lambda x_k, x_k = per-tile offset in [0, 700] + per-sample uniform in [0, 30], one x_k exactly 0."""
    rng = _seed(K, T, nu, 1 + extra)
    nblk = (K + TILE - 1) // TILE
    x = np.repeat(rng.uniform(0.0, 700.0, nblk), TILE)[:K] + rng.uniform(0.0, 30.0, K)
    x[int(rng.integers(K))] = 0.0
    return Case(f"wide-K{K}-T{T}-nu{nu}-lam{lam:g}-c0{c0:g}", c0 + lam * x, _noise(rng, K, T, nu), lam)


def ties(K, T=3, nu=1, lam=0.7):
    """b: all costs equal to a value that is no small integer."""
    rng = _seed(K, T, nu, 2)
    return Case(f"ties-K{K}", np.full(K, 1e6 + 0.1), _noise(rng, K, T, nu), lam)


SURVIVORS = [(1000, 0), (1000, 15), (1000, 16), (1000, 999), (4097, 1023), (4097, 1024), (4097, 4095), (4097, 4096),
             (16400, 16399)]


def one_survivor(K, kstar, T=3, nu=1, lam=0.7):
    """c: every other cost is 1000 .. 1100 lambda above the winner's (at least 800 lambda: exp underflows to exactly 0)."""
    rng = _seed(K, T, nu, 3 + kstar)
    c = 3.7 + lam * (1000.0 + rng.uniform(0.0, 100.0, K))
    c[kstar] = 3.7
    return Case(f"survivor-K{K}-at{kstar}", c, _noise(rng, K, T, nu), lam)


def padding(K, sign, T=3, nu=1, lam=0.7):
    """d: ragged K, all costs at sign * 1e6 +- small: a padded lane's cost must not reach the tile minimum."""
    rng = _seed(K, T, nu, 4)
    return Case(f"padding-K{K}-{'plus' if sign > 0 else 'minus'}", sign * 1e6 + rng.uniform(-2.0, 2.0, K), _noise(rng, K, T, nu), lam)


def _finite_costs(rng, K, lam):
    return 5.0 + lam * rng.uniform(0.0, 40.0, K)


def inf_cases():
    """e: +inf costs weigh zero; everything else as if those samples were absent."""
    out = []
    for name, K, (T, nu), sel in (
        ("tile", 1000, (3, 1), lambda K: np.arange(32, 48)),
        ("halftile", 1000, (3, 1), lambda K: np.arange(40, 48)),
        ("chunk", 5000, (3, 1), lambda K: np.arange(1024, 2048)),
        ("all-but-one-ragged", 1000, (3, 1), lambda K: np.delete(np.arange(K), 995)),
        ("all-chunks-but-last", 16400, (3, 1), lambda K: np.arange(0, 16384)),
        ("tile-81", 1000, (40, 2), lambda K: np.arange(32, 48)),
    ):
        for lam in (0.7,) if name != "tile" else LAMBDAS:
            rng = _seed(K, T, nu, 5)
            c = _finite_costs(rng, K, lam)
            c[sel(K)] = np.inf
            out.append(Case(f"inf-{name}-lam{lam:g}", c, _noise(rng, K, T, nu), lam))
    return out


def poisoned_cases():
    """h: a NaN cost, a -inf cost and all costs +inf make the reference's action NaN; that must stay visible."""
    out = []
    for name, K, fill in (("nan", 40, lambda c: c.__setitem__(21, np.nan)), ("neginf", 40, lambda c: c.__setitem__(21, -np.inf)),
                          ("allinf", 40, lambda c: c.fill(np.inf)), ("nan-first", 17, lambda c: c.__setitem__(0, np.nan))):
        rng = _seed(K, 3, 1, 6)
        c = _finite_costs(rng, K, 0.7)
        fill(c)
        out.append(Case(f"poisoned-{name}", c, _noise(rng, K, 3, 1), 0.7))
    return out


def shard_cases():
    """g: (G, case) pairs; shard g owns samples [g K/G, (g+1) K/G)."""
    out = []
    for G in (2, 4):
        K, T, nu, lam = 272 * G, 5, 1, 0.7  # 272 = 17 tiles per shard
        Kl = K // G
        rng = _seed(K, T, nu, 7)
        base = _finite_costs(rng, K, lam)
        far = base.copy()
        far[Kl:2 * Kl] += 900.0 * lam  # shard 1's beta_g is > 800 lambda above the others: scale exactly 0
        out.append((G, Case(f"shard-G{G}-far", far, _noise(rng, K, T, nu), lam)))
        inf1 = base.copy()
        inf1[(G - 1) * Kl:] = np.inf  # the last shard is entirely +inf
        out.append((G, Case(f"shard-G{G}-inf", inf1, _noise(rng, K, T, nu), lam)))
        only = np.full(K, np.inf)
        only[Kl + 100] = base[Kl + 100]  # shard 1 holds the only finite sample
        out.append((G, Case(f"shard-G{G}-only", only, _noise(rng, K, T, nu), lam)))
        plain = base.copy()  # an ordinary population, for the finite-cost merge
        out.append((G, Case(f"shard-G{G}-plain", plain, _noise(rng, K, T, nu), lam)))
    return out


def all_finite_result_cases():
    """Every case whose reference result is finite (a - e, and g as whole populations)."""
    cs = [wide_spread(K, T, nu, lam, c0) for (K, T, nu) in SHAPES for lam in LAMBDAS for c0 in C0S]
    cs += [ties(K) for K in (1000, 4097)]
    cs += [one_survivor(K, k) for (K, k) in SURVIVORS]
    cs += [padding(K, s) for K in (1000, 17) for s in (1, -1)]
    cs += inf_cases()
    cs += [c for (_, c) in shard_cases()]
    return cs


# ------------------------------------------------------------------ reference
def reference(case):
    """One-level formula in np.longdouble.  Returns dict(beta, x, w, eta, omega, dU) (dU: (T, nu))."""
    c = case.cost.astype(LD)
    lam = LD(case.lam)
    with np.errstate(invalid="ignore", over="ignore"):
        beta = np.min(c)  # propagates NaN, like torch.min
        x = (c - beta) / lam
        w = np.exp(-x)
        eta = np.sum(w)
        omega = w / eta
        # (an absent sample contributes nothing: 0 * noise, noise finite)
        dU = np.einsum("k,ktj->tj", omega, case.noise.astype(LD))
    return dict(beta=beta, x=x, w=w, eta=eta, omega=omega, dU=dU)


def reference_mpmath(case, digits=50):
    """The same formula at `digits` decimal digits (the check of `reference` itself)."""
    import mpmath

    with mpmath.workdps(digits):
        c = [mpmath.mpf(float(v)) for v in case.cost]
        lam = mpmath.mpf(case.lam)
        beta = min(c)
        w = [mpmath.exp(-(v - beta) / lam) for v in c]
        eta = mpmath.fsum(w)
        omega = [v / eta for v in w]
        n = case.noise.reshape(case.K, -1)
        dU = [mpmath.fsum(omega[k] * mpmath.mpf(float(n[k, i])) for k in range(case.K)) for i in range(n.shape[1])]
        return dict(eta=eta, omega=omega, dU=dU)


def bounds(case, ref):
    """(rel, cap, dU_bound): per-sample relative bound where x <= 690 (inf elsewhere), the absolute cap on omega where
    x > 690 (inf elsewhere), and the per-entry bound on dU, as derived in the module docstring."""
    x = ref["x"]
    small = x > X_DENORMAL  # (+inf costs: x = inf)
    xs = np.where(small, LD(0), x)
    rel = np.where(small, LD(np.inf), (4 * xs + 256) * LD(EPS))
    cap_value = np.exp(LD(-680)) / ref["eta"]
    cap = np.where(small, cap_value, LD(np.inf))
    an = np.abs(case.noise.astype(LD))
    per = np.where(small, cap_value, ref["omega"] * (4 * xs + 256) * LD(EPS))
    return rel, cap, np.einsum("k,ktj->tj", per, an)


def check(case, ref, w, omega, dU, what=""):
    """Assert the bound; returns the largest observed error / bound ratio (over w, omega and dU)."""
    rel, cap, dUb = bounds(case, ref)
    w, omega, dU = np.asarray(w, dtype=LD), np.asarray(omega, dtype=LD), np.asarray(dU, dtype=LD).reshape(case.T, case.nu)
    assert np.all(np.isfinite(w.astype(np.float64))) and np.all(np.isfinite(omega.astype(np.float64))), f"{case} {what}: non-finite weight"
    assert np.all(np.isfinite(dU.astype(np.float64))), f"{case} {what}: non-finite dU"
    big = np.isfinite(rel)
    worst = 0.0
    for name, got, want in (("cost_total_non_zero", w, ref["w"]), ("omega", omega, ref["omega"])):
        err = np.abs(got - want)[big]
        bnd = want[big] * rel[big]
        ratio = float(np.max(err / bnd)) if err.size else 0.0
        assert ratio <= 1.0, f"{case} {what}: {name} error / bound = {ratio:.3g}"
        worst = max(worst, ratio)
    lim = cap[~big]
    assert np.all(omega[~big] >= 0) and np.all(omega[~big] <= lim), f"{case} {what}: a weight past x = 690 is not in [0, e^-680/eta]"
    err = np.abs(dU - ref["dU"])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, LD(0), err / dUb)
    ratio = float(np.max(r))
    assert ratio <= 1.0, f"{case} {what}: dU error / bound = {ratio:.3g}"
    return max(worst, ratio)


# ------------------------------------------------------------------ float64 emulation of the three-level fold
def _tile_partials(cost, noise, lam, inf_rule):
    """weight_tile: (beta_b, eta_b, S_b) of every 16-sample tile of one shard."""
    K, TN = noise.shape
    nblk = (K + TILE - 1) // TILE
    pad = nblk * TILE - K
    c = np.concatenate((cost, np.zeros(pad))).reshape(nblk, TILE)
    valid = (np.arange(nblk * TILE) < K).reshape(nblk, TILE)
    n = np.concatenate((noise, np.zeros((pad, TN)))).reshape(nblk, TILE, TN)
    beta = np.where(valid, c, np.inf)
    lane = np.arange(TILE)
    for o in (8, 4, 2, 1):
        beta = np.fmin(beta, beta[:, lane ^ o])  # fmin: a NaN operand is ignored, as on the device
    w = np.exp(-(1.0 / lam) * (c - beta))
    w = np.where(valid, w, 0.0)
    if inf_rule:
        w = np.where(c == np.inf, 0.0, w)
    eta = w.copy()
    for o in (8, 4, 2, 1):
        eta = eta + eta[:, lane ^ o]
    S = np.zeros((nblk, TN))
    for s in range(TILE):
        on = valid[:, s]
        S[on] = S[on] + w[on, s, None] * n[on, s]
    return beta[:, 0], eta[:, 0], S


def _rank_fold(beta_b, eta_b, S_b, lam, inf_rule):
    """weight_beta + weight_chunk + the ascending chunk sum: the shard's (beta_r, eta_r, S_r)."""
    nblk = beta_b.shape[0]
    beta = np.fmin.reduce(beta_b)
    scale = np.exp(-(1.0 / lam) * (beta_b - beta))
    if inf_rule:
        scale = np.where(beta_b == np.inf, 0.0, scale)
    v = np.concatenate((eta_b[:, None], S_b), axis=1)  # entry 0: eta, 1 + tj: S
    tot = np.zeros(v.shape[1])
    for j in range((nblk + CHUNK - 1) // CHUNK):
        waves = []
        for wv in range(4):
            acc = np.zeros(v.shape[1])
            for b in range(j * CHUNK + 16 * wv, min(j * CHUNK + 16 * wv + 16, nblk)):
                acc = acc + scale[b] * v[b]
            waves.append(acc)
        tot = tot + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return beta, tot[0], tot[1:]


def emulate_fold(case, G=1, inf_rule=True):
    """float64 restatement of weight_tile -> weight_chunk / weight_rank -> merge_kernel for G equal shards, U = 0 before the
    update.  Returns dict(beta, eta, w, omega, dU) for the whole population."""
    lam, K, TN = case.lam, case.K, case.T * case.nu
    noise = case.noise.reshape(K, TN)
    Kl = K // G
    assert Kl * G == K
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        parts = [_rank_fold(*_tile_partials(case.cost[g * Kl:(g + 1) * Kl], noise[g * Kl:(g + 1) * Kl], lam, inf_rule), lam, inf_rule)
                 for g in range(G)]
        beta = np.inf
        for (b, _, _) in parts:
            beta = np.fmin(beta, b)

        def scale(b):
            return 0.0 if (inf_rule and b == np.inf) else np.exp(-(b - beta) / lam)

        eta = 0.0
        for (b, e, _) in parts:
            eta = eta + scale(b) * e
        acc = np.zeros(TN)
        for (b, _, S) in parts:
            acc = acc + scale(b) * S
        inv = 1.0 / eta
        dU = 0.0 + inv * acc
        w = np.exp(-(1.0 / lam) * (case.cost - beta))
        omega = inv * w
    return dict(beta=beta, eta=eta, w=w, omega=omega, dU=dU.reshape(case.T, case.nu), parts=parts)
