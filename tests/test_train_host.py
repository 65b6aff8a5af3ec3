"""CPU: the element math of the fused training step (csrc/nlc_train.h), built with g++, against torch on the CPU:
GRU-cell backward (autograd through torch.nn.GRUCell), sphere-map backward (autograd through the reference's expression),
clip_grad_norm_'s coefficient and torch.optim.Adam's element update (weight decay included)."""

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("trainhost") / "libtrain_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "train_host.cpp")])
    return ctypes.CDLL(str(out))


def _call(lib, name, x, ncols_out):
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.shape[0]
    y = np.empty((n, ncols_out), dtype=np.float64)
    f = getattr(lib, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    f(x.ctypes.data, y.ctypes.data, n)
    return y


def _ulp(y, ref):
    return np.abs(y - ref) / np.spacing(np.abs(ref) + 1e-300)


def test_gru_cell_backward_vs_autograd(lib):
    """Given the gates torch.nn.GRUCell computes, the gate / hidden gradients equal autograd's through the cell (a 1-unit
    cell, so every product is one element).  Bound: 1e-15 relative to the gradient's scale (autograd's own chain of the
    same products; the two sides round differently in the last bits)."""
    torch.manual_seed(0)
    n = 4000
    x = torch.randn(n, 1, dtype=torch.float64)
    h = torch.randn(n, 1, dtype=torch.float64) * 0.8
    dh = torch.randn(n, 1, dtype=torch.float64)
    Wi = torch.randn(n, 3, dtype=torch.float64)
    Wh = torch.randn(n, 3, dtype=torch.float64)
    bi = torch.randn(n, 3, dtype=torch.float64)
    bh = torch.randn(n, 3, dtype=torch.float64)
    gi = (Wi * x + bi).requires_grad_()  # input-side pre-activations [r z n] per row
    gh = (Wh * h + bh).requires_grad_()
    hp = h.clone().requires_grad_()
    r = torch.sigmoid(gi[:, 0] + gh[:, 0])
    z = torch.sigmoid(gi[:, 1] + gh[:, 1])
    nn_ = torch.tanh(gi[:, 2] + r * gh[:, 2])
    hnew = (1.0 - z) * nn_ + z * hp[:, 0]
    hnew.backward(dh[:, 0])
    inp = torch.stack([dh[:, 0], r.detach(), z.detach(), nn_.detach(), gh[:, 2].detach(), h[:, 0]], dim=1).numpy()
    out = _call(lib, "nlc_t_gru_cell_bwd", inp, 5)
    ref = np.stack([gi.grad[:, 0], gi.grad[:, 1], gi.grad[:, 2], gh.grad[:, 2], hp.grad[:, 0]], axis=1)
    # hidden side r / z gradients equal the input side's
    np.testing.assert_allclose(gh.grad[:, :2].numpy(), gi.grad[:, :2].numpy(), rtol=0, atol=0)
    scale = np.abs(ref).max(axis=0) + 1e-300
    assert (np.abs(out - ref) / scale).max() <= 1e-15


def test_sphere_map_backward_vs_autograd(lib):
    """theta = tanh(o) pi, phi = tanh(o) pi / 2 - pi/2 + pi/2 (w_nl.py:59-62): the pre-activation gradients equal autograd's
    to 4 ulp of g * pi (the factor 1 - y^2 cancels near saturation, and torch's CPU kernel may contract it to an FMA: the
    bound is on the scale of the product, not on the cancelled result)."""
    torch.manual_seed(1)
    o = (torch.randn(20000, dtype=torch.float64) * 3).requires_grad_()
    g = torch.randn(20000, dtype=torch.float64)
    y = torch.tanh(o)
    th = y * torch.pi
    th.backward(g)
    ref_t = o.grad.clone()
    o.grad = None
    phi_scale = torch.pi / 2.0 - -torch.pi / 2.0
    ph = torch.tanh(o) * phi_scale / 2.0 - torch.pi / 2.0 + phi_scale / 2.0
    ph.backward(g)
    ref_p = o.grad.clone()
    out = _call(lib, "nlc_t_sphere_bwd", np.stack([g.numpy(), y.detach().numpy()], axis=1), 2)
    sc = np.spacing(np.abs(g.numpy()) * np.pi)
    assert (np.abs(out[:, 0] - ref_t.numpy()) / sc).max() <= 4
    assert (np.abs(out[:, 1] - ref_p.numpy()) / sc).max() <= 4


def test_clip_coefficient_vs_clip_grad_norm(lib):
    """clip_grad_norm_ multiplies by min(1, max_norm / (total + 1e-6)): a one-element gradient of value `total` (its own
    norm) clipped by torch equals total * the host coefficient to 2 ulp (active and inactive; torch's division may round the
    coefficient one ulp differently)."""
    rng = np.random.default_rng(2)
    rows = []
    for total in np.concatenate([rng.uniform(1e-3, 10, 200), [0.05, 0.1, 0.1000001, 1e6]]):
        for max_norm in (0.1, 1.0):
            p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
            p.grad = torch.tensor([float(total)], dtype=torch.float64)
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            rows.append((max_norm, total, float(p.grad[0])))
    rows = np.array(rows)
    out = _call(lib, "nlc_t_clip_coef", rows[:, :2], 1)[:, 0]
    assert _ulp(out * rows[:, 1], rows[:, 2]).max() <= 2
    assert out.max() == 1.0 and out.min() < 1.0


def test_fourier_query_points_and_prediction_factor_vs_numpy(lib):
    """fourier_query_point / fourier_pred_factor (both NL kernels call them) against the same float64 expressions in numpy
    (torchlaplace's Fourier series at scale 2: T = 2 t, gamma = alpha - log(tol) / (2 T), s_k = gamma + i pi k / T, the
    prediction's e^{gamma t} / T), at the models' alpha = 1e-3 and tol = 1e-9.  The arithmetic is the same in the same order,
    so the two differ by their atan2 / asin / exp only: 4 ulp of the result (each library's is within 1; exp's argument
    gamma t is below 6 here, so its rounding adds at most 1 more)."""
    alpha, log_tol = 1e-3, float(np.log(1e-9))
    t = np.array([0.05, 1.0, 7.3])
    k = np.array([0, 1, 16, 128], dtype=np.int32)
    th, ph, fac = np.empty((3, 4)), np.empty((3, 4)), np.empty(3)
    f = lib.nlc_t_fourier
    vp = ctypes.c_void_p
    f.argtypes = [ctypes.c_double, ctypes.c_double, vp, ctypes.c_long, vp, ctypes.c_int, vp, vp, vp]
    f(alpha, log_tol, t.ctypes.data, 3, k.ctypes.data, 4, th.ctypes.data, ph.ctypes.data, fac.ctypes.data)
    T = 2.0 * t
    gamma = alpha - log_tol / (2.0 * T)
    im = np.pi * k.astype(np.float64)[None, :] / T[:, None]
    a2 = gamma[:, None] * gamma[:, None] + im * im
    refs = (np.arctan2(im, np.broadcast_to(gamma[:, None], im.shape)), np.arcsin((a2 - 1.0) / (a2 + 1.0)), np.exp(gamma * t) / T)
    for got, ref in zip((th, ph, fac), refs):
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= 4 * np.spacing(np.abs(ref))).all(), (got, ref)
    assert (th[:, 0] == 0.0).all() and (th[:, 1:] > 0.0).all()  # k = 0 is the real axis


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_element_vs_torch_adam(lib, wd):
    """Three torch.optim.Adam steps (foreach off and on give the same element formula) against the host element update
    with the host-side scalars of nlc_train_step: parameters and exp_avg_sq to 4 ulp; exp_avg to 4 ulp of |exp_avg| + max |g|
    over the steps (the lerp m + w (g - m) cancels when g and m have opposite signs)."""
    torch.manual_seed(3)
    n = 5000
    p0 = torch.randn(n, dtype=torch.float64)
    grads = [torch.randn(n, dtype=torch.float64) * 10.0 ** torch.randint(-9, 2, (n,)).double() for _ in range(3)]
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    state = np.ascontiguousarray(np.stack([p0.numpy(), np.zeros(n), np.zeros(n)], axis=1))
    f = lib.nlc_t_adam
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    for step, g in enumerate(grads, start=1):
        p.grad = g.clone()
        opt.step()
        bc1, bc2 = 1 - b1**step, 1 - b2**step
        k = np.array([wd, 1 - b1, b2, 1 - b2, (lr / bc1) * -1, bc2**0.5, eps])
        gn = np.ascontiguousarray(g.numpy())
        f(state.ctypes.data, gn.ctypes.data, k.ctypes.data, n)
    st = opt.state[p]
    assert _ulp(state[:, 0], p.detach().numpy()).max() <= 4
    m_ref = st["exp_avg"].numpy()
    assert (np.abs(state[:, 1] - m_ref) / np.spacing(np.abs(m_ref) + np.abs(torch.stack(grads).numpy()).max(axis=0) + wd * np.abs(p0.numpy()))).max() <= 4
    assert _ulp(state[:, 2], st["exp_avg_sq"].numpy()).max() <= 4


@pytest.mark.parametrize("foreach", [False, True])
def test_adam_element_other_lerp_branch_and_large_eps(lib, foreach):
    """beta1 = 0.3 makes the lerp weight 1 - beta1 = 0.7 >= 0.5, torch.lerp's other branch (end - (end - self)(1 - w)),
    which the default betas never take; eps = 1e-2 is large against sqrt(v) for many elements; weight decay on; 10 steps of
    torch.optim.Adam.  Each step is checked from torch's own state before it (so roundoff does not compound over the steps;
    every step's bias corrections are exercised).  Bounds in ulp of the terms' magnitudes, not of the results, because torch's
    CPU kernels may contract g + wd p and the lerp into FMAs and both cancel: exp_avg_sq to 8 ulp of b2 |v| + (1 - b2) G^2
    (one ulp of G in the decayed gradient is two of G^2),
    exp_avg to 4 ulp of |exp_avg| + G, the parameter to 4 ulp of |p| + |its update| (G = |g| + wd |p|)."""
    torch.manual_seed(4)
    n = 5000
    p0 = torch.randn(n, dtype=torch.float64)
    grads = [torch.randn(n, dtype=torch.float64) * 10.0 ** torch.randint(-7, 2, (n,)).double() for _ in range(10)]
    lr, b1, b2, eps, wd = 1e-3, 0.3, 0.95, 1e-2, 1e-2
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=foreach)
    f = lib.nlc_t_adam
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    eps_dominated = 0.0
    for step, g in enumerate(grads, start=1):
        st = opt.state.get(p)
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n)
        pre = p.detach().numpy().copy()
        state = np.ascontiguousarray(np.stack([pre, m0, v0], axis=1))
        p.grad = g.clone()
        opt.step()
        bc1, bc2 = 1 - b1**step, 1 - b2**step
        k = np.array([wd, 1 - b1, b2, 1 - b2, (lr / bc1) * -1, bc2**0.5, eps])
        assert k[1] >= 0.5
        gn = np.ascontiguousarray(g.numpy())
        f(state.ctypes.data, gn.ctypes.data, k.ctypes.data, n)
        st = opt.state[p]
        p_ref, m_ref, v_ref = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        geff = np.abs(gn) + wd * np.abs(pre)
        assert (np.abs(state[:, 2] - v_ref) / np.spacing(b2 * v0 + (1 - b2) * geff * geff)).max() <= 8, step
        assert (np.abs(state[:, 1] - m_ref) / np.spacing(np.abs(m_ref) + geff)).max() <= 4, step
        assert (np.abs(state[:, 0] - p_ref) / np.spacing(np.abs(pre) + np.abs(p_ref - pre))).max() <= 4, step
        eps_dominated = max(eps_dominated, float((np.sqrt(v_ref) / bc2**0.5 < eps).mean()))
    # the large eps dominates the denominator for a good share of the elements: not the default regime
    assert eps_dominated > 0.1


# every (d, nin, h, S) nlc_set_model accepts for a Fourier model: d 1..6, nin 1..3, h 64 / 128 / 256, S 1..129 (the ILT
# tables) with the last layer's 2 d S outputs in at most 25 output tiles (nlc_pack.h ilt_tiles_needed, nl_pick_nt3)
def _ilt_tiles_needed(d, S):
    n_even, n_odd = d * ((S + 1) // 2), d * (S // 2)
    return ((n_even + 3) // 4 + (n_odd + 3) // 4 + 1) // 2


def _accepted_shapes():
    for d in range(1, 7):
        for nin in (1, 2, 3):
            for h in (64, 128, 256):
                for S in range(1, 130):
                    if _ilt_tiles_needed(d, S) <= 25:
                        yield d, nin, h, S


_FIELDS = ["X0", "H0", "G0", "H1", "G1", "a0", "a1", "a2", "u", "d3", "d2", "d1", "denc", "tn", "tgt", "sq", "DI0", "DH0",
           "DI1", "DH1", "DX1", "dhA", "dD"]


def _extents(d, nin, g, h, S, B):
    """Doubles each slab array is indexed over by train_fwd_bwd_kernel (R = 16 rows, K0 = 2S + d + 2, O = 2dS)."""
    R, K0, O = 16, 2 * S + d + 2, 2 * d * S
    return dict(X0=B * R * nin, H0=(B + 1) * R * g, G0=B * R * 4 * g, H1=(B + 1) * R * g, G1=B * R * 4 * g, a0=R * K0,
                a1=R * h, a2=R * h, u=R * O, d3=R * O, d2=R * h, d1=R * h, denc=R * 2, tn=R, tgt=R * d, sq=R * d,
                DI0=B * R * 3 * g, DH0=B * R * 3 * g, DI1=B * R * 3 * g, DH1=B * R * 3 * g, DX1=B * R * g, dhA=R * g, dD=R * g)


def test_act_layout_aligned_disjoint_and_within_the_slab(lib):
    """The per-workgroup slab of the fused step (nlc_train.h act_layout): for every accepted (d, nin, h, S) and every window
    B in 1..16, each array starts on an 8-double boundary, the arrays (at the extents the kernel indexes) do not overlap and
    end inside total(B), and total(B) <= total(16) -- abi_train.hip's plan_of sizes every workgroup's slab for B = 16, so a
    shorter window must not reach into the next workgroup's."""
    f = lib.nlc_t_act_layout
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    out = np.zeros(24, dtype=np.int64)
    n_shapes = 0
    for d, nin, h, S in _accepted_shapes():
        g = h // 2
        f(d, nin, g, h, S, 16, out.ctypes.data)
        total16 = int(out[23])
        for B in range(1, 17):
            f(d, nin, g, h, S, B, out.ctypes.data)
            ext = _extents(d, nin, g, h, S, B)
            spans = sorted((int(out[i]), int(out[i]) + ext[k], k) for i, k in enumerate(_FIELDS))
            where = f"d={d} nin={nin} h={h} S={S} B={B}"
            assert all(o % 8 == 0 for o, _, _ in spans), where
            assert spans[0][0] == 0, where
            for (o0, e0, k0), (o1, _, k1) in zip(spans, spans[1:]):
                assert e0 <= o1, f"{where}: {k0} [{o0}, {e0}) runs into {k1} at {o1}"
            assert spans[-1][1] <= int(out[23]) <= total16, where
        n_shapes += 1
    assert n_shapes == 3 * 3 * (129 + 100 + 66 + 50 + 40 + 33)


def test_blob_offsets_match_the_state_dict(lib):
    """nlc_train.h blob_offsets (where the kernels read each weight and write each gradient) against the sizes of the
    reference architecture's tensors in state_dict order, at a spread of accepted shapes."""
    from oracle import nl_model as onl

    f = lib.nlc_t_blob_offsets
    f.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    out = np.zeros(17, dtype=np.int64)
    for d, nu, enc, h, S in [(1, 1, False, 64, 129), (2, 2, True, 128, 4), (4, 3, False, 64, 13), (6, 2, False, 256, 33),
                             (5, 1, True, 128, 17)]:
        sd = onl.make_synthetic_state_dict(0, d, nu, h, S, encode_obs_time=enc)
        sizes = [v.numel() for k, v in sd.items() if k.startswith(("action_encoder.", "laplace_rep_func."))]
        f(d, nu + int(enc), h // 2, h, S, out.ctypes.data)
        assert len(sizes) == 16
        assert list(np.diff(out)) == sizes, (d, nu, enc, h, S)


_T, _CHUNK = 16, 1024  # kTensors, kChunk


def _offsets(sizes):
    assert len(sizes) == _T
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _chunk_tables(lib):
    """name -> off[0..16]: the NL table at d = 5, nin = 2, h = 64, S = 17; the RNN table (six tensors, ten empty) at H = 64;
    a synthetic table over the sizes around the chunk length, the empty tensor first and the ten spare slots empty."""
    out = np.zeros(_T + 1, dtype=np.int64)
    tables = {}
    f = lib.nlc_t_blob_offsets
    f.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    f(5, 2, 32, 64, 17, out.ctypes.data)
    tables["nl"] = out.copy()
    f = lib.nlc_t_rnn_blob_offsets
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    f(5, 2, 64, 1, out.ctypes.data)
    tables["rnn"] = out.copy()
    assert (np.diff(tables["rnn"])[6:] == 0).all() and (np.diff(tables["rnn"])[:6] > 0).all()
    tables["synthetic"] = _offsets([0, 1, 1023, 1024, 1025, 2049] + [0] * 10)
    return tables


def _chunk_ranges(lib, off):
    f = lib.nlc_t_chunk_ranges
    f.argtypes = [ctypes.c_void_p] * 3
    f.restype = ctypes.c_int
    off = np.ascontiguousarray(off, dtype=np.int64)
    cstart = np.zeros(_T + 1, dtype=np.int32)
    n = f(off.ctypes.data, cstart.ctypes.data, None)
    rng = np.zeros((n, 3), dtype=np.int64)
    assert f(off.ctypes.data, cstart.ctypes.data, rng.ctypes.data) == n == cstart[_T]
    return cstart, rng


def _clip_total(lib, off, grad):
    f = lib.nlc_t_clip_total
    f.argtypes = [ctypes.c_void_p] * 3
    f.restype = ctypes.c_double
    off = np.ascontiguousarray(off, dtype=np.int64)
    grad = np.ascontiguousarray(grad, dtype=np.float64)
    assert grad.size == off[_T]
    sq = np.zeros(max(1, int(np.sum((np.diff(off) + _CHUNK - 1) // _CHUNK))), dtype=np.float64)
    return f(off.ctypes.data, grad.ctypes.data, sq.ctypes.data), sq


def test_chunk_range_tiles_the_blob_tensor_by_tensor(lib):
    """nlc_train.h chunk_range over a ChunkTable (what train_reduce_kernel and both Adam kernels call): every chunk b in
    [0, cstart[kTensors]) maps to one tensor; its range is non-empty and at most kChunk long; the ranges tile [0, P) in order
    with no gap or overlap; none straddles a tensor; an empty tensor owns none."""
    for name, off in _chunk_tables(lib).items():
        cstart, rng = _chunk_ranges(lib, off)
        sizes = np.diff(off)
        assert list(np.diff(cstart)) == [int(-(-n // _CHUNK)) for n in sizes], name
        P, pos, owners = int(off[_T]), 0, np.zeros(_T, dtype=np.int64)
        for b, (t, e0, e1) in enumerate(rng):
            where = f"{name} chunk {b}"
            assert 0 <= t < _T and cstart[t] <= b < cstart[t + 1], where
            assert 0 < e1 - e0 <= _CHUNK, where
            assert e0 == pos, where  # in order, no gap, no overlap
            assert off[t] <= e0 and e1 <= off[t + 1], where  # inside tensor t
            pos = int(e1)
            owners[t] += 1
        assert pos == P, name
        assert ((owners == 0) == (sizes == 0)).all(), name


def test_clip_total_norm_vs_clip_grad_norm(lib):
    """nlc_train.h clip_total_norm on chunk sums of squares formed as train_reduce_kernel forms them, against the total
    torch.nn.utils.clip_grad_norm_ returns for the same tensors: 2 ulp, the bound of the clip coefficient above."""
    rng = np.random.default_rng(5)
    for name, off in _chunk_tables(lib).items():
        grad = rng.standard_normal(int(off[_T])) * 10.0 ** rng.integers(-3, 2, int(off[_T]))
        total, _ = _clip_total(lib, off, grad)
        params = []
        for i in range(_T):
            p = torch.nn.Parameter(torch.zeros(int(off[i + 1] - off[i]), dtype=torch.float64))
            p.grad = torch.from_numpy(grad[off[i] : off[i + 1]].copy())
            params.append(p)
        ref = float(torch.nn.utils.clip_grad_norm_(params, 1.0))
        print(f"{name}: total {total!r} torch {ref!r} ulp {float(_ulp(np.float64(total), np.float64(ref)))}")
        assert _ulp(np.float64(total), np.float64(ref)) <= 2, name


def test_clip_total_norm_ignores_empty_tensors_bit_for_bit(lib):
    """What the RNN and NODE tables' padding relies on: the total of a table with empty tensors has the bits of the total
    without them -- the same tensors with the empty ones moved (between, in front, behind), and the same sums with no empty
    tensor at all, restated here over the non-empty tensors only."""
    rng = np.random.default_rng(6)
    for name, off in _chunk_tables(lib).items():
        sizes = [int(n) for n in np.diff(off)]
        full = [n for n in sizes if n]
        pad = _T - len(full)
        grad = rng.standard_normal(int(off[_T]))
        total, sq = _clip_total(lib, off, grad)
        # the non-empty tensors alone: their chunks' sums in order, sqrt, squared again, summed in tensor order
        tot2, c = np.float64(0.0), 0
        for n in full:
            s = np.float64(0.0)
            for _ in range(-(-n // _CHUNK)):
                s = s + sq[c]
                c += 1
            r = np.sqrt(s)
            tot2 = tot2 + r * r
        assert c == sq.size or not full
        assert float(np.sqrt(tot2)).hex() == total.hex(), name
        if not pad:
            continue
        # the same tensors in the same order, the empty ones elsewhere
        for lay in (full + [0] * pad, [0] * pad + full, [x for n in full for x in (n, 0)][: 2 * pad] + full[pad:]):
            lay = (lay + [0] * _T)[:_T]
            assert [n for n in lay if n] == full, name
            other, sq2 = _clip_total(lib, _offsets(lay), grad)
            assert (sq2 == sq).all() and other.hex() == total.hex(), (name, lay)


def test_blockwise_comparator_catches_what_the_per_tensor_scale_hides():
    """tests/train_compare.py: an autograd gradient of the oracle's loss for a model whose layer-0 reset gate is saturated
    (its input bias shifted by +8: r(1 - r) ~ 3e-4), so the r block of weight_ih_l0 is orders of magnitude below the n block.
    An error of 1e-7 of that block's own max, put into one element, fails the block-wise comparison at the GPU tests' 1e-9,
    while the earlier per-tensor scale passes it; the unperturbed gradient passes both."""
    import train_compare as tc
    from oracle import nl_model as onl

    d, nu, h, S, B, N = 2, 1, 64, 5, 3, 8
    g = h // 2
    sd = onl.make_synthetic_state_dict(5, d, nu, h, S, [1.0, 2.0], [1.5], tame=True)
    sd["action_encoder.gru.bias_ih_l0"][:g] += 8.0
    gen = torch.Generator().manual_seed(0)
    s0 = torch.randn(N, d, dtype=torch.float64, generator=gen)
    a0 = torch.rand(N, B, nu, dtype=torch.float64, generator=gen) * 2 - 1
    ts = torch.rand(N, 1, dtype=torch.float64, generator=gen) * 0.08 + 0.02
    tgt = torch.randn(N, d, dtype=torch.float64, generator=gen) * 0.05
    leaves = {k: (v.clone().requires_grad_() if k.startswith(("action_encoder.", "laplace_rep_func.")) else v)
              for k, v in sd.items()}
    ((onl.nl_forward(leaves, s0, a0, ts, S=S).reshape(N, d) - tgt) ** 2).mean().backward()
    name = "action_encoder.gru.weight_ih_l0"
    ref = leaves[name].grad.clone()
    block = ref[:g]
    ratio = float(block.abs().max()) / float(ref.abs().max())
    assert ratio < 1e-2, f"r block is {ratio:.2e} of the tensor: not the regime this test needs"
    bad = ref.clone()
    i = int(block.abs().argmax())
    bad[i] += 1e-7 * float(block.abs().max())
    tc.assert_grad_close(name, ref.clone(), ref, 1e-9)
    assert tc.per_tensor_close(ref.clone(), ref, 1e-9)
    assert tc.per_tensor_close(bad, ref, 1e-9), "the per-tensor scale was expected to miss this error"
    with pytest.raises(AssertionError, match=r"weight_ih_l0\[r\]"):
        tc.assert_grad_close(name, bad, ref, 1e-9)
    # the same for the phi half of the last layer when its theta half dominates
    name = "laplace_rep_func.linear_tanh_stack.4.bias"
    ref = leaves[name].grad.clone()
    ref[d * S :] *= 1e-4  # a phi half four orders below the theta half
    bad = ref.clone()
    bad[-1] += 1e-7 * float(ref[d * S :].abs().max())
    assert tc.per_tensor_close(bad, ref, 1e-9)
    with pytest.raises(AssertionError, match=r"\[phi\]"):
        tc.assert_grad_close(name, bad, ref, 1e-9)
