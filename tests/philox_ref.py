"""An independent statement of the device random streams, for tests/test_philox_host.py (CPU) and
tests/test_gpu_random_streams.py (GPU): Philox4x32-10 from the paper's definition (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11, section 4.3 and table 2) in vectorised NumPy uint64 arithmetic, the 53-bit
uniform, the Box-Muller pair in extended precision, and one function per DOCUMENTED draw.  Every counter here is built from
the documents -- include/nlc.h (nlc_mppi_rollout, nlc_collect_step, nlc_synth_generate), docs/collector.md "Random draws",
docs/synthetic.md's stream table, DESIGN.md's "Philox counters use the global sample index" -- not from the kernels.

Everything broadcasts: the index arguments are Python ints or integer arrays of any (mutually broadcastable) shape.
"""

import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)
# table 2 of the paper: the two multipliers of Philox-4x32 and the Weyl increments of its key schedule (golden ratio, sqrt 3 - 1)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288419716939937510")  # pi to the precision of the extended type


def _u64(x):
    """Integers (Python ints of any sign below 2^64, or arrays) as uint64 arrays."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in x], dtype=np.uint64)
    return np.array(int(x) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def lo32(x):
    return _u64(x) & MASK32


def hi32(x):
    return (_u64(x) >> np.uint64(32)) & MASK32


def philox4x32(counter, key, rounds=10):
    """Philox-4x32-R.  counter (..., 4), key (..., 2): 32-bit words held in uint64 -> (..., 4) words.

    One round (the paper's S-box for N = 4): with (hi, lo) = mulhilo(M, x) the 64-bit product's halves,
        (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0));
    the key is bumped by the Weyl constants between rounds (round r uses k + r W)."""
    c = np.broadcast_arrays(*(_u64(counter[..., i]) for i in range(4)))
    k0, k1 = _u64(key[..., 0]), _u64(key[..., 1])
    c0, c1, c2, c3 = (x & MASK32 for x in c)
    for r in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        kr0 = (k0 + np.uint64(r) * PHILOX_W0) & MASK32
        kr1 = (k1 + np.uint64(r) * PHILOX_W1) & MASK32
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ kr0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ kr1, p0 & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def u53(hi, lo):
    """(hi, lo) -> a double in (0, 1): v = the top 53 bits of the 64-bit word hi:lo, u = (v + 1/2) / 2^53 rounded to
    double, and never 1: the one value of v whose rounding would give 1.0 (v = 2^53 - 1, exact value 1 - 2^-54, a tie between
    1 - 2^-53 and 1) takes the double below 1.  v + 1/2 is exact below 2^52; above, the sum rounds to nearest-even like any
    IEEE addition -- computed here in integers, not by trusting the float addition."""
    v = ((_u64(hi) << np.uint64(32)) | (_u64(lo) & MASK32)) >> np.uint64(11)
    small = v < np.uint64(1 << 52)
    # v + 1/2 for v >= 2^52 is a tie between v and v + 1: the even one
    rounded = np.where(small, v, v + (v & np.uint64(1)))
    rounded = np.minimum(rounded, np.uint64((1 << 53) - 1))
    x = rounded.astype(np.float64) + np.where(small, 0.5, 0.0)  # exact either way
    return x * 2.0 ** -53


def normal_pair(u1, u2):
    """Box-Muller in extended precision: (rad cos(2 pi u2 - pi), rad sin(2 pi u2 - pi)), rad = sqrt(-2 ln u1); also rad."""
    u1, u2 = np.asarray(u1, dtype=LD), np.asarray(u2, dtype=LD)
    rad = np.sqrt(LD(-2) * np.log(u1))
    ang = LD(2) * PI_LD * u2 - PI_LD
    return rad * np.cos(ang), rad * np.sin(ang), rad


def _block(counter, key):
    r = philox4x32(counter, key)
    return u53(r[..., 0], r[..., 1]), u53(r[..., 2], r[..., 3])


def _stack_words(*words):
    return np.stack(np.broadcast_arrays(*(_u64(w) for w in words)), axis=-1)


# ---------------------------------------------------------------------------------------------------- the planner
def planner_counter(kg, t, seed, counter):
    """nlc_mppi_rollout, rng = 1 (include/nlc.h): counter words (kg lo, kg hi, t, command lo), key (seed lo, seed hi ^ command
    hi); kg is the GLOBAL sample index, k_offset + k, and e * K_global + k_offset + k for episode e of a batched planner
    (DESIGN.md).  -> (..., 6) words: four of the counter, two of the key."""
    return _stack_words(lo32(kg), hi32(kg), lo32(t), lo32(counter), lo32(seed), hi32(seed) ^ hi32(counter))


def planner_eps(kg, t, seed, counter, mu, chol, with_rad=False):
    """eps (..., nu) ~ N(mu, L L^T) of global sample kg, horizon step t of command `counter`: one block, u1 from words 0, 1 and
    u2 from words 2, 3, z = the Box-Muller pair, eps_i = mu_i + sum_{j <= i} L_ij z_j (the LOWER factor).  Extended
    precision.  with_rad: also the radius, for the tolerance."""
    w = planner_counter(kg, t, seed, counter)
    u1, u2 = _block(w[..., :4], w[..., 4:])
    z0, z1, rad = normal_pair(u1, u2)
    mu = np.asarray(mu, dtype=LD).reshape(-1)
    L = np.asarray(chol, dtype=LD).reshape(mu.size, mu.size)
    z = (z0, z1)
    eps = np.stack([mu[i] + sum(L[i, j] * z[j] for j in range(i + 1)) for i in range(mu.size)], axis=-1)
    return (eps, rad) if with_rad else eps


# ---------------------------------------------------------------------------------------------------- the collector
COLLECT_INTERVAL, COLLECT_ACTION_NOISE, COLLECT_OBS_NOISE_01, COLLECT_OBS_NOISE_23, COLLECT_RANDOM_POLICY = range(5)


def collector_counter(seed, episode, it, stream):
    """docs/collector.md "Random draws": counter (episode lo, episode hi, step it, stream), key = seed; episode is GLOBAL."""
    return _stack_words(lo32(episode), hi32(episode), lo32(it), lo32(stream), lo32(seed), hi32(seed))


def collector_draws(seed, episode, it):
    """The draws of (global episode, step): `interval` one uniform (stream 0); `action_noise` (..., 2) one uniform per action
    dim (stream 1); `obs_noise` (..., 4) standard normals, components 0, 1 the pair of stream 2 and 2, 3 the pair of stream
    3, with `obs_rad` (..., 4) their radii; `policy` (..., 2) one uniform per action dim (stream 4)."""
    def blk(stream):
        w = collector_counter(seed, episode, it, stream)
        return _block(w[..., :4], w[..., 4:])

    za = normal_pair(*blk(COLLECT_OBS_NOISE_01))
    zb = normal_pair(*blk(COLLECT_OBS_NOISE_23))
    return dict(
        interval=blk(COLLECT_INTERVAL)[0],
        action_noise=np.stack(blk(COLLECT_ACTION_NOISE), axis=-1),
        obs_noise=np.stack([za[0], za[1], zb[0], zb[1]], axis=-1),
        obs_rad=np.stack([za[2], za[2], zb[2], zb[2]], axis=-1),
        policy=np.stack(blk(COLLECT_RANDOM_POLICY), axis=-1),
    )


# ---------------------------------------------------------------------------------------------------- the synthetic dataset
SYNTH_STATE_01, SYNTH_STATE_23, SYNTH_ACTION, SYNTH_INTERVAL, SYNTH_FILL = range(5)


def synth_counter(seed, index, second, stream):
    """docs/synthetic.md "Random draws": counter (index lo, index hi, second index, stream), key = seed."""
    return _stack_words(lo32(index), hi32(index), lo32(second), lo32(stream), lo32(seed), hi32(seed))


def synth_draws(seed, ti, i, j, r, b, reuse):
    """The uniforms of the stream table: `state` (..., 4) at (j, ti), streams 0 and 1; `action` (..., 2) at (i, ti), stream 2;
    `interval` at (0, ti), stream 3; `fill` (..., 2) at (global row r, buffer row b), stream 4.  With `reuse` the state and
    action counters take ti = 0; the interval and the fills do not."""
    def blk(index, second, stream):
        w = synth_counter(seed, index, second, stream)
        return _block(w[..., :4], w[..., 4:])

    tsa = 0 if reuse else ti
    return dict(
        state=np.stack(blk(j, tsa, SYNTH_STATE_01) + blk(j, tsa, SYNTH_STATE_23), axis=-1),
        action=np.stack(blk(i, tsa, SYNTH_ACTION), axis=-1),
        interval=blk(0, ti, SYNTH_INTERVAL)[0],
        fill=np.stack(blk(r, b, SYNTH_FILL), axis=-1),
    )


# ---------------------------------------------------------------------------------------------------- element math and bounds
def box(u, mx):
    """(2 u - 1) * max in double, one rounding per operation (2 u is exact)."""
    return (2.0 * np.asarray(u, dtype=np.float64) - 1.0) * mx


def exp_interval(u, dt):
    """-dt ln u in extended precision."""
    return -LD(dt) * np.log(np.asarray(u, dtype=LD))


def ulp(x):
    """The spacing of doubles at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


NORMAL_TOL = 4e-15  # per standard normal: NORMAL_TOL * max(rad, 1), twice the bound derived from the device's operations


def normal_bound(rad):
    return NORMAL_TOL * np.maximum(np.asarray(rad, dtype=np.float64), 1.0)


def eps_bound(rad, chol, eps):
    """sum_j |L_ij| NORMAL_TOL max(rad, 1) + 4 ulp(|eps_i|) for a coloured planner draw, (..., nu)."""
    L = np.abs(np.asarray(chol, dtype=np.float64))
    L = L.reshape(int(round(L.size ** 0.5)), -1)
    return normal_bound(rad)[..., None] * L.sum(axis=1) + 4 * ulp(eps)
