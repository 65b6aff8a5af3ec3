"""CPU: the planner host's pure decisions (csrc/nlc_plan.h), built with g++: the pinned block's layout, the fused body's
schedule, the staged step chain's partition, the chunk clamp and the de Hoog calibration's decision rule, each against the
formula the planner host used before they were gathered there (restated here in Python) and against the tables measured on
the MI355X that the schedule's comments quote."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("planhost") / "libplan_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", str(out),
                           os.path.join(HERE, "helpers", "plan_host.cpp")])
    return ctypes.CDLL(str(out))


# ---------------------------------------------------------------------------------------------------------- pinned block
def _pin(lib, E, d, B, nu, T):
    out = (ctypes.c_long * 7)()
    lib.nlc_p_pin_layout(E, d, B, nu, T, out)
    return dict(zip(["state", "abuf", "action", "giveup", "seq", "merge_status", "total"], list(out)))


@pytest.mark.parametrize("E,d,B,nu,T", [(1, 3, 1, 1, 1), (1, 6, 4, 2, 40), (5, 5, 16, 1, 7)])
def test_pin_layout_equals_the_earlier_formulas(lib, E, d, B, nu, T):
    """Offsets (in doubles) as nlc_mppi_configure / nlc_mppi_rollout / nlc_mppi_finish each computed them: staging at 0 and
    E d, the action behind the staged action buffer, the give-up word behind the (E, T, nu) action rows, the sequence word one
    and the merge status word two doubles further, and 8 doubles of tail in the total."""
    p = _pin(lib, E, d, B, nu, T)
    un = E * T * nu
    timeout_word = E * d + E * B * nu + E * T * nu
    assert p["state"] == 0
    assert p["abuf"] == E * d
    assert p["action"] == E * d + E * B * nu
    assert p["giveup"] == timeout_word
    assert p["seq"] == timeout_word + 1
    assert p["merge_status"] == timeout_word + 2
    assert p["total"] == E * d + E * B * nu + un + 8
    # regions (extent in doubles; the control words are one double each) do not overlap and end inside the block
    spans = sorted([(p["state"], E * d), (p["abuf"], E * B * nu), (p["action"], un), (p["giveup"], 1), (p["seq"], 1),
                    (p["merge_status"], 1)])
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1
    assert spans[-1][0] + spans[-1][1] <= p["total"]
    # offsets are in doubles from a page-aligned base: every control word is 8-byte aligned
    for k in ("giveup", "seq", "merge_status"):
        assert (p[k] * 8) % 8 == 0


# --------------------------------------------------------------------------------------------------------- fused schedule
_FUSED = ["built", "bpc", "ntk", "n_enc", "roll_cap", "adaptive_q8", "pool_wgs", "chain_first_tiles", "partner_tiles", "grid"]


def _fused(lib, K, T=40, ncu=256, h=128, occ=(4, 3), bpc=0, roll_cap=0, first=-1, partner=-2, ratio=0.0):
    out = (ctypes.c_int * 10)()
    knobs = (ctypes.c_int * 4)(bpc, roll_cap, first, partner)
    lib.nlc_p_fused_schedule(ncu, ctypes.c_long(K), T, h, occ[0], occ[1], knobs, ctypes.c_double(ratio), out)
    return dict(zip(_FUSED, list(out)))


def _partner_before(K, T, ncu, built, roll_cap_opt=0):
    """The partner-tile fit as rollout_nl_fused spelled it out (C's (int) truncates towards zero)."""
    ntk = (K + 15) // 16
    roll_cap = min(roll_cap_opt if roll_cap_opt > 0 else ncu, ntk)
    f_chain = roll_cap / ncu
    extra = (16.0 * f_chain - 4.5) * T / 40.0
    auto = 1 + (int(extra) if extra > 0 else 0)
    if built <= 3:
        m3 = 1.0 if f_chain <= 0.3125 else 1.0 + 26.7 * (f_chain - 0.3125)
        auto = int(1.0 + (m3 - 1.0) * T / 40.0)
    return auto if roll_cap <= ncu // 2 else -1


def test_fused_schedule_reproduces_the_measured_tables(lib):
    """256 CUs, T = 40: the best schedules measured on the MI355X (profiles/r2_fused_small_shard.md), as the comments of
    fused_schedule quote them."""
    for K, M in [(1024, 1), (1536, 2), (1792, 3), (2048, 4)]:
        s = _fused(lib, K, bpc=4)
        assert (s["built"], s["bpc"], s["partner_tiles"]) == (4, 4, M), K
    for K, M in [(512, 1), (1024, 1), (1280, 1), (1536, 2), (1792, 4), (2048, 6)]:
        s = _fused(lib, K)  # auto: chains on at most half of the CUs -> the 3-per-CU instance
        assert (s["built"], s["bpc"], s["partner_tiles"]) == (3, 3, M), K
        assert s["ntk"] == K // 16 and s["n_enc"] == 40 * s["ntk"] and s["roll_cap"] == s["ntk"]
        assert s["grid"] == 256 * 3 and s["pool_wgs"] == (256 - s["ntk"]) * 3
        assert s["chain_first_tiles"] == 1 and s["adaptive_q8"] == 0


@pytest.mark.parametrize("T", [20, 40, 80])
def test_fused_schedule_scales_with_the_horizon(lib, T):
    for bpc in (3, 4):
        for K in (512, 1024, 1280, 1536, 1792, 2048):
            assert _fused(lib, K, T=T, bpc=bpc)["partner_tiles"] == _partner_before(K, T, 256, bpc), (T, bpc, K)


def test_fused_schedule_caps_instances_and_overrides(lib):
    # roll_cap: the option, clamped to the tile count; the default is one chain per tile, at most one per CU
    assert _fused(lib, 2048, roll_cap=64)["roll_cap"] == 64
    assert _fused(lib, 160, roll_cap=64)["roll_cap"] == 10
    assert _fused(lib, 8192)["roll_cap"] == 256
    # chains on more than half of the CUs: partners never sleep; the auto instance is then the 4-per-CU one
    s = _fused(lib, 2064)
    assert (s["built"], s["roll_cap"], s["partner_tiles"]) == (4, 129, -1)
    assert _fused(lib, 4096, partner=5)["partner_tiles"] == -1
    # explicit partner tiles, "never", and the chain's own first tiles
    assert _fused(lib, 1024, partner=7)["partner_tiles"] == 7
    assert _fused(lib, 1024, partner=-1)["partner_tiles"] == -1
    assert _fused(lib, 1024, first=3)["chain_first_tiles"] == 3
    # the adaptive rule: one tile first, the ratio in 1/256ths, also with chains on more than half of the CUs; an explicit
    # partner count switches it off
    s = _fused(lib, 2048, ratio=1.5)
    assert (s["adaptive_q8"], s["partner_tiles"]) == (384, 1)
    assert _fused(lib, 4096, ratio=1.5)["partner_tiles"] == 1
    s = _fused(lib, 2048, ratio=1.5, partner=2)
    assert (s["adaptive_q8"], s["partner_tiles"]) == (0, 2)
    # the 3-per-CU instance needs three resident workgroups; what is resident bounds the launch
    s = _fused(lib, 1024, occ=(4, 2))
    assert (s["built"], s["bpc"], s["grid"]) == (4, 4, 1024)
    s = _fused(lib, 1024, occ=(2, 3), bpc=4)
    assert (s["built"], s["bpc"], s["grid"]) == (4, 2, 512)
    # hidden_units 256: one instance, two workgroups per CU
    s = _fused(lib, 1024, h=256, occ=(2, 2))
    assert (s["built"], s["bpc"], s["grid"]) == (2, 2, 512)
    assert s["partner_tiles"] == _partner_before(1024, 40, 256, 2)


# ------------------------------------------------------------------------------------------------------- staged partition
def _parts_before(KE, P):
    """rollout_nl_staged's loop."""
    P = min(P, 4)
    while P > 1 and KE // P < 1024:
        P -= 1
    per = ((KE // P) + 63) // 64 * 64
    off, n = [], []
    for h in range(P):
        o = h * per if h * per < KE else KE
        off.append(o)
        n.append(KE - o if h == P - 1 else (per if o + per <= KE else KE - o))
    return P, off, n


@pytest.mark.parametrize("KE", [64, 1000, 1024, 2047, 8192, 16400])
def test_staged_partition(lib, KE):
    for req in (1, 2, 3, 4):
        out = (ctypes.c_long * 9)()
        lib.nlc_p_staged_partition(ctypes.c_long(KE), req, out)
        P, off, n = out[0], list(out[1:5]), list(out[5:9])
        assert 1 <= P <= req and (P == 1 or KE // P >= 1024)
        assert P == req or KE // (P + 1) < 1024  # shrinks only while a part would fall below 1024 samples
        at = 0
        for h in range(P):  # contiguous, covering [0, KE)
            assert off[h] == at and n[h] >= 0
            at += n[h]
            if h < P - 1:
                assert n[h] % 64 == 0
        assert at == KE
        assert (P, off[:P], n[:P]) == _parts_before(KE, req)


def test_horizon_chunk_clamp(lib):
    """At least one chunk (0 = the option's "off"), at most eight and one per step; Tc = ceil(T / C)."""
    out = (ctypes.c_int * 2)()
    for T in (1, 3, 7, 8, 10, 40):
        for req in range(0, 9):
            lib.nlc_p_horizon_chunks(req, T, out)
            C = max(1, min(req, T, 8))
            assert (out[0], out[1]) == (C, (T + C - 1) // C), (T, req)


# ---------------------------------------------------------------------------------------------------- de Hoog calibration
def _pick(lib, n, ncand, elapsed, ms):
    a = np.ascontiguousarray(ms, dtype=np.float32)
    assert a.shape == (3, 2)
    lib.nlc_p_dehoog_pick.restype = ctypes.c_int
    return lib.nlc_p_dehoog_pick(n, ncand, ctypes.c_double(elapsed), a.ctypes.data_as(ctypes.c_void_p))


def test_dehoog_calibration_rule(lib):
    big = 1e30
    ms = [[3.0, 2.5], [2.0, 9.0], [2.25, 2.125]]
    for ncand in (2, 3):
        # no choice before four rounds AND half a second, and only between rounds
        for n in range(0, 4 * ncand):
            assert _pick(lib, n, ncand, 100.0, ms) == -1
        assert _pick(lib, 4 * ncand, ncand, 0.49, ms) == -1
        assert _pick(lib, 4 * ncand + 1, ncand, 100.0, ms) == -1
        assert _pick(lib, 63 * ncand, ncand, 0.49, ms) == -1
        # the candidate whose faster of the last two rounds is smallest
        assert _pick(lib, 4 * ncand, ncand, 0.5, ms) == 1
        # forced at 64 rounds whatever the clock says
        assert _pick(lib, 64 * ncand, ncand, 0.0, ms) == 1
    assert _pick(lib, 12, 3, 1.0, [[3.0, 2.5], [2.75, 9.0], [2.25, 2.125]]) == 2
    assert _pick(lib, 8, 2, 1.0, [[3.0, 2.5], [2.75, 9.0], [2.25, 2.125]]) == 0  # the third is no candidate
    # ties go to the lowest index; nothing measured (all 1e30) is candidate 0
    assert _pick(lib, 12, 3, 1.0, [[2.0, 5.0], [7.0, 2.0], [2.0, 2.0]]) == 0
    assert _pick(lib, 12, 3, 1.0, [[big, big]] * 3) == 0
    assert _pick(lib, 12, 3, 1.0, [[big, big], [big, 4.0], [4.0, big]]) == 1
