// The planner host's pure decisions (abi_planner.hip, abi_planner_nl.hip): functions of a few integers, no HIP, so that
// tests/helpers/plan_host.cpp compiles them with g++ and tests/test_plan_host.py checks them without a GPU --
//   pin_layout        the pinned (host-coherent) block of a configured planner
//   horizon_chunks    GRU encode in horizon chunks: the clamp of C and the chunk length
//   staged_partition  the staged step chain's population in parts, one per stream
//   dehoog_pick       the decision rule of the de Hoog chain-form calibration
//   fused_schedule    role assignment of the one-launch fused body
#pragma once
#include <cstddef>
#include <cstdint>

namespace nlc {
namespace plan {

// ---- pinned block, in doubles: per-command staging of state (E, d) and action_buffer (E, B, nu), the action the merge kernel
// stores (E, T, nu; the first u_per_command rows are used), then the tail of control words the kernels write --
//   giveup        unsigned: a rollout workgroup of the fused body gave up waiting for an encoder tile
//   seq           unsigned long long: sequence number the merge kernel stores behind the action (host_spin)
//   merge_status  unsigned: the merge kernel met a partial row marked invalid
constexpr size_t kPinTail = 8;  // doubles; three words in use
struct PinLayout {
  size_t state, abuf, action, giveup, seq, merge_status, total;
};
inline PinLayout pin_layout(int E, int d, int B, int nu, int T) {
  PinLayout p{};
  p.state = 0;
  p.abuf = p.state + (size_t)E * d;
  p.action = p.abuf + (size_t)E * B * nu;
  p.giveup = p.action + (size_t)E * T * nu;
  p.seq = p.giveup + 1;
  p.merge_status = p.giveup + 2;
  p.total = p.giveup + kPinTail;
  return p;
}

// ---- GRU encode in C horizon chunks of Tc steps (options "horizon_chunks", "dehoog_gru_chunks"; 0 = off): at most one
// chunk per step and eight in all
struct Chunks {
  int C, Tc;
};
inline Chunks horizon_chunks(int requested, int T) {
  int C = requested < 1 ? 1 : requested;
  if (C > T) C = T;
  if (C > 8) C = 8;
  return Chunks{C, (T + C - 1) / C};
}

// ---- staged step chain: the population cut into P contiguous parts, multiples of 64 samples but the last, at most four and
// none below 1024 samples; part h holds samples [off[h], off[h] + n[h]) (n[h] may be 0 when the rounding leaves nothing)
struct Parts {
  int P;
  int64_t off[4], n[4];
};
inline Parts staged_partition(int64_t KE, int requested) {
  Parts s{};
  int P = requested < 1 ? 1 : requested;
  if (P > 4) P = 4;
  while (P > 1 && KE / P < 1024) --P;
  s.P = P;
  const int64_t per = ((KE / P) + 63) / 64 * 64;
  for (int h = 0; h < P; ++h) {
    s.off[h] = (int64_t)h * per < KE ? (int64_t)h * per : KE;
    s.n[h] = (h == P - 1) ? KE - s.off[h] : (s.off[h] + per <= KE ? per : KE - s.off[h]);
  }
  return s;
}

// ---- de Hoog chain-form calibration: `n` measured commands so far, the `ncand` candidates taking turns round after round;
// ms[candidate][round & 1] holds the last two rounds.  Between rounds, once at least four rounds AND half a second have passed
// (the clocks of an idle GPU ramp for ~0.3 s: whoever is measured last in a cold start would win), or after 64 rounds, the
// candidate whose faster of the last two rounds is smallest wins (ties: the lowest index).  -1: keep measuring.
inline int dehoog_pick(int n, int ncand, double elapsed_s, const float (*ms)[2]) {
  const int round = n / ncand;
  if (n % ncand != 0 || !((round >= 4 && elapsed_s >= 0.5) || round >= 64)) return -1;
  int choice = 0;
  float best = 1e30f;
  for (int v = 0; v < ncand; ++v) {
    const float mv = ms[v][0] < ms[v][1] ? ms[v][0] : ms[v][1];
    if (mv < best) {
      best = mv;
      choice = v;
    }
  }
  return choice;
}

// ---- one-launch fused body: which instance runs and who does what in its grid
struct FusedKnobs {            // options, as nlc_set_option stores them
  int blocks_per_cu = 0;       // 0 auto, 3 or 4
  int roll_cap = 0;            // 0 auto
  int chain_first_tiles = -1;  // -1 auto
  int partner_tiles = -2;      // -2 auto, -1 never
  double tile_step_ratio = 0.0;  // > 0 with partner_tiles on auto: the adaptive partner rule
};
struct FusedSchedule {
  int built;  // instance: workgroups per CU it was compiled for
  int bpc;    // workgroups per CU of the launch (what is resident of `built`)
  int ntk, n_enc, roll_cap, adaptive_q8, pool_wgs, chain_first_tiles, partner_tiles;  // FusedCtl's fields of the same name
  unsigned grid;
};
// occ_hi / occ_lo: resident workgroups per CU of the width's wider and narrower instance (4 and 3 per CU at h = 64 / 128, 2
// and 2 at h = 256: 68 KB of LDS per workgroup)
inline FusedSchedule fused_schedule(int ncu, int64_t KE, int T, int h, int occ_hi, int occ_lo, const FusedKnobs& o) {
  const int bpc_hi = h == 256 ? 2 : 4, bpc_lo = h == 256 ? 2 : 3;
  FusedSchedule s{};
  s.ntk = (int)((KE + 15) / 16);
  s.n_enc = s.ntk * T;
  // instance: three workgroups per CU (168 VGPRs) while chains sit on at most half of the CUs, else four (128 VGPRs)
  s.built = o.blocks_per_cu ? o.blocks_per_cu : (2 * s.ntk <= ncu ? 3 : 4);
  if (s.built == 3 && occ_lo < 3) s.built = 4;
  if (h == 256) s.built = 2;
  s.bpc = s.built == bpc_lo ? (occ_lo < bpc_lo ? occ_lo : bpc_lo) : (occ_hi < bpc_hi ? occ_hi : bpc_hi);
  // rollout workgroups start one per CU on the first CUs to arrive; by default on half the CUs at most
  // chains start on distinct CUs, one per 16-sample tile (the tiles beyond the CU count drain after the encoders)
  s.roll_cap = o.roll_cap > 0 ? o.roll_cap : ncu;
  if (s.roll_cap > s.ntk) s.roll_cap = s.ntk;
  // Schedule (profiles/r2_fused_small_shard.md).  Every workgroup -- the chains' too -- encodes one tile first.  A
  // chain's CU partners then encode M - 1 more tiles each and sleep until the chain is done: with few chains the CUs
  // WITHOUT one feed them alone (M = 1); the more CUs walk a chain, the longer their partners have to help.  M is an
  // empirical fit to the best schedule measured on the MI355X at T = 40 (chains on 25 / 37.5 / 43.75 / 50 % of the
  // CUs, K = 1024 / 1536 / 1792 / 2048: M = 1 / 2 / 3 / 4; e.g. 0.672 ms at K = 2048 against 0.723 without any of
  // this and 0.846 with M = 1), scaled with the horizon.
  const double f_chain = (double)s.roll_cap / (double)ncu;
  const double extra = (16.0 * f_chain - 4.5) * (double)T / 40.0;
  int auto_partner = 1 + (extra > 0 ? (int)extra : 0);
  if (s.built <= 3) {
    // two partners per chain CU instead of three: measured best M = 1 / 1 / 2 / 6 at chains on 12.5 / 25 / 37.5 / 50 %
    // of the CUs (K = 512 / 1024 / 1536 / 2048, T = 40; 0.521 / 0.527 / 0.563 / 0.674 ms per launch)
    // (K = 1280 / 1792, 31 / 44 %: M = 1 / 4; linear in between)
    const double m3 = f_chain <= 0.3125 ? 1.0 : 1.0 + 26.7 * (f_chain - 0.3125);
    auto_partner = (int)(1.0 + (m3 - 1.0) * (double)T / 40.0);
  }
  // experiment (option "fused_tile_step_ratio" > 0): partners sleep unless the chain-free CUs alone would
  // finish the remaining encoder tiles later than the chain finishes its remaining steps (the kernel's feedback
  // rule).  Measured SLOWER than the static schedule at every K (K = 2048: 0.83 vs 0.67 ms): the rule balances the
  // finishing times but not the ORDER -- the chains consume a horizon step per 11.5 us, the chain-free CUs produce one
  // per 15 us, so the chains starve behind the encoder front while their partners sleep; default off.
  const bool adaptive = o.partner_tiles == -2 && o.tile_step_ratio > 0.0;
  s.adaptive_q8 = adaptive ? (int)(256.0 * o.tile_step_ratio) : 0;
  s.pool_wgs = (ncu - s.roll_cap) * s.bpc;
  if (adaptive) auto_partner = 1;  // every partner encodes one tile first, then the rule decides
  s.chain_first_tiles = o.chain_first_tiles >= 0 ? o.chain_first_tiles : 1;
  const int partner = o.partner_tiles >= -1 ? o.partner_tiles : auto_partner;
  // (sleepers need CUs without a chain to produce the latents the chains wait for)
  s.partner_tiles = (adaptive || s.roll_cap <= ncu / 2) ? partner : -1;
  // every workgroup must be resident at once: a rollout workgroup waits for encoder workgroups of the same launch
  s.grid = (unsigned)(ncu * s.bpc);
  return s;
}

}  // namespace plan
}  // namespace nlc
