// Host build of the planner's pure decisions (csrc/nlc_plan.h) for tests/test_plan_host.py: C entry points over plain
// integer / double arrays.  With -DNLC_PLAN_HOST_MAIN the file is a stand-alone program that sweeps the same functions over
// their whole argument ranges (for a run under -fsanitize=address,undefined) and checks the invariants as it goes.
#include "../../neurallaplacecontrol_amd/csrc/nlc_plan.h"

using namespace nlc::plan;

extern "C" {

// out[7]: state, abuf, action, giveup, seq, merge_status, total (doubles)
void nlc_p_pin_layout(int E, int d, int B, int nu, int T, long* out) {
  const PinLayout p = pin_layout(E, d, B, nu, T);
  const size_t v[7] = {p.state, p.abuf, p.action, p.giveup, p.seq, p.merge_status, p.total};
  for (int i = 0; i < 7; ++i) out[i] = (long)v[i];
}

// out[2]: C, Tc
void nlc_p_horizon_chunks(int requested, int T, int* out) {
  const Chunks c = horizon_chunks(requested, T);
  out[0] = c.C;
  out[1] = c.Tc;
}

// out[9]: P, off[4], n[4]
void nlc_p_staged_partition(long KE, int requested, long* out) {
  const Parts s = staged_partition(KE, requested);
  out[0] = s.P;
  for (int h = 0; h < 4; ++h) {
    out[1 + h] = h < s.P ? (long)s.off[h] : -1;
    out[5 + h] = h < s.P ? (long)s.n[h] : -1;
  }
}

// ms: [3][2] floats
int nlc_p_dehoog_pick(int n, int ncand, double elapsed_s, const float* ms) {
  return dehoog_pick(n, ncand, elapsed_s, reinterpret_cast<const float(*)[2]>(ms));
}

// knobs[4]: blocks_per_cu, roll_cap, chain_first_tiles, partner_tiles; out[10]: built, bpc, ntk, n_enc, roll_cap, adaptive_q8,
// pool_wgs, chain_first_tiles, partner_tiles, grid
void nlc_p_fused_schedule(int ncu, long KE, int T, int h, int occ_hi, int occ_lo, const int* knobs, double tile_step_ratio,
                          int* out) {
  FusedKnobs o;
  o.blocks_per_cu = knobs[0];
  o.roll_cap = knobs[1];
  o.chain_first_tiles = knobs[2];
  o.partner_tiles = knobs[3];
  o.tile_step_ratio = tile_step_ratio;
  const FusedSchedule s = fused_schedule(ncu, KE, T, h, occ_hi, occ_lo, o);
  const int v[10] = {s.built, s.bpc, s.ntk, s.n_enc, s.roll_cap, s.adaptive_q8, s.pool_wgs, s.chain_first_tiles, s.partner_tiles,
                     (int)s.grid};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
}

}  // extern "C"

#ifdef NLC_PLAN_HOST_MAIN
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define REQUIRE(x)                                                  \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "plan_host: %s failed (line %d)\n", #x, __LINE__); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

int main() {
  long checked = 0;
  for (int E : {1, 2, 5, 65535})
    for (int d = 1; d <= 6; ++d)
      for (int B : {1, 4, 16})
        for (int nu = 1; nu <= 2; ++nu)
          for (int T : {1, 7, 40, 200}) {
            long o[7];
            nlc_p_pin_layout(E, d, B, nu, T, o);
            REQUIRE(o[0] == 0 && o[0] < o[1] && o[1] < o[2] && o[2] < o[3] && o[3] < o[4] && o[4] < o[5] && o[5] < o[6]);
            REQUIRE(o[6] == (long)E * d + (long)E * B * nu + (long)E * T * nu + 8);
            ++checked;
          }
  for (int T = 1; T <= 64; ++T)
    for (int req = 0; req <= 9; ++req) {
      int o[2];
      nlc_p_horizon_chunks(req, T, o);
      REQUIRE(o[0] >= 1 && o[0] <= 8 && o[0] <= T && o[1] * o[0] >= T);
      ++checked;
    }
  for (long KE = 1; KE <= 20000; KE += 37)
    for (int req = 0; req <= 5; ++req) {
      long o[9];
      nlc_p_staged_partition(KE, req, o);
      long at = 0;
      for (int h = 0; h < o[0]; ++h) {
        REQUIRE(o[1 + h] == at && o[5 + h] >= 0);
        at += o[5 + h];
      }
      REQUIRE(at == KE && o[0] >= 1 && o[0] <= 4);
      ++checked;
    }
  float ms[3][2] = {{3.f, 2.f}, {2.f, 5.f}, {1e30f, 1e30f}};
  for (int ncand = 2; ncand <= 3; ++ncand)
    for (int n = 0; n <= 64 * ncand; ++n)
      for (double el : {0.0, 0.49, 0.5, 10.0}) {
        const int v = nlc_p_dehoog_pick(n, ncand, el, &ms[0][0]);
        REQUIRE(v >= -1 && v < ncand);
        ++checked;
      }
  for (int ncu : {1, 8, 256, 304})
    for (long KE : {1L, 16L, 17L, 512L, 2048L, 4096L, 100000L})
      for (int T : {1, 20, 40, 80})
        for (int h : {64, 128, 256})
          for (int bpc : {0, 3, 4})
            for (int partner : {-2, -1, 0, 5})
              for (double ratio : {0.0, 1.5}) {
                const int knobs[4] = {bpc, ncu / 3, -1, partner};
                int o[10];
                nlc_p_fused_schedule(ncu, KE, T, h, h == 256 ? 2 : 4, h == 256 ? 2 : 3, knobs, ratio, o);
                REQUIRE(o[4] >= 1 && o[4] <= o[2] && o[1] >= 1 && o[9] == ncu * o[1] && o[6] >= 0 && o[8] >= -1);
                ++checked;
              }
  std::printf("plan_host: %ld cases ok\n", checked);
  return 0;
}
#endif
