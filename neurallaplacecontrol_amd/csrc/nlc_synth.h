// Per-element math of the synthetic transition dataset (kernels_synth.hip: synth_kernel), the device form of
// generate_irregular_data_delay_time_multi / compute_state_actions (overlay.py:603-737, rand=True) over
// batch_integrate_system (base_env.py:231-280).  Everything here is __host__ __device__ so that tests/helpers/synth_host.cpp
// compiles the same functions with g++ and tests/test_synth_host.py checks them on the CPU.
#pragma once
#include <stdint.h>

#include "../../include/nlc.h"
#include "nlc_math.h"

namespace nlc {
namespace synth {

// Philox streams of a dataset: key = the dataset's seed, counter = (index lo, index hi, second index, stream)
//   state     (j, ti, kStreamState)      components 0, 1; kStreamState + 1: components 2, 3
//   action    (i, ti, kStreamAction)     one uniform per action dim
//   interval  (0, ti, kStreamInterval)   one uniform
//   fill      (r, b,  kStreamFill)       one uniform per action dim; r is the GLOBAL row
// With reuse_state_actions_when_sampling_times the state and action counters take ti = 0 in every block.
constexpr uint32_t kStreamState = 0, kStreamAction = 2, kStreamInterval = 3, kStreamFill = 4;

// TI * A * S must stay below this: global rows are Philox counter words (lo, hi) and int64 element indices
constexpr int64_t kMaxRows = (int64_t)1 << 40;

// ---- row order: TI time blocks x A actions x S states, blocks concatenated (overlay.py:713-716), action-major within a
// block as batch_integrate_system stacks them (base_env.py:263-276): r = (ti * A + i) * S + j
struct RowIndex {
  int64_t ti, i, j;
};
NLC_HD int64_t row_of(int64_t ti, int64_t i, int64_t j, int64_t A, int64_t S) { return (ti * A + i) * S + j; }
NLC_HD RowIndex row_index(int64_t r, int64_t A, int64_t S) {
  const int64_t q = r / S;
  RowIndex x;
  x.j = r - q * S;
  x.ti = q / A;
  x.i = q - x.ti * A;
  return x;
}
// global row of row `local` of a call that starts at time block ti_begin
NLC_HD int64_t global_row(int64_t local, int64_t ti_begin, int64_t A, int64_t S) { return ti_begin * A * S + local; }

// ---- (rand - 0.5) * 2.0 * max (overlay.py:605-629, 718) from u in (0, 1): symmetric, inside [-max, max]
NLC_HD double box(double u, double max) { return (2.0 * u - 1.0) * max; }

// ---- observation-time column of the (B, W) buffer: flip(arange(B)) (overlay.py:722-731)
NLC_HD double time_column(int b, int B) { return (double)(B - 1 - b); }

// ---- entry (b, col) of a row's (B, W = nu [+ 1]) action buffer: uniform fill (:718) except buffer row B - 1 - delay, which
// is the row's action (:720); column nu, where there is one, is the time column.  act, u: nu values each.
NLC_HD double buffer_entry(int b, int col, int B, int nu, int delay, const double* act, const double* u, double high) {
  if (col >= nu) return time_column(b, B);
  if (b == B - 1 - delay) return act[col];
  return box(u[col], high);
}

}  // namespace synth
}  // namespace nlc
