// Synthetic transition dataset: generate_irregular_data_delay_time_multi with rand=True (overlay.py:664-737) on the device.
//   compute_state_actions   :603-631   S states and A actions per time block, uniform over a box
//   batch_integrate_system  base_env.py:231-280   one Euler step of the block's interval for every (action, state) pair
//   the action buffer       overlay.py:718-731    uniform fill, the row's action at B - 1 - delay, the time column
// One lane per row, 256 rows per workgroup; a workgroup's rows are one contiguous span of each of the four arrays.  No
// atomics and no communication beyond the store staging: the observations before and after the step go through LDS and
// leave as unit-stride stores (16 B per lane where the span is 16-byte aligned); the action buffer is produced in output
// order -- its draws are indexed by (row, buffer row), so the lane that stores an entry can draw it -- and ts is unit
// stride as it is.  The dynamics and the observation are the device bodies env_step_kernel runs (nlc_env_dev.h), the
// element math is nlc_synth.h (host-testable).  Built with -ffp-contract=off (csrc/Makefile), as nlc_env_dev.h requires.
#include "nlc_device.h"

#include "nlc_collect.h"
#include "nlc_env_dev.h"
#include "nlc_kernels.h"
#include "nlc_synth.h"

namespace nlc {

constexpr int kSynthRows = 256;  // rows (= lanes) per workgroup

// one Philox block of (index, second index, stream): a draw depends on nothing else (not on the launch shape or ti_begin)
__device__ __forceinline__ u4 synth_block(uint64_t seed, int64_t idx, int64_t idx2, uint32_t stream) {
  return philox4x32_10(u4{(uint32_t)idx, (uint32_t)((uint64_t)idx >> 32), (uint32_t)idx2, stream}, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}
// action i of time block ti (block 0's with reuse)
__device__ __forceinline__ void synth_action(const SynthArgs& a, int64_t ti, int64_t i, double* act) {
  const u4 r = synth_block(a.seed, i, a.reuse ? 0 : ti, synth::kStreamAction);
  static_assert(NLC_MAX_NU <= 2, "one Philox block yields two uniforms");
  act[0] = synth::box(u53(r.x, r.y), a.action_high);
  act[1] = synth::box(u53(r.z, r.w), a.action_high);
}

// `count` doubles of a workgroup's LDS image to its span of an output array, unit stride
__device__ __forceinline__ void synth_store_span(double* __restrict__ dst, const double* src, int count, int t) {
  if (((uintptr_t)dst & 15) == 0) {
    const int pairs = count >> 1;
    for (int p = t; p < pairs; p += kSynthRows) reinterpret_cast<double2*>(dst)[p] = reinterpret_cast<const double2*>(src)[p];
    if (t == 0 && (count & 1)) dst[count - 1] = src[count - 1];
  } else {
    for (int e = t; e < count; e += kSynthRows) dst[e] = src[e];
  }
}

template <int ENV>
__global__ __launch_bounds__(kSynthRows) void synth_kernel(const SynthArgs a) {
  constexpr int n = (ENV == NLC_ENV_PENDULUM) ? 2 : 4;
  constexpr int d = (ENV == NLC_ENV_CARTPOLE) ? 5 : ((ENV == NLC_ENV_PENDULUM) ? 3 : 6);
  __shared__ __attribute__((aligned(16))) double stage[2][kSynthRows * d];
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kSynthRows;  // first row of this workgroup, within the call
  const int nrows = (int)(a.rows - row0 < kSynthRows ? a.rows - row0 : kSynthRows);
  const int64_t g0 = synth::global_row(row0, a.ti_begin, a.A, a.S);
  if (t < nrows) {
    const synth::RowIndex x = synth::row_index(g0 + t, a.A, a.S);
    const int64_t tic = a.reuse ? 0 : x.ti;
    // state j of the block: (2u - 1) * state_max per component
    double s[4], o[6], act[NLC_MAX_NU];
    {
      const u4 r = synth_block(a.seed, x.j, tic, synth::kStreamState);
      s[0] = synth::box(u53(r.x, r.y), a.state_max[0]);
      s[1] = synth::box(u53(r.z, r.w), a.state_max[1]);
      s[2] = s[3] = 0.0;
      if (n > 2) {
        const u4 q = synth_block(a.seed, x.j, tic, synth::kStreamState + 1);
        s[2] = synth::box(u53(q.x, q.y), a.state_max[2]);
        s[3] = synth::box(u53(q.z, q.w), a.state_max[3]);
      }
    }
    synth_action(a, x.ti, x.i, act);
    // the block's interval (build_time_grid(only_one_step), once per batch_integrate_system call)
    double tsn = a.dt;
    if (a.ts_grid != NLC_TS_GRID_FIXED) {
      const u4 r = synth_block(a.seed, 0, x.ti, synth::kStreamInterval);
      tsn = collect::interval(a.ts_grid, a.dt, u53(r.x, r.y));
    }
    env_observe(ENV, s, o);
#pragma unroll
    for (int c = 0; c < d; ++c) stage[0][t * d + c] = o[c];
    env_euler_step(ENV, s, act, a.friction, tsn);
    env_observe(ENV, s, o);
#pragma unroll
    for (int c = 0; c < d; ++c) stage[1][t * d + c] = o[c];
    a.ts[row0 + t] = tsn;
  }
  __syncthreads();
  synth_store_span(a.s0 + row0 * d, stage[0], nrows * d, t);
  synth_store_span(a.sn + row0 * d, stage[1], nrows * d, t);
  // the action buffers, in output order: unit q = (row, buffer row b) holds W consecutive doubles
  const int W = a.nu + a.time_channel;
  const int units = nrows * a.B;
  double* __restrict__ a0 = a.a0 + row0 * a.B * W;
  for (int q = t; q < units; q += kSynthRows) {
    const int lr = q / a.B, b = q - lr * a.B;
    double act[NLC_MAX_NU + 1] = {0.0, 0.0, 0.0}, u[NLC_MAX_NU + 1] = {0.5, 0.5, 0.5};  // (entry NLC_MAX_NU is never read)
    if (b == a.B - 1 - a.delay) {
      const synth::RowIndex x = synth::row_index(g0 + lr, a.A, a.S);
      synth_action(a, x.ti, x.i, act);
    } else {
      const u4 r = synth_block(a.seed, g0 + lr, b, synth::kStreamFill);
      u[0] = u53(r.x, r.y);
      u[1] = u53(r.z, r.w);
    }
    // (constant subscripts of act / u: a run-time one would put the two arrays in scratch)
#pragma unroll
    for (int col = 0; col < NLC_MAX_NU + 1; ++col)
      if (col < W) a0[(int64_t)q * W + col] = synth::buffer_entry(b, col, a.B, a.nu, a.delay, act, u, a.action_high);
  }
}

hipError_t launch_synth(const SynthArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipErrorInvalidValue;
  const int64_t blocks = (a.rows + kSynthRows - 1) / kSynthRows;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kSynthRows);
  if (a.env == NLC_ENV_CARTPOLE)
    hipLaunchKernelGGL(synth_kernel<NLC_ENV_CARTPOLE>, grid, block, 0, s, a);
  else if (a.env == NLC_ENV_PENDULUM)
    hipLaunchKernelGGL(synth_kernel<NLC_ENV_PENDULUM>, grid, block, 0, s, a);
  else if (a.env == NLC_ENV_ACROBOT)
    hipLaunchKernelGGL(synth_kernel<NLC_ENV_ACROBOT>, grid, block, 0, s, a);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace nlc
