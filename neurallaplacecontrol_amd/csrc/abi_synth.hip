// Host side of libnlc_hip.so, synthetic-dataset unit: nlc_synth_generate validates a nlc_synth_desc and a range of time
// blocks on the host and launches synth_kernel (kernels_synth.hip) over the range's rows.
#include "nlc_host.h"
#include "nlc_synth.h"

using namespace nlc;
using namespace nlc::host;

extern "C" int nlc_synth_generate(nlc_ctx* c, const nlc_synth_desc* d, int64_t ti_begin, int64_t ti_end, double* s0,
                                  double* a0, double* sn, double* ts) {
  if (!c) return NLC_ERR_BAD_ARG;
  NLC_GUARD_BEGIN
  static const int env_nu[3] = {1, 1, 2};
  static const int env_n[3] = {4, 2, 4};
  if (!d) return fail(c, NLC_ERR_BAD_ARG, "NULL synth desc");
  if (d->env < 0 || d->env > 2) return fail(c, NLC_ERR_UNSUPPORTED, "synth: unknown env id");
  if (d->nu < 1 || d->nu > NLC_MAX_NU) return fail(c, NLC_ERR_BAD_SHAPE, "nu must be in 1..NLC_MAX_NU");
  if (d->nu != env_nu[d->env]) return fail(c, NLC_ERR_BAD_SHAPE, "nu does not match the env's action space");
  if (d->B < 1 || d->delay < 0 || d->delay > d->B - 1) return fail(c, NLC_ERR_BAD_SHAPE, "synth: delay must be in [0, B - 1], B >= 1");
  if (d->S < 1 || d->A < 1) return fail(c, NLC_ERR_BAD_SHAPE, "synth: S and A must be >= 1");
  if (ti_begin < 0 || ti_end <= ti_begin || ti_end > 0x7fffffff)
    return fail(c, NLC_ERR_BAD_SHAPE, "synth: time blocks must satisfy 0 <= ti_begin < ti_end < 2^31");
  // rows: the global row index of the last block must stay below 2^40 (128-bit product: S, A and ti_end are only known
  // to be positive here)
  const unsigned __int128 global_rows = (unsigned __int128)d->S * (unsigned __int128)d->A * (unsigned __int128)ti_end;
  if (global_rows >= (unsigned __int128)synth::kMaxRows) return fail(c, NLC_ERR_UNSUPPORTED, "synth: TI * A * S must be below 2^40");
  if (((ti_end - ti_begin) * d->A * d->S + 255) / 256 > 0x7fffffff)
    return fail(c, NLC_ERR_UNSUPPORTED, "synth: more than 2^31 - 1 workgroups of 256 rows in one call");
  if (d->ts_grid != NLC_TS_GRID_FIXED && d->ts_grid != NLC_TS_GRID_UNIFORM && d->ts_grid != NLC_TS_GRID_EXP)
    return fail(c, NLC_ERR_BAD_ARG, "synth: unknown ts_grid");
  if (!s0 || !a0 || !sn || !ts) return fail(c, NLC_ERR_BAD_ARG, "NULL device pointer");
  if (!(d->dt > 0.0) || !(d->action_high > 0.0)) return fail(c, NLC_ERR_BAD_ARG, "synth: dt and action_high must be > 0");
  for (int i = 0; i < env_n[d->env]; ++i)
    if (!(d->state_max[i] > 0.0)) return fail(c, NLC_ERR_BAD_ARG, "synth: state_max must be > 0");
  NLC_HIP(c, hipSetDevice(c->device));
  SynthArgs a{};
  a.env = d->env;
  a.friction = d->friction ? 1 : 0;
  a.B = d->B;
  a.nu = d->nu;
  a.delay = d->delay;
  a.time_channel = d->time_channel ? 1 : 0;
  a.ts_grid = d->ts_grid;
  a.reuse = d->reuse ? 1 : 0;
  a.S = d->S;
  a.A = d->A;
  a.ti_begin = ti_begin;
  a.rows = (ti_end - ti_begin) * d->A * d->S;
  a.dt = d->dt;
  a.action_high = d->action_high;
  for (int i = 0; i < 4; ++i) a.state_max[i] = d->state_max[i];
  a.seed = d->seed;
  a.s0 = s0;
  a.a0 = a0;
  a.sn = sn;
  a.ts = ts;
  ProfScope ps(c, "synth_kernel");
  NLC_HIP(c, launch_synth(a, c->stream));
  return NLC_OK;
  NLC_GUARD_END(c)
}
