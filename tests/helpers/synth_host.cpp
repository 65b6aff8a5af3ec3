// Host build of the element math of the synthetic transition dataset (neurallaplacecontrol_amd/csrc/nlc_synth.h) for
// tests/test_synth_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_synth.h"
using namespace nlc::synth;
extern "C" {
// rows[k] -> out[3 k ..] = (ti, i, j)
void nlc_s_row_index(const long long* rows, long n, long long A, long long S, long long* out) {
  for (long k = 0; k < n; ++k) {
    const RowIndex x = row_index(rows[k], A, S);
    out[3 * k] = x.ti;
    out[3 * k + 1] = x.i;
    out[3 * k + 2] = x.j;
  }
}
long long nlc_s_row_of(long long ti, long long i, long long j, long long A, long long S) { return row_of(ti, i, j, A, S); }
long long nlc_s_global_row(long long local, long long ti_begin, long long A, long long S) {
  return global_row(local, ti_begin, A, S);
}
long long nlc_s_max_rows(void) { return kMaxRows; }
void nlc_s_box(const double* u, double max, double* out, long n) {
  for (long k = 0; k < n; ++k) out[k] = box(u[k], max);
}
// one row's (B, W) buffer from its action act (nu) and the fill uniforms u (B, nu)
void nlc_s_buffer(int B, int nu, int time_channel, int delay, const double* act, const double* u, double high, double* out) {
  const int W = nu + time_channel;
  for (int b = 0; b < B; ++b)
    for (int col = 0; col < W; ++col) out[b * W + col] = buffer_entry(b, col, B, nu, delay, act, u + b * nu, high);
}
int nlc_s_stream(int which) {
  const unsigned s[4] = {kStreamState, kStreamAction, kStreamInterval, kStreamFill};
  return (int)s[which];
}
}
