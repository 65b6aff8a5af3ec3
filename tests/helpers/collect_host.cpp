// Host build of the element math of the expert-data collector's control step (neurallaplacecontrol_amd/csrc/nlc_collect.h)
// for tests/test_collect_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_collect.h"
using namespace nlc::collect;
extern "C" {
// interval(ts_grid, dt, u) over n uniforms
void nlc_c_interval(int ts_grid, double dt, const double* u, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = interval(ts_grid, dt, u[i]);
}
// noisy_action over rows (a, u); random_action over u
void nlc_c_noisy_action(const double* in, double low, double high, double scale, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = noisy_action(in[2 * i], in[2 * i + 1], low, high, scale);
}
void nlc_c_random_action(const double* u, double low, double high, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = random_action(u[i], low, high);
}
// the time column of one (B, W) buffer over `steps` control steps with intervals ts: buffer after every step -> out (steps, B, W)
void nlc_c_time_channel(double* ab, int B, int W, int nu, const double* ts, int steps, double* out) {
  for (int s = 0; s < steps; ++s) {
    time_channel_roll(ab, B, W, nu);
    time_channel_advance(ab, B, W, nu, ts[s]);
    for (int i = 0; i < B * W; ++i) out[(long)s * B * W + i] = ab[i];
  }
}
long long nlc_c_row_index(long long episode_base, long long e, int steps_per_episode, int it) {
  return (long long)row_index(episode_base, e, steps_per_episode, it);
}
int nlc_c_stream(int which) {
  const unsigned s[4] = {kStreamInterval, kStreamActionNoise, kStreamObsNoise, kStreamRandomPolicy};
  return (int)s[which];
}
}
