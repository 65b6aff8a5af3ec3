// Host build of the patience rule and the per-member step size (csrc/nlc_train_members.h, plain C++) for
// tests/test_train_members_host.py.  With a main() of its own, so the same file also builds stand-alone (under
// -fsanitize=address,undefined): it runs the patience kernel's loop on the host over exact-size heap blocks.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train_members.h"

using namespace nlc::train;

// one member over n checks: improved[k] in, the three words after check k out ([n] each); tag of check k is k + 1
extern "C" void nlc_t_patience_run(const int32_t* improved, long n, double patience, int64_t waiting, int32_t active,
                                   int64_t stopped_at, int64_t* waiting_out, int32_t* active_out, int64_t* stopped_out) {
  for (long k = 0; k < n; ++k) {
    patience_step(improved[k] != 0, patience, k + 1, &waiting, &active, &stopped_at);
    waiting_out[k] = waiting;
    active_out[k] = active;
    stopped_out[k] = stopped_at;
  }
}

// out[i] = member_step_size(lr[i], 1 - beta1 ** step[i]), the bias correction formed as the library's host side forms it
extern "C" void nlc_t_step_size(const double* lr, const int64_t* step, double beta1, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = member_step_size(lr[i], 1.0 - pow(beta1, (double)step[i]));
}

// what train_patience_kernel does, member by member
static void patience_host(const PatienceArgs& a) {
  for (int64_t m = 0; m < a.M; ++m) {
    int64_t waiting = a.waiting[m], stopped_at = a.stopped_at[m];
    int32_t active = a.active[m];
    if (active == 0) continue;
    patience_step(a.improved[m] != 0, a.patience, a.tag, &waiting, &active, &stopped_at);
    a.waiting[m] = waiting;
    a.active[m] = active;
    a.stopped_at[m] = stopped_at;
  }
}

int main() {
  const int Ms[] = {1, 3, 255, 256, 257};
  for (int M : Ms) {
    // exact-size heap blocks: a step past either end is an ASan report
    std::vector<int32_t> improved(M), active(M, 1);
    std::vector<int64_t> waiting(M, 0), stopped(M, -1);
    const double patience = 1.0;
    // member m improves at check k iff k < m % 4: it stops at check m % 4 + 3 (two checks of waiting 0 -> 2, then the stop)
    for (int k = 0; k < 12; ++k) {
      for (int m = 0; m < M; ++m) improved[m] = k < m % 4 ? 1 : 0;
      const PatienceArgs a{improved.data(), waiting.data(), active.data(), stopped.data(), patience, k + 1, M};
      patience_host(a);
    }
    for (int m = 0; m < M; ++m)
      if (active[m] != 0 || stopped[m] != m % 4 + 3 || waiting[m] != 2) {
        printf("bad member M=%d m=%d active=%d stopped=%lld waiting=%lld\n", M, m, active[m], (long long)stopped[m],
               (long long)waiting[m]);
        return 1;
      }
  }
  // inf never stops; the step size is finite and negative for a positive lr at every step count
  int64_t w = 0, s = -1;
  int32_t act = 1;
  for (int k = 0; k < 1000; ++k) patience_step(false, INFINITY, k, &w, &act, &s);
  if (act != 1 || w != 1000 || s != -1) return 1;
  for (int64_t step = 1; step < 100000; step = step * 3 + 1) {
    const double v = member_step_size(1e-4, 1.0 - pow(0.9, (double)step));
    if (!(v < 0.0) || !isfinite(v)) return 1;
  }
  printf("ok\n");
  return 0;
}
