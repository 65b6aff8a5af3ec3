// Host build of the evaluation layouts (csrc/nlc_train_eval.h, plain C++) for tests/test_train_eval_host.py: the workspace of
// the held-out loss, its grid rule and a workgroup's LDS partition, as abi_train.hip computes them.  With a main() of its own,
// so the same file also builds stand-alone (under -fsanitize=address,undefined) and walks every shape the library accepts.
#include <stdint.h>
#include <stdio.h>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train_eval.h"

using namespace nlc::train;

// out = ntiles, tile_loss offset, a member's total (doubles)
extern "C" void nlc_t_eval_ws_layout(int64_t N, int64_t* out) {
  const EvalWsLayout w = eval_ws_layout(N);
  out[0] = w.ntiles;
  out[1] = w.tile_loss;
  out[2] = w.total;
}

extern "C" int nlc_t_eval_grid(int64_t ntiles, int cus, int per_cu, int M) { return eval_grid(ntiles, cus, per_cu, M); }

extern "C" int nlc_t_eval_ld(int n) { return eval_ld(n); }

// out[0..11] = X, a0, tn, tgt, sq, h0, h1, G, a1, a2, u, total (doubles); out[12..17] = ldg, ldG, ldK, ldh, ldu, dc
extern "C" void nlc_t_eval_lds_layout(int d, int nin, int h, int S, int B, int64_t* out) {
  const EvalLdsLayout L = eval_lds_layout(d, nin, h / 2, h, S, B);
  const int64_t v[18] = {L.X, L.a0, L.tn, L.tgt, L.sq, L.h0, L.h1, L.G, L.a1, L.a2, L.u, L.total,
                         L.ldg, L.ldG, L.ldK, L.ldh, L.ldu, L.dc};
  for (int i = 0; i < 18; ++i) out[i] = v[i];
}

extern "C" int64_t nlc_t_rnn_eval_lds_bytes(int H) { return rnn_eval_lds_doubles(H) * (int64_t)sizeof(double); }

// every shape nlc_set_model takes: the LDS partition fits a compute unit and holds at least one state dim of the last layer
int main() {
  const int hs[3] = {64, 128, 256};
  int64_t worst = 0;
  for (int h : hs)
    for (int d = 1; d <= 8; ++d)
      for (int nin = 1; nin <= 3; ++nin)
        for (int S = 1; S <= 129; ++S)
          for (int B = 1; B <= kMaxB; B += 5) {
            const EvalLdsLayout L = eval_lds_layout(d, nin, h / 2, h, S, B);
            const int64_t bytes = L.total * (int64_t)sizeof(double);
            if (bytes > kLdsBytes || L.dc < 1 || L.dc > d || L.ldu < 2 * L.dc * S) {
              printf("bad layout h=%d d=%d nin=%d S=%d B=%d: %lld bytes dc=%d\n", h, d, nin, S, B, (long long)bytes, L.dc);
              return 1;
            }
            if (bytes > worst) worst = bytes;
          }
  printf("ok worst=%lld\n", (long long)worst);
  return 0;
}
