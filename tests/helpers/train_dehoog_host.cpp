// Host build of the de Hoog training step's workspace layout (csrc/nlc_train_dehoog.h, plain C++) for
// tests/test_train_dehoog_host.py, as abi_train.hip computes it.  With a main() of its own, so the same file also builds
// stand-alone (under -fsanitize=address,undefined) and walks every shape the step accepts.
#include <stdint.h>
#include <stdio.h>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train_dehoog.h"

using namespace nlc::train;

// one member's region of the shared part (TrainWsLayout::total), as plan_of / plan_rows size it: slabs for the longest window
static int64_t member_total(int64_t N, int d, int nin, int h, int S) {
  int64_t off[kTensors + 1];
  int cstart[kTensors + 1];
  blob_offsets(d, nin, h / 2, h, S, off);
  const int64_t ntiles = (N + kRows - 1) / kRows;
  const int nblk = (int)(ntiles < kMaxBlocks ? ntiles : kMaxBlocks);
  const int chunks = chunk_starts(off, cstart);
  return train_ws_layout(nblk, off[kTensors], act_layout(d, nin, h / 2, h, S, kMaxB).total, chunks).total;
}

extern "C" int64_t nlc_t_dehoog_member_total(int64_t N, int d, int nin, int h, int S) { return member_total(N, d, nin, h, S); }

// out = rows, theta, phi, gtheta, gphi, pred, gx, t, scratch, scratch_bytes, total (doubles but scratch_bytes)
extern "C" void nlc_t_dehoog_ws_layout(int M, int64_t N, int d, int nin, int h, int S, int64_t* out) {
  const DehoogWsLayout w = dehoog_ws_layout(M, N, d, S, member_total(N, d, nin, h, S));
  const int64_t v[11] = {w.rows, w.theta, w.phi, w.gtheta, w.gphi, w.pred, w.gx, w.t, w.scratch, w.scratch_bytes, w.total};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
}

// the ILT launcher's own figures (csrc/nlc_dehoog_tape.h, which kernels_dehoog_bwd.hip includes)
extern "C" int64_t nlc_t_dehoog_tape_entries(int Mq) { return nlc::DhLayout{Mq}.entries(); }
extern "C" int64_t nlc_t_dehoog_scratch_bytes(int64_t ilt_rows, int S) { return nlc::dehoog_bwd_tape_bytes(ilt_rows, S); }

// every accepted shape: the arrays are in order, aligned and inside the total
int main() {
  const int hs[3] = {64, 128, 256};
  const int64_t Ns[6] = {1, 16, 17, 37, 2048, 5000};
  int64_t worst = 0;
  for (int h : hs)
    for (int d = 1; d <= 8; ++d)
      for (int S = 3; S <= 33; S += 2)
        for (int64_t N : Ns)
          for (int M = 1; M <= 65; M += 32) {
            const int64_t mt = member_total(N, d, 3, h, S);
            const DehoogWsLayout w = dehoog_ws_layout(M, N, d, S, mt);
            const int64_t o[9] = {w.theta, w.phi, w.gtheta, w.gphi, w.pred, w.gx, w.t, w.scratch, w.total};
            if (w.theta < (int64_t)M * mt) return 1;
            for (int i = 0; i < 9; ++i)
              if (o[i] % 32 != 0 || (i > 0 && o[i] <= o[i - 1])) return 2;
            if (w.total - w.scratch < (w.scratch_bytes + 7) / 8) return 3;
            if (w.total > worst) worst = w.total;
          }
  printf("ok %lld\n", (long long)worst);
  return 0;
}
