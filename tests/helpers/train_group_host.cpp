// Host build of the training workspace partition (csrc/nlc_train.h, plain C++) for tests/test_train_group_host.py: one member's
// layout for a call's sizes, as abi_train.hip computes it.
#include <stdint.h>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train.h"

using namespace nlc::train;

// out[0..5] = partial, tile_loss, act, grad, sq offsets and the member's total (doubles); out[6..9] = nblk, P, A, chunks.
// rnn: DeltaTRNN / RNN of width h (S unused), else NeuralLaplaceModel of width h with S terms.
extern "C" void nlc_t_member_layout(int rnn, int d, int nin, int h, int S, int64_t N, int64_t* out) {
  int64_t off[kTensors + 1];
  int cstart[kTensors + 1];
  int64_t A;
  if (rnn) {
    rnn_blob_offsets(d, nin, h, 1, off);
    A = rnn_act_layout(nin, h, kMaxB).total;
  } else {
    blob_offsets(d, nin, h / 2, h, S, off);
    A = act_layout(d, nin, h / 2, h, S, kMaxB).total;
  }
  const int64_t P = off[kTensors], ntiles = (N + kRows - 1) / kRows;
  const int nblk = (int)(ntiles < kMaxBlocks ? ntiles : kMaxBlocks);
  const int chunks = chunk_starts(off, cstart);
  const TrainWsLayout w = train_ws_layout(nblk, P, A, chunks);
  const int64_t v[10] = {w.partial, w.tile_loss, w.act, w.grad, w.sq, w.total, nblk, P, A, chunks};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
}
