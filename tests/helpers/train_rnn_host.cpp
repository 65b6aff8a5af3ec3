// Host build of the DeltaTRNN / RNN training step's shape functions (neurallaplacecontrol_amd/csrc/nlc_train.h) for
// tests/test_train_rnn_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_train.h"
using namespace nlc::train;
extern "C" {
int nlc_t_tensors() { return kTensors; }
int nlc_t_chunk() { return kChunk; }
// rnn_blob_offsets(d, nin, H, time_input): off[0..kTensors], then chunk_starts of it: cstart[0..kTensors]
void nlc_t_rnn_plan(int d, int nin, int H, int time_input, long long* off_out, int* cstart_out) {
  int64_t off[kTensors + 1];
  int cstart[kTensors + 1];
  rnn_blob_offsets(d, nin, H, time_input, off);
  chunk_starts(off, cstart);
  for (int i = 0; i <= kTensors; ++i) {
    off_out[i] = (long long)off[i];
    cstart_out[i] = cstart[i];
  }
}
// rnn_act_layout(nin, H, B): X, Hs, G, DI, DH, total
void nlc_t_rnn_act_layout(int nin, int H, int B, long long* out) {
  const RnnActLayout L = rnn_act_layout(nin, H, B);
  const int64_t f[6] = {L.X, L.Hs, L.G, L.DI, L.DH, L.total};
  for (int i = 0; i < 6; ++i) out[i] = (long long)f[i];
}
}
