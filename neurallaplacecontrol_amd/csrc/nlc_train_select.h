// Snapshot selection of the fused trainers (kernels_train_select.hip, abi_train_select.hip): "copy the weights if the loss is
// the best so far", the reference's save-on-improvement (train_utils.py:439-448) and best_val_loss (:491), per member of a
// group and on the device.  Plain C++: tests/helpers/train_select_host.cpp compiles the rule and the chunk plan with g++.
//
// A header of its own, not part of nlc_train.h: the training and evaluation kernels do not include it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NLC_SELECT_HD __host__ __device__ __forceinline__
#else
#define NLC_SELECT_HD inline
#endif

namespace nlc {
namespace train {

constexpr int kSelectThreads = 256;                  // both kernels
constexpr int64_t kSelectChunk = 2048;               // doubles of a member's row one workgroup copies (16 KiB)
constexpr int kSelectMaxGroup = 65535;               // the member is the grid's y axis (kMaxGroup of nlc_train.h)
constexpr int64_t kSelectMaxChunks = 2147483647LL;   // the chunks are the grid's x axis

// The rule.  Strict: an equal loss keeps the earlier snapshot.  Every comparison with a NaN is false, so a NaN loss never
// improves and a NaN best is never replaced; best starts at +inf, which +inf does not beat and -inf does, once.  -0.0 and
// 0.0 compare equal.
NLC_SELECT_HD bool improves(double loss, double best) { return loss < best; }

// workgroups on x for a row of P doubles
NLC_SELECT_HD int64_t select_chunks(int64_t P) { return (P + kSelectChunk - 1) / kSelectChunk; }

// How a workgroup copies n doubles from s to d (both 8-byte aligned): `head` single doubles up to the first 16-byte
// boundary, `pairs` 16-byte accesses, `tail` single doubles.  Source and destination must reach a 16-byte boundary
// together; when they do not (one row starts on an odd double, the other on an even one) everything goes as singles.
struct SelectSpan {
  int64_t head, pairs, tail;
};
NLC_SELECT_HD SelectSpan select_span(uint64_t s_addr, uint64_t d_addr, int64_t n) {
  SelectSpan sp;
  if (((s_addr ^ d_addr) & 15) != 0) {
    sp.head = n;
    sp.pairs = 0;
    sp.tail = 0;
    return sp;
  }
  sp.head = (s_addr & 15) != 0 && n > 0 ? 1 : 0;
  sp.pairs = (n - sp.head) / 2;
  sp.tail = n - sp.head - 2 * sp.pairs;
  return sp;
}

struct KeepBestArgs {
  const double* loss;       // [M]
  const double* params;     // [M][P]
  double* best_loss;        // [M]; read-only in the copy launch
  double* best_params;      // [M][P]
  int64_t* best_tag;        // [M]
  int32_t* improved;        // [M] or NULL
  int64_t P, tag;
  int M;
};

}  // namespace train
}  // namespace nlc

#if defined(__HIPCC__)
namespace nlc {
namespace train {
// the copy: select_chunks(P) workgroups on x, the M members on y; a member that did not improve returns after two reads
hipError_t launch_train_keep_best(const KeepBestArgs& a, hipStream_t s);
// the commit: one thread per member writes best_loss, best_tag, improved
hipError_t launch_train_commit_best(const KeepBestArgs& a, hipStream_t s);
}  // namespace train
}  // namespace nlc
#endif
