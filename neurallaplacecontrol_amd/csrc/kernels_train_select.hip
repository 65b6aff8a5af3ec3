// Snapshot selection (nlc_train_keep_best, abi_train_select.hip): keep the parameters of the best loss seen so far, per member,
// on the device -- the reference's save-on-improvement, train_utils.py:439-448.  Two launches on one stream:
//
//   train_keep_best_kernel    grid (chunks of the row, M).  Reads loss[m] and best_loss[m] (nobody writes them in this launch)
//                             and returns at once unless the member improved; else copies its kSelectChunk doubles of
//                             params[m] to best_params[m].
//   train_commit_best_kernel  one thread per member: best_loss[m] = loss[m], best_tag[m] = tag on improvement; improved[m].
//
// One launch would not do: a workgroup that wrote best_loss[m] could make a later workgroup of the same member read "not
// improved" and leave the row half copied.  With best_loss read-only in the copy, every workgroup of a member decides alike,
// and the commit runs after all of them in stream order.  No atomics.
//
// A member that did not improve costs two 8-byte reads per workgroup and no other traffic.
//
// Rows start m * P doubles into the buffers, so with odd P every second row is only 8-byte aligned: the copy takes 16-byte
// accesses between the first and last 16-byte boundaries of its span when source and destination reach them together, and
// 8-byte ones for the rest (nlc_train_select.h select_span).  Element indices are int64.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage): docs/training.md, "Keeping the best weights".
#include <hip/hip_runtime.h>

#include "nlc_train_select.h"

namespace nlc {
namespace train {

__global__ __launch_bounds__(kSelectThreads) void train_keep_best_kernel(const KeepBestArgs a) {
  const int64_t m = blockIdx.y;
  if (!improves(a.loss[m], a.best_loss[m])) return;
  const int64_t beg = (int64_t)blockIdx.x * kSelectChunk;
  if (beg >= a.P) return;
  const int64_t n = a.P - beg < kSelectChunk ? a.P - beg : kSelectChunk;
  const double* s = a.params + m * a.P + beg;
  double* d = a.best_params + m * a.P + beg;
  const SelectSpan sp = select_span((uint64_t)(uintptr_t)s, (uint64_t)(uintptr_t)d, n);
  const int t = threadIdx.x;
  for (int64_t i = t; i < sp.head; i += kSelectThreads) d[i] = s[i];
  const double2* s2 = reinterpret_cast<const double2*>(s + sp.head);
  double2* d2 = reinterpret_cast<double2*>(d + sp.head);
  for (int64_t i = t; i < sp.pairs; i += kSelectThreads) d2[i] = s2[i];
  const int64_t done = sp.head + 2 * sp.pairs;
  for (int64_t i = t; i < sp.tail; i += kSelectThreads) d[done + i] = s[done + i];
}

__global__ __launch_bounds__(kSelectThreads) void train_commit_best_kernel(const KeepBestArgs a) {
  const int64_t m = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x;
  if (m >= a.M) return;
  const double loss = a.loss[m];
  const bool better = improves(loss, a.best_loss[m]);
  if (better) {
    a.best_loss[m] = loss;
    a.best_tag[m] = a.tag;
  }
  if (a.improved) a.improved[m] = better ? 1 : 0;
}

hipError_t launch_train_keep_best(const KeepBestArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(train_keep_best_kernel, dim3((unsigned)select_chunks(a.P), a.M), dim3(kSelectThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_train_commit_best(const KeepBestArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(train_commit_best_kernel, dim3((a.M + kSelectThreads - 1) / kSelectThreads), dim3(kSelectThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace train
}  // namespace nlc
