// The value tape of ilt_dehoog_bwd_kernel (kernels_dehoog_bwd.hip): where every entry of a row's quotient-difference table
// sits in a wavefront's slab, how many slabs a launch holds, and so the bytes of scratch it needs.  Plain C++ (constexpr
// functions: host and device alike), because two units size that scratch -- the kernel's launcher, and the training
// workspace of de Hoog models (nlc_train_dehoog.h), which tests/helpers/train_dehoog_host.cpp builds with g++.
#pragma once
#include <stdint.h>

namespace nlc {

struct DhLayout {
  int M;
  // Round 5: the terms a_k and the odd e columns are not taped, and the slab is laid out without them: q columns | even e columns |
  // first entry of every odd e column | A | B -- 466 entries per row at M = 16 instead of 627 (0.49 GB of scratch for 1024 resident
  // wavefronts instead of 0.66).
  // value tape
  constexpr int q(int r, int i) const { return (r - 1) * (2 * M + 2 - r) + i; }                 // r = 1..M, i = 0..2(M-r)+1
  constexpr int even_before(int n) const { return n * (2 * M + 1) - 2 * n * (n + 1); }            // entries of the even columns 2 .. 2n
  constexpr int e(int r, int i) const {                                                          // r = 1..M, i = 0..2(M-r)
    if ((r & 1) == 0) return M * (M + 1) + even_before((r - 2) / 2) + i;
    return M * (M + 1) + even_before(M / 2) + (r - 1) / 2;  // odd column: only i == 0 is taped
  }
  constexpr int e_end() const { return M * (M + 1) + even_before(M / 2) + (M + 1) / 2; }
  constexpr int A(int i) const { return e_end() + (i + 1); }                                     // i = -1..2M-1
  constexpr int B(int i) const { return e_end() + (2 * M + 1) + (i + 1); }                       // i = -1..2M-1
  constexpr int entries() const { return e_end() + 2 * (2 * M + 1); }
};
static_assert(DhLayout{16}.entries() == 466, "compact tape layout at M = 16");
static_assert(DhLayout{16}.e(4, 0) - DhLayout{16}.e(2, 0) == 2 * 14 + 1 && DhLayout{16}.e(16, 0) + 1 == DhLayout{16}.e(1, 0) &&
                  DhLayout{5}.e(5, 0) + 1 == DhLayout{5}.A(-1) && DhLayout{1}.entries() == 2 + 0 + 1 + 6,
              "compact tape layout: columns are contiguous and disjoint");

// a slab entry is (re, im) = 16 bytes per lane, 64 lanes
constexpr int64_t kTapeElemBytes = 16;

// workgroups (= wavefronts of 64 table rows, a slab each) of a backward launch over `rows` (point, dim) rows of S terms
// (slabs in flight, measured at 3.3 M rows, S = 33: 256 -> 36.3 ms, 512 -> 29.8, 768 -> 22.7, 1024 -> 19.8, 2048 (1024
// resident) -> 20.9: fewer slabs would fit the Infinity Cache but starve the latency hiding)
inline unsigned dehoog_bwd_grid(int64_t rows, int S) {
  const int64_t nblk = (rows + 63) / 64;
  const int64_t cap = (S - 1) / 2 <= 8 ? 2048 : 1024;
  return (unsigned)(nblk < cap ? nblk : cap);
}
inline int64_t dehoog_bwd_tape_bytes(int64_t rows, int S) {
  return (int64_t)dehoog_bwd_grid(rows, S) * DhLayout{(S - 1) / 2}.entries() * 64 * kTapeElemBytes;
}

}  // namespace nlc
