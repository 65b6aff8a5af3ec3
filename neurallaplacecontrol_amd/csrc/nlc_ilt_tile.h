// The tiling of the Fourier ILT kernels (kernels_ilt.hip) as functions of the term count S: plain C++17, host and device, no
// HIP, so that tests/helpers/ilt_tile_host.cpp compiles it with g++ and tests/test_ilt_tile_host.py checks it without a GPU --
//   stream_fwd / stream_bwd   block tile of the term-per-lane stream kernels (ilt_fourier_kernel, ilt_fourier_bwd_kernel)
//   RowTile<S>                a wavefront's 64-row tile of the row-per-lane kernels and its LDS slot
//   rows_depth / rows_*_per_cu / rows_grid   launch shape of the row-per-lane kernels
//   rows_fwd_accepts / rows_bwd_accepts      which launches the row-per-lane kernels take; the stream kernels take the rest
// The launchers and the row kernels take these quantities from here and nowhere else.
#pragma once
#include <cstddef>
#include <cstdint>

namespace nlc {

constexpr int kMaxTerms = 129;  // ILT terms the coefficient tables hold

namespace ilt_tile {

// ------------------------------------------------------------------ term-per-lane stream kernels
// A block of 256 threads streams passes of rpp whole rows (rpp * S consecutive doubles, one per active thread), a software
// pipeline 8 passes deep, and one thread per row of the tile forms the row's result: rows = rpp * iters <= 256.
constexpr int kStreamThreads = 256;
constexpr int kStreamDepth = 8;              // passes in flight; iters is a multiple of it
constexpr int kStreamLdsBytes = 60 * 1024;   // forward: the tile's per-term values, row stride S | 1 doubles
constexpr int kStreamMaxTerms = 256;         // a pass holds at least one whole row
struct StreamTile {
  int rpp, iters, rows;  // rows per pass, passes per tile, rows per tile
  size_t lds_bytes;      // dynamic LDS of a workgroup
};
constexpr int stream_rpp(int S) {
  const int rpp = kStreamThreads / S;
  return rpp > 32 ? 32 : rpp;  // rpp * 8 passes must fit the 256 row-sum threads
}
constexpr StreamTile stream_fwd(int S) {
  const int SP = S | 1;
  const int lds_rows = (kStreamLdsBytes / 8) / SP;
  const int max_rows = lds_rows > kStreamThreads ? kStreamThreads : lds_rows;
  const int rpp = stream_rpp(S);
  const int iters = max_rows / rpp / kStreamDepth * kStreamDepth;
  return StreamTile{rpp, iters, rpp * iters, (size_t)(rpp * iters) * SP * sizeof(double)};
}
// backward: LDS holds the rows' scaled upstream gradients only
constexpr StreamTile stream_bwd(int S) {
  const int rpp = stream_rpp(S);
  const int iters = kStreamThreads / rpp / kStreamDepth * kStreamDepth;
  return StreamTile{rpp, iters, rpp * iters, (size_t)(rpp * iters) * sizeof(double)};
}
constexpr bool stream_tile_ok(const StreamTile& t) {
  return t.iters >= kStreamDepth && t.iters % kStreamDepth == 0 && t.rpp >= 1 && t.rpp * kStreamDepth <= kStreamThreads &&
         t.rows <= kStreamThreads && t.lds_bytes <= (size_t)kStreamLdsBytes;
}
constexpr bool stream_tiles_ok(int S_max) {
  for (int S = 1; S <= S_max; ++S)
    if (!stream_tile_ok(stream_fwd(S)) || !stream_tile_ok(stream_bwd(S))) return false;
  return true;
}
// every term count the launchers accept (the ABI stops at kMaxTerms) has a tile: no launch is refused for its tiling
static_assert(kMaxTerms <= kStreamMaxTerms && stream_tiles_ok(kStreamMaxTerms), "stream tiling: iters >= 8, LDS <= 60 KiB");

// ------------------------------------------------------------------ row-per-lane kernels
// A wavefront owns a tile of 64 rows = 64 S consecutive doubles of theta and of phi; a tile lands in the wavefront's LDS slot by
// 16-byte direct loads, 1 KB per instruction.
struct RowGeom {
  int tile;  // bytes of one array's tile
  int slot;  // its LDS slot: the last (partial) load writes a full KB
  int nld;   // whole-wavefront loads of a tile
  int rem;   // bytes of the last, partial one
  int lpt;   // loads per tile and array
};
constexpr RowGeom row_geom(int S) {
  const int tile = 64 * S * 8;
  const int slot = (tile + 1023) / 1024 * 1024;
  return RowGeom{tile, slot, tile / 1024, tile % 1024, slot / 1024};
}
constexpr int kRowWaves = 4;  // wavefronts of a workgroup
// workgroup LDS: DEPTH (theta, phi) slot pairs per wavefront, and the forward's (phase, weight) table behind them
constexpr size_t row_lds_bytes(int S, int depth, bool table) {
  return (size_t)kRowWaves * depth * 2 * row_geom(S).slot + (table ? (size_t)2 * S * 8 : 0);
}
template <int S>
struct RowTile {
  static_assert(S % 2 == 1, "row stride S doubles must be odd: conflict-free row-wise reads, 16-byte tile sizes");
  static constexpr int TILE = row_geom(S).tile, SLOT = row_geom(S).slot, NLD = row_geom(S).nld, REM = row_geom(S).rem,
                       LPT = row_geom(S).lpt;
  static constexpr size_t lds_bytes(int depth, bool table) { return row_lds_bytes(S, depth, table); }
};
// forward: tiles a wavefront keeps in flight -- two where two slot pairs fit four wavefronts' LDS
constexpr int rows_depth(int S) { return S <= 17 ? 2 : 1; }
// workgroups of four wavefronts per CU (launch bounds, LDS)
constexpr int rows_fwd_per_cu(int S, int depth) { return (S <= 17 && depth == 1) ? 2 : 1; }
constexpr int rows_bwd_per_cu(int S) { return S <= 17 ? 2 : 1; }
// persistent grid over `tiles` 64-row tiles: one wavefront per tile, at most per_cu workgroups on each of 256 CUs
constexpr int64_t rows_grid(int64_t tiles, int per_cu) {
  const int64_t want = (tiles + kRowWaves - 1) / kRowWaves, cap = (int64_t)256 * per_cu;
  return want > cap ? cap : want;
}

// odd term counts 3 .. 33: row-wise LDS reads are conflict-free for an odd stride (the reference's default 17, its de Hoog
// ablation's 33, fixed Talbot's 17)
constexpr bool rows_term_count(int S) { return S >= 3 && S <= 33 && (S & 1) != 0; }
// ptr_bits: the OR of the addresses of every array the kernel loads or stores 16 bytes at a time
constexpr bool rows_aligned(uintptr_t ptr_bits) { return (ptr_bits & 15) == 0; }
// forward: any scale and the linear algorithms (both of their tables given)
constexpr bool rows_fwd_accepts(int S, bool lin_wr, bool lin_wi, uintptr_t ptr_bits) {
  return rows_term_count(S) && !(lin_wr && !lin_wi) && rows_aligned(ptr_bits);
}
// ... of which these take the per-term (phase, weight) table instead of the compile-time quarter turns i^k of scale == 2
constexpr bool rows_fwd_general(double scale, bool lin_wr) { return lin_wr || scale != 2.0; }
// backward: the Fourier series at scale == 2 only
constexpr bool rows_bwd_accepts(int S, double scale, uintptr_t ptr_bits) {
  return rows_term_count(S) && scale == 2.0 && rows_aligned(ptr_bits);
}

}  // namespace ilt_tile
}  // namespace nlc
