// GRU encoder, saturated leading steps from a table (option "gru_prefix"): the pure part -- which windows of the MPPI
// history start with clipped actions, and where their precomputed state sits.  No HIP: tests/helpers/gru_prefix_host.cpp
// compiles this with g++ and tests/test_gru_prefix_host.py checks it without a GPU; the kernels (kernels_gru.hip) and the
// planner host (abi_planner_nl.hip) call the same functions.
//
// MPPI clips every perturbed action: perturb_kernel stores clip(u_scale V, u_min, u_max) / u_scale (nlc_mppi_dev.h
// mppi_bound), so a clipped action is stored as exactly u_max / u_scale or u_min / u_scale -- the bound's IMAGE.  The encoder
// consumes a window newest action first from h = 0 (nlc_gru_tile.h); while the consumed actions are images, the two layers'
// hidden states are constants of (weights, bounds, normalisation, pattern of max / min), kept in a table of
// 1 + 2 + 4 + 8 + 16 entries built when the planner is configured -- and with them the hidden-side products of the step that
// follows an entry (below).  nu = 1 only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NLC_PREFIX_HD __host__ __device__
#else
#define NLC_PREFIX_HD
#endif

namespace nlc {
namespace prefix {

constexpr int kMaxLen = 4;                    // leading steps taken from the table, at most
constexpr int kEntries = (2 << kMaxLen) - 1;  // 31: entry 0 is h = 0 (no step taken), then 2^len entries per length
constexpr int kLists = kMaxLen + 1;           // window lists by prefix length 0 .. 4 (a window of length B has no list)
constexpr int kMaxB = 32;                     // the table's own input windows are laid out for action buffers up to this
constexpr int kPatternShift = 27;             // list entry = window index | pattern << 27
constexpr int64_t kMaxWindows = (int64_t)1 << kPatternShift;

NLC_PREFIX_HD inline uint64_t bits_of(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return u;
}
// what perturb_kernel stores for an action clipped at `bound`
NLC_PREFIX_HD inline double bound_image(double bound, double u_scale) { return bound / u_scale; }
NLC_PREFIX_HD inline int cap(int B) { return B < kMaxLen ? B : kMaxLen; }
// lists exist for the lengths below B: 0 .. min(B, 5) - 1
NLC_PREFIX_HD inline int n_lists(int B) { return B < kLists ? B : kLists; }
// table entry of the state after `len` steps whose step s consumed the u_min image iff bit s of `pattern` is set
NLC_PREFIX_HD inline int entry_index(int len, int pattern) { return (1 << len) - 1 + pattern; }

struct Class {
  int len, pattern;
};
// Window (k, t) of the history hist[i] = i < B - 1 ? action_buffer[1 + i] : u_scale * perturbed[k][i - (B - 1)]: GRU step s
// consumes hist[t + B - 1 - s].  len = the number of leading steps s = 0, 1, ... whose element is a stored perturbed value
// equal, bit for bit, to the u_max image or the u_min image; counting stops at the first action-buffer element (whatever its
// value) and at min(B, 4).  Bit s of pattern: step s consumed the u_min image (and not the u_max image: with u_min == u_max
// every bit is 0).  With symmetric bounds that is the element's sign bit.  -0.0 is not +0.0, a NaN is no image.
// `row`: the sample's T stored perturbed values (nu = 1).
NLC_PREFIX_HD inline Class classify(const double* row, int t, int B, uint64_t img_max, uint64_t img_min) {
  Class c{0, 0};
  const int L = cap(B);
  for (int s = 0; s < L; ++s) {
    const int i = t + B - 1 - s;
    if (i < B - 1) break;  // from the action buffer
    const uint64_t v = bits_of(row[i - (B - 1)]);
    if (v == img_max) {
    } else if (v == img_min) {
      c.pattern |= 1 << s;
    } else {
      break;
    }
    c.len = s + 1;
  }
  return c;
}

// ---- the hidden-side products of a table-started tile's first step.  A tile on list len >= 1 runs step s = len first; there
// W_hh0 H0 and W_hh1 H1 are functions of the table entry alone.  The step body (nlc_gru_tile.h) sums "bias + hh" FIRST in every
// accumulation chain, so the table build stores the six accumulator sets (layer 0: r, z from 0 and hn from b_hn; layer 1: r, z,
// hn from their biases) as the full step has them at that point, and the list launch loads them in place of 2 KS 3 GT MFMAs.
// Entries 1 .. 30 have products (entry 0 is h = 0: step 0 has no hidden side; an entry of length B starts no tile and its
// block stays unwritten), 6 g doubles each, in accumulator-register order: a lane (q = lane >> 4) reads register r of gate
// set `set` in {r, z, hn} of layer `layer`'s chunk j -- one aligned 32-byte v4d per set.
NLC_PREFIX_HD inline bool starts_tile(int len, int B) { return len >= 1 && len < n_lists(B); }
// steps the table build runs: one beyond the last image when tiles start from the longest entries (B > 4)
NLC_PREFIX_HD inline int build_steps(int B) { return B <= kMaxLen ? B : kMaxLen + 1; }
NLC_PREFIX_HD inline int64_t products_doubles(int g) { return (int64_t)(kEntries - 1) * 6 * g; }
NLC_PREFIX_HD inline int64_t products_entry_offset(int entry, int g) { return (int64_t)(entry - 1) * 6 * g; }
NLC_PREFIX_HD inline int products_index(int layer, int j, int set, int q, int r, int g) {
  return (((layer * (g / 16) + j) * 3 + set) * 4 + q) * 4 + r;
}

// encoder tiles of the list launch: sum over the lists of ceil(count / 16) <= N / 16 + lists; no count is read back
NLC_PREFIX_HD inline int64_t worst_case_tiles(int64_t N, int B) { return N / 16 + n_lists(B); }

// Why a planner's encoder launch cannot start from the table, or nullptr.  (nin == nu: no encode_obs_time channel.)
inline const char* out_of_scope(int nu, int nin, int has_bounds, int B, int64_t N, bool images_finite) {
  if (nu != 1 || nin != 1) return "gru_prefix: one action dimension and no time channel only (nu == nin == 1)";
  if (!has_bounds) return "gru_prefix: the planner has no action bounds";
  if (B > kMaxB) return "gru_prefix: action buffers of up to 32 rows only";
  if (N > kMaxWindows) return "gru_prefix: at most 2^27 windows per launch";
  if (!images_finite) return "gru_prefix: a bound's normalised image is not finite";
  return nullptr;
}

}  // namespace prefix
}  // namespace nlc
