// The counter-based generator behind every device draw (planner sampling, expert collector, synthetic dataset).  Plain C++17:
// tests/helpers/philox_host.cpp compiles the same functions with g++ and tests/test_philox_host.py checks them on the CPU.
#pragma once
#include <stdint.h>

#include "nlc_math.h"

namespace nlc {

// ---- Philox4x32-10 (Salmon et al. 2011), counter-based so a K-shard reproduces the unsharded stream
struct u4 {
  uint32_t x, y, z, w;
};
NLC_HD u4 philox4x32_10(u4 ctr, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)M0 * ctr.x, p1 = (uint64_t)M1 * ctr.z;
    u4 n;
    n.x = (uint32_t)(p1 >> 32) ^ ctr.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ ctr.w ^ k1;
    n.w = (uint32_t)p0;
    ctr = n;
    k0 += W0;
    k1 += W1;
  }
  return ctr;
}
// two uint32 -> uniform double in (0,1): 53 random bits, never 0 and never 1.  v + 0.5 is exact below 2^52 and rounds to
// nearest-even above; v = 2^53 - 1 alone would round to 2^53, that is to 1.0 (log(u) = 0: a zero interval), and takes the
// double below 1 instead
NLC_HD double u53(uint32_t hi, uint32_t lo) {
  const uint64_t v = (((uint64_t)hi << 32) | lo) >> 11;
  return fmin(((double)v + 0.5) * (1.0 / 9007199254740992.0), 0x1.fffffffffffffp-1);
}

}  // namespace nlc
