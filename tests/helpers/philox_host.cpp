// Host build of the library's counter-based generator (neurallaplacecontrol_amd/csrc/nlc_philox.h) for
// tests/test_philox_host.py (g++, no GPU).
#include "../../neurallaplacecontrol_amd/csrc/nlc_philox.h"
using namespace nlc;
extern "C" {
// ctr[4 k ..], key[2 k ..] -> out[4 k ..] = (x, y, z, w)
void nlc_p_philox(const uint32_t* ctr, const uint32_t* key, long n, uint32_t* out) {
  for (long k = 0; k < n; ++k) {
    const u4 r = philox4x32_10(u4{ctr[4 * k], ctr[4 * k + 1], ctr[4 * k + 2], ctr[4 * k + 3]}, key[2 * k], key[2 * k + 1]);
    out[4 * k] = r.x;
    out[4 * k + 1] = r.y;
    out[4 * k + 2] = r.z;
    out[4 * k + 3] = r.w;
  }
}
void nlc_p_u53(const uint32_t* hi, const uint32_t* lo, long n, double* out) {
  for (long k = 0; k < n; ++k) out[k] = u53(hi[k], lo[k]);
}
}
