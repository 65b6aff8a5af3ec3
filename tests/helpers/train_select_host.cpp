// Host build of the snapshot-selection rule and copy plan (csrc/nlc_train_select.h, plain C++) for
// tests/test_train_select_host.py.  With a main() of its own, so the same file also builds stand-alone (under
// -fsanitize=address,undefined): it runs the kernels' two loops on the host over guarded buffers for a sweep of row lengths
// and both row parities.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../neurallaplacecontrol_amd/csrc/nlc_train_select.h"

using namespace nlc::train;

// out[i] = improves(loss[i], best[i])
extern "C" void nlc_t_improves(const double* loss, const double* best, int32_t* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = improves(loss[i], best[i]) ? 1 : 0;
}

extern "C" int64_t nlc_t_select_chunks(int64_t P) { return select_chunks(P); }

// out = head, pairs, tail
extern "C" void nlc_t_select_span(uint64_t s_addr, uint64_t d_addr, int64_t n, int64_t* out) {
  const SelectSpan sp = select_span(s_addr, d_addr, n);
  out[0] = sp.head;
  out[1] = sp.pairs;
  out[2] = sp.tail;
}

// what the two launches do, member by member and chunk by chunk, with the kernels' index arithmetic; 16-byte accesses are
// checked for alignment instead of made
static int keep_best_host(const KeepBestArgs& a) {
  for (int64_t m = 0; m < a.M; ++m) {
    if (!improves(a.loss[m], a.best_loss[m])) continue;
    for (int64_t c = 0; c < select_chunks(a.P); ++c) {
      const int64_t beg = c * kSelectChunk;
      const int64_t n = a.P - beg < kSelectChunk ? a.P - beg : kSelectChunk;
      const double* s = a.params + m * a.P + beg;
      double* d = a.best_params + m * a.P + beg;
      const SelectSpan sp = select_span((uint64_t)(uintptr_t)s, (uint64_t)(uintptr_t)d, n);
      if (sp.head + 2 * sp.pairs + sp.tail != n || sp.head < 0 || sp.pairs < 0 || sp.tail < 0) return 1;
      for (int64_t i = 0; i < sp.head; ++i) d[i] = s[i];
      if (sp.pairs > 0 && ((((uintptr_t)(s + sp.head)) | ((uintptr_t)(d + sp.head))) & 15) != 0) return 2;
      memcpy(d + sp.head, s + sp.head, (size_t)sp.pairs * 16);
      const int64_t done = sp.head + 2 * sp.pairs;
      for (int64_t i = 0; i < sp.tail; ++i) d[done + i] = s[done + i];
    }
  }
  for (int64_t m = 0; m < a.M; ++m) {
    const bool better = improves(a.loss[m], a.best_loss[m]);
    if (better) {
      a.best_loss[m] = a.loss[m];
      a.best_tag[m] = a.tag;
    }
    if (a.improved) a.improved[m] = better ? 1 : 0;
  }
  return 0;
}

int main() {
  const int M = 4;
  const int64_t Ps[] = {1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4099};
  for (int64_t P : Ps)
    for (int soff = 0; soff < 2; ++soff)
      for (int doff = 0; doff < 2; ++doff) {
        // exact-size heap blocks: a step past either end is an ASan report
        std::vector<double> src(M * P + soff), dst(M * P + doff, -1.0);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (double)i;
        double loss[M] = {1.0, 2.0, 0.5, 3.0}, best[M] = {2.0, 2.0, 1.0, 1.0};
        int64_t tag[M] = {-1, -1, -1, -1};
        int32_t imp[M];
        const KeepBestArgs a{loss, src.data() + soff, best, dst.data() + doff, tag, imp, P, 7, M};
        if (int rc = keep_best_host(a)) {
          printf("bad span P=%lld soff=%d doff=%d rc=%d\n", (long long)P, soff, doff, rc);
          return 1;
        }
        for (int m = 0; m < M; ++m) {
          const bool want = m == 0 || m == 2;
          for (int64_t i = 0; i < P; ++i)
            if (dst[doff + m * P + i] != (want ? src[soff + m * P + i] : -1.0)) {
              printf("bad copy P=%lld soff=%d doff=%d m=%d i=%lld\n", (long long)P, soff, doff, m, (long long)i);
              return 1;
            }
          if (imp[m] != (int)want || tag[m] != (want ? 7 : -1)) return 1;
        }
      }
  printf("ok\n");
  return 0;
}
