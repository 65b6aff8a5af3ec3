// Host build of csrc/nlc_devbuf.h (plain C++ under g++) for tests/test_devbuf_host.py: Buf over a counting malloc policy,
// and the two weight folds.  With a main() of its own, so the same file also builds stand-alone (under
// -fsanitize=address,undefined): it runs the buffer's whole life and a "setter" that follows the model setters' commit rule
// (build a local group, move it into the ctx only when nothing failed) with every allocation failing in turn.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "../../neurallaplacecontrol_amd/csrc/nlc_devbuf.h"

using namespace nlc::host;

// malloc / free that count, and fail on request: the allocation `fail_at` calls from now fails (-1: none)
struct CountingMem {
  static long live, allocs, frees, fail_at;
  static int alloc(void** p, size_t bytes) {
    if (fail_at == 0) {
      fail_at = -1;
      return 2;  // (hipErrorOutOfMemory's value; any non-zero status)
    }
    if (fail_at > 0) --fail_at;
    *p = malloc(bytes ? bytes : 1);
    ++live, ++allocs;
    return 0;
  }
  static void free(void* p) {
    ::free(p);
    --live, ++frees;
  }
};
long CountingMem::live = 0, CountingMem::allocs = 0, CountingMem::frees = 0, CountingMem::fail_at = -1;
typedef Buf<double, CountingMem> B;

// ---- the buffer, one operation per entry (Python keeps the handle)
extern "C" void* nlc_t_buf_new(void) { return new B(); }
extern "C" void nlc_t_buf_delete(void* b) { delete (B*)b; }
extern "C" int nlc_t_buf_hold(void* b, long n) { return ((B*)b)->hold((size_t)n); }
extern "C" int nlc_t_buf_grow(void* b, long n) { return ((B*)b)->grow((size_t)n); }
extern "C" void nlc_t_buf_reset(void* b) { ((B*)b)->reset(); }
extern "C" long nlc_t_buf_size(void* b) { return (long)((B*)b)->size(); }
extern "C" void* nlc_t_buf_get(void* b) { return ((B*)b)->get(); }
extern "C" void nlc_t_buf_move(void* dst, void* src) { *(B*)dst = std::move(*(B*)src); }
extern "C" void* nlc_t_buf_move_new(void* src) { return new B(std::move(*(B*)src)); }
extern "C" void nlc_t_fail_at(long k) { CountingMem::fail_at = k; }
extern "C" void nlc_t_counts(long* out) {
  out[0] = CountingMem::live;
  out[1] = CountingMem::allocs;
  out[2] = CountingMem::frees;
}

// ---- the folds
extern "C" void nlc_t_fold_b1(const double* W1s, const double* b1, int h, int S, const double* sph, double* out) {
  std::vector<double> v;
  fold_b1(W1s, b1, h, S, sph, v);
  memcpy(out, v.data(), (size_t)h * sizeof(double));
}
extern "C" void nlc_t_fold_input_bias(const double* Wih, const double* bih, const double* bhh, int rows, int nin,
                                      int gate_rows, double* out) {
  const std::vector<double> v = fold_input_bias(Wih, bih, bhh, rows, nin, gate_rows);
  memcpy(out, v.data(), v.size() * sizeof(double));
}

// ---- a group of three buffers and a setter with the commit rule of nlc_set_model
struct Group {
  bool has = false;
  int tag = 0;
  B a, b, c;
};
static int set_group(Group& ctx, int tag, size_t n) {
  Group m;
  if (int e = m.a.hold(n)) return e;
  if (int e = m.b.hold(2 * n)) return e;
  if (int e = m.c.hold(3 * n)) return e;
  m.has = true;
  m.tag = tag;
  for (size_t i = 0; i < n; ++i) m.a.get()[i] = (double)tag;
  ctx = std::move(m);
  return 0;
}
struct Snapshot {  // (no padding: compared with memcmp)
  int has, tag;
  double *a, *b, *c;
  size_t na, nb, nc;
  double first;
};
static Snapshot snap(const Group& g) {
  return Snapshot{g.has, g.tag, g.a.get(), g.b.get(), g.c.get(), g.a.size(), g.b.size(), g.c.size(), g.a.get() ? g.a.get()[0] : 0.0};
}

#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #x);          \
      return 1;                                              \
    }                                                        \
  } while (0)

static int buffer_life() {
  typedef CountingMem M;
  const long a0 = M::allocs, f0 = M::frees;
  {
    B x;
    CHECK(x.get() == nullptr && x.size() == 0);
    CHECK(x.hold(5) == 0 && x.size() == 5 && M::allocs == a0 + 1);
    x.get()[4] = 1.0;
    CHECK(x.hold(9) == 0 && x.size() == 9 && M::frees == f0 + 1 && M::live == 1);  // replaced: the old block freed once
    x.get()[8] = 1.0;
    double* p = x.get();
    CHECK(x.grow(9) == 0 && x.grow(3) == 0 && x.get() == p && x.size() == 9 && M::allocs == a0 + 2);  // no-op
    CHECK(x.grow(10) == 0 && x.size() == 10 && M::allocs == a0 + 3 && M::frees == f0 + 2);
    p = x.get();
    B y(std::move(x));  // ownership moves, nothing is freed
    CHECK(x.get() == nullptr && x.size() == 0 && y.get() == p && y.size() == 10 && M::frees == f0 + 2);
    B z;
    CHECK(z.hold(2) == 0);
    z = std::move(y);  // the target's own block is freed, once
    CHECK(y.get() == nullptr && y.size() == 0 && z.get() == p && z.size() == 10 && M::frees == f0 + 3 && M::live == 1);
    z.reset();
    z.reset();  // idempotent
    CHECK(z.get() == nullptr && z.size() == 0 && M::frees == f0 + 4 && M::live == 0);
    CHECK(z.hold(4) == 0);
    M::fail_at = 0;
    CHECK(z.hold(6) == 2 && z.get() == nullptr && z.size() == 0 && M::live == 0);  // a failed allocation: empty, reported
    M::fail_at = 0;
    CHECK(z.grow(6) == 2 && z.get() == nullptr && z.size() == 0);
    CHECK(z.grow(6) == 0 && z.size() == 6);
  }
  CHECK(M::live == 0 && M::allocs - a0 == M::frees - f0);
  return 0;
}

static int setter_commit() {
  typedef CountingMem M;
  {
    Group ctx;
    CHECK(set_group(ctx, 1, 8) == 0 && ctx.has && ctx.tag == 1 && M::live == 3);
    const Snapshot before = snap(ctx);
    for (int k = 0; k < 3; ++k) {
      const long frees = M::frees;
      M::fail_at = k;
      CHECK(set_group(ctx, 2, 16) == 2);
      const Snapshot now = snap(ctx);
      CHECK(memcmp(&now, &before, sizeof(Snapshot)) == 0);  // the ctx's group is the one from before, bit for bit
      CHECK(M::live == 3 && M::frees == frees + k);         // and the k blocks of the local group are gone
      CHECK(M::fail_at == -1);
    }
    const long frees = M::frees;
    CHECK(set_group(ctx, 3, 16) == 0);
    CHECK(ctx.tag == 3 && ctx.a.size() == 16 && ctx.c.size() == 48 && ctx.a.get()[0] == 3.0);
    CHECK(M::live == 3 && M::frees == frees + 3);  // the old group's three blocks, freed once each
  }
  CHECK(M::live == 0);
  return 0;
}

int main() {
  if (buffer_life() || setter_commit()) return 1;
  if (CountingMem::live != 0 || CountingMem::allocs != CountingMem::frees) {
    printf("FAILED: %ld live blocks\n", CountingMem::live);
    return 1;
  }
  printf("ok: %ld blocks allocated and freed\n", CountingMem::allocs);
  return 0;
}
