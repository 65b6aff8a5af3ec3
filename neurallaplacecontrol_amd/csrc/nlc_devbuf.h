// The parts of nlc_host.h that compile without HIP, for the g++ build of tests/helpers/devbuf_host.cpp: the one owner of a
// device or pinned allocation, and the two weight folds whose bits a model upload must keep.  No kernel unit includes this.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace nlc {
namespace host {

// Owns one allocation of size() elements: movable, not copyable, freed by reset() / the destructor.  Mem is alloc(void**,
// bytes) -> status (0 = ok) and free(void*): HIP's below, a counting malloc in the CPU test.  hold / grow return Mem's
// status; a failed allocation leaves the buffer empty.
template <class T, class Mem>
class Buf {
  T* p_ = nullptr;
  size_t n_ = 0;

 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {  // (declaring the moves deletes the copies)
    Buf old(std::move(*this));
    p_ = std::exchange(o.p_, nullptr), n_ = std::exchange(o.n_, 0);
    return *this;
  }
  ~Buf() { reset(); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  void reset() {
    if (p_) Mem::free(p_);
    p_ = nullptr, n_ = 0;
  }
  // exactly n elements: frees what it held, then allocates
  int hold(size_t n) {
    reset();
    void* q = nullptr;
    if (int e = Mem::alloc(&q, n * sizeof(T))) return e;
    p_ = static_cast<T*>(q), n_ = n;
    return 0;
  }
  // at least n elements: nothing happens while n <= size()
  int grow(size_t n) { return n <= n_ ? 0 : hold(n); }
};

#if defined(__HIP__)
struct DeviceMem {
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
// mapped, coherent pinned host memory
struct PinnedMem {
  static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static void free(void* p) { (void)hipHostFree(p); }
};
using DevDoubles = Buf<double, DeviceMem>;
using DevInts = Buf<int, DeviceMem>;
using PinnedDoubles = Buf<double, PinnedMem>;
#endif

// Constant prediction time => the 2S sphere-coordinate inputs `sph` of layer 1 are constants: they fold into its bias.
// W1s is (h, 2S) row-major.  One accumulator seeded with b1[r], j ascending: that order is the folded bias's bits.
inline void fold_b1(const double* W1s, const double* b1, int h, int S, const double* sph, std::vector<double>& out) {
  out.resize(h);
  for (int r = 0; r < h; ++r) {
    double acc = b1[r];
    for (int j = 0; j < 2 * S; ++j) acc += W1s[(size_t)r * 2 * S + j] * sph[j];
    out[r] = acc;
  }
}

// A GRU's layer-0 input weights (rows, nin) as the (rows, 4) matrix the encoders take, x = [a_0..a_{nin-1}, 0.., 1]: the
// bias rides in column 3, with the hidden-side bias of the first gate_rows rows (the r and z gates) added to it.
inline std::vector<double> fold_input_bias(const double* Wih, const double* bih, const double* bhh, int rows, int nin,
                                           int gate_rows) {
  std::vector<double> W((size_t)rows * 4, 0.0);
  for (int r = 0; r < rows; ++r) {
    for (int j = 0; j < nin; ++j) W[(size_t)r * 4 + j] = Wih[(size_t)r * nin + j];
    W[(size_t)r * 4 + 3] = bih[r] + (r < gate_rows ? bhh[r] : 0.0);
  }
  return W;
}

}  // namespace host
}  // namespace nlc
