// Device build (gfx950) of the kernel math, for tests/test_gpu_math_device.py: the extern "C" symbols of
// tests/helpers/math_host.cpp and tests/helpers/exp_ratio_host.cpp with the same signatures, plus the device-only forms of
// nlc_gru_tile.h, nlc_rollout.h and nlc_cplx.h.  Every entry copies its inputs to the device, runs ONE kernel -- one thread per
// element, 256-thread blocks, guarded ragged tail -- that calls the shipped inline function from the shipped header, and copies
// the result back; it returns 0, or non-zero when a HIP call failed (or, nlc_t_exp_ratio, when the two instantiations of
// exp_ratio_parts disagree).  Compiled with the library's flags (csrc/Makefile, target `tools`), so contraction is the library's.
// Not part of libnlc_hip.so.
//   make -C neurallaplacecontrol_amd/csrc tools   ->   tools/libnlc_math_dev.so
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "nlc_cplx.h"
#include "nlc_gru_tile.h"
#include "nlc_rollout.h"
#include "nlc_math_table.h"  // tools/: tanh_t / sigmoid_t

using namespace nlc;

namespace {

constexpr int kMaxIn = 5, kMaxOut = 3;
struct Ptrs {
  const double* in[kMaxIn];
  double* out[kMaxOut];
  int* bad;  // entries that count disagreements add to it
};
struct In {
  const double* host;
  long count;
};
struct Out {
  double* host;
  long count;
};

template <class F>
__global__ void __launch_bounds__(256) per_element(Ptrs p, long threads, F f) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < threads) f(p, i);
}

struct DevMem {
  void* ptr[kMaxIn + kMaxOut + 1] = {};
  int n = 0;
  ~DevMem() {
    for (int i = 0; i < n; ++i) (void)hipFree(ptr[i]);
  }
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 8);
    if (e == hipSuccess) ptr[n++] = *p;
    return e;
  }
};

// 0: done; 1: a HIP call failed; 2: the kernel counted disagreements
template <class F>
int run(std::initializer_list<In> ins, std::initializer_list<Out> outs, long threads, F f) {
  if (threads <= 0) return 0;
  if ((int)ins.size() > kMaxIn || (int)outs.size() > kMaxOut || threads > (1L << 31)) return 1;
  DevMem mem;
  Ptrs p = {};
  int k = 0;
  for (const In& s : ins) {
    void* d = nullptr;
    if (mem.alloc(&d, s.count * sizeof(double)) != hipSuccess) return 1;
    if (s.count > 0 && hipMemcpy(d, s.host, s.count * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 1;
    p.in[k++] = static_cast<const double*>(d);
  }
  k = 0;
  for (const Out& s : outs) {
    void* d = nullptr;
    if (mem.alloc(&d, s.count * sizeof(double)) != hipSuccess) return 1;
    p.out[k++] = static_cast<double*>(d);
  }
  void* bad = nullptr;
  if (mem.alloc(&bad, sizeof(int)) != hipSuccess) return 1;
  if (hipMemset(bad, 0, sizeof(int)) != hipSuccess) return 1;
  p.bad = static_cast<int*>(bad);
  per_element<<<dim3((unsigned)((threads + 255) / 256)), dim3(256)>>>(p, threads, f);
  if (hipGetLastError() != hipSuccess) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  k = 0;
  for (const Out& s : outs) {
    if (s.count > 0 && hipMemcpy(s.host, p.out[k], s.count * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    ++k;
  }
  int nbad = 0;
  if (hipMemcpy(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return nbad ? 2 : 0;
}

__device__ const double kTab[64] = {NLC_EXP_TABLE_VALUES};

__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

}  // namespace

// y[i] = EXPR of x = x[i], one thread per element
#define NLC_T_UNARY(name, EXPR)                                                                   \
  extern "C" int name(const double* x, double* y, long n) {                                       \
    return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {                      \
      const double x = p.in[0][i];                                                                \
      p.out[0][i] = (EXPR);                                                                       \
    });                                                                                           \
  }

// ---- the symbols of tests/helpers/math_host.cpp
NLC_T_UNARY(nlc_t_tanh, m::tanh_d(x))
NLC_T_UNARY(nlc_t_sigmoid, m::sigmoid_d(x))
NLC_T_UNARY(nlc_t_exp, m::exp_d(x))
NLC_T_UNARY(nlc_t_tan, m::tan_0_halfpi(x))
NLC_T_UNARY(nlc_t_tan_pi4, m::tan_pi4_plus(x))
NLC_T_UNARY(nlc_t_tanh_t, m::tanh_t(x, kTab))
NLC_T_UNARY(nlc_t_sigmoid_t, m::sigmoid_t(x, kTab))
extern "C" int nlc_t_sin(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    double s, c;
    m::sincos_bounded(p.in[0][i], &s, &c);
    p.out[0][i] = s;
  });
}
extern "C" int nlc_t_cos(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    double s, c;
    m::sincos_bounded(p.in[0][i], &s, &c);
    p.out[0][i] = c;
  });
}
extern "C" int nlc_t_cosq(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) { p.out[0][i] = m::cos_quadrant(p.in[0][i], (int)(i % 7) - 3); });
}
// short forms of the Fourier ILT kernel: cos(x + m pi/2) with m = i & 1, tan(x) on [0, pi/2] as num/den
extern "C" int nlc_t_cos_mpio2(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    const double dm = (double)(i & 1);
    p.out[0][i] = m::cos_plus_mpio2(m::ilt_trig_k(), p.in[0][i], 0.5 * dm, dm);
  });
}
extern "C" int nlc_t_sin_mpio2(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    const double dm = (double)(i & 1);
    double sn, cs;
    m::sincos_plus_mpio2(m::ilt_trig_k(), p.in[0][i], 0.5 * dm, dm, &sn, &cs);
    p.out[0][i] = sn;
  });
}
extern "C" int nlc_t_tan_short(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    double num, den;
    m::tan_parts_short(m::ilt_trig_k(), p.in[0][i], &num, &den);
    p.out[0][i] = num / den;
  });
}
// the row-per-lane Fourier ILT kernel's forms: tan(pi/4 + a) as num/den, cos(x + m pi/2) with m = i & 1, sin and cos by one reduction
extern "C" int nlc_t_tan_rat(const double* a, double* y, long n) {
  return run({{a, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    double num, den;
    m::tan_parts_rat(m::ilt_row_k(), p.in[0][i], &num, &den);
    p.out[0][i] = num / den;
  });
}
extern "C" int nlc_t_cos_kpio2(const double* x, double* y, long n) {
  return run({{x, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) {
    const double x = p.in[0][i];
    p.out[0][i] = (i & 1) ? -m::cos_or_sin_reduced<1>(m::ilt_row_k(), x) : m::cos_or_sin_reduced<0>(m::ilt_row_k(), x);
  });
}
extern "C" int nlc_t_sincos_reduced(const double* x, double* sn, double* cs, long n) {
  return run({{x, n}}, {{sn, n}, {cs, n}}, n,
             [] __device__(const Ptrs& p, long i) { m::sincos_reduced(m::ilt_row_k(), p.in[0][i], &p.out[0][i], &p.out[1][i]); });
}

// pairs (x[i], x[i + 1]), i even; an odd n pairs its last element with 0.  Each thread evaluates its element's pair and keeps
// its own half.
#define NLC_T_PAIR(name, FN)                                                                      \
  extern "C" int name(const double* x, double* y, long n) {                                       \
    return run({{x, n}}, {{y, n}}, n, [n] __device__(const Ptrs& p, long i) {                     \
      const long a = i & ~1L;                                                                     \
      double ta, tb;                                                                              \
      FN(p.in[0][a], a + 1 < n ? p.in[0][a + 1] : 0.0, &ta, &tb);                                 \
      p.out[0][i] = (i & 1) ? tb : ta;                                                            \
    });                                                                                           \
  }
NLC_T_PAIR(nlc_t_tanh_pair_fast, m::tanh_pair_fast)
NLC_T_PAIR(nlc_t_tanh_pair_d, m::tanh_pair_d)

NLC_T_UNARY(nlc_t_exp_neg, m::exp_neg(x))
NLC_T_UNARY(nlc_t_expm1_neg, m::expm1_neg(x))
NLC_T_UNARY(nlc_t_rcp_refined, m::rcp_refined(x))
NLC_T_UNARY(nlc_t_min_abs, m::min_abs(x, 372.5))
extern "C" int nlc_t_div_fast(const double* num, const double* den, double* y, long n) {
  return run({{num, n}, {den, n}}, {{y, n}}, n, [] __device__(const Ptrs& p, long i) { p.out[0][i] = m::div_fast(p.in[0][i], p.in[1][i]); });
}

// ---- the symbols of tests/helpers/exp_ratio_host.cpp
// e^y = 2^n num / den: m[i] = 2^n num, d[i] = den (half = 0), or from the half argument y / 2 (half = 1, tanh's form).  Both
// instantiations of exp_ratio_parts run -- the scalar one on y[i], the two-wide one on (y[i], y[i + 1]) -- and every number they
// return must agree bit for bit (else: return 2).
extern "C" int nlc_t_exp_ratio(const double* y, double* mm, double* d, long n, int half) {
  return run({{y, n}}, {{mm, n}, {d, n}}, n, [n, half] __device__(const Ptrs& p, long i) {
    const long j = i + 1 < n ? i + 1 : i;
    const double y0 = p.in[0][i], y1 = p.in[0][j];
    double num, den, sh, num1, den1, sh1;
    m::v2d_e N2, D2, S2;
    if (half) {
      m::exp_ratio_parts<true>(0.5 * y0, &num, &den, &sh);
      m::exp_ratio_parts<true>(0.5 * y1, &num1, &den1, &sh1);
      m::exp_ratio_parts<true>(m::v2d_e{0.5 * y0, 0.5 * y1}, &N2, &D2, &S2);
    } else {
      m::exp_ratio_parts<false>(y0, &num, &den, &sh);
      m::exp_ratio_parts<false>(y1, &num1, &den1, &sh1);
      m::exp_ratio_parts<false>(m::v2d_e{y0, y1}, &N2, &D2, &S2);
    }
    const bool same = same_bits(num, N2.x) && same_bits(den, D2.x) && same_bits(sh, S2.x) && same_bits(num1, N2.y) &&
                      same_bits(den1, D2.y) && same_bits(sh1, S2.y);
    if (!same) atomicAdd(p.bad, 1);
    p.out[0][i] = ldexp(num, m::exp_shift_int(sh));
    p.out[1][i] = den;
  });
}
// sigmoid_pair2 on (x[i], x[i + 1]) as (a, b) of one hidden unit and (x[i + 2], x[i + 3]) as the other's; whole groups of four only
extern "C" int nlc_t_sigmoid_ratio(const double* x, double* y, long n) {
  const long whole = n & ~3L;
  return run({{x, n}}, {{y, whole}}, whole, [] __device__(const Ptrs& p, long i) {
    const long g = i & ~3L;
    const double* x = p.in[0] + g;
    v2d sa, sb;
    sigmoid_pair2(v2d{x[0], x[2]}, v2d{x[1], x[3]}, &sa, &sb);
    const double r[4] = {sa.x, sb.x, sa.y, sb.y};
    p.out[0][i] = r[i & 3];
  });
}
// tanh2 on (x[i], x[i + 1]); whole pairs only
extern "C" int nlc_t_tanh_ratio(const double* x, double* y, long n) {
  const long whole = n & ~1L;
  return run({{x, n}}, {{y, whole}}, whole, [] __device__(const Ptrs& p, long i) {
    const long a = i & ~1L;
    const v2d t = tanh2(v2d{p.in[0][a], p.in[0][a + 1]});
    p.out[0][i] = (i & 1) ? t.y : t.x;
  });
}

// ---- device-only forms
NLC_T_UNARY(nlc_t_rcp_refined1, rcp_refined1(x))
NLC_T_UNARY(nlc_t_min_neg, min_neg(x, 170.0))
NLC_T_UNARY(nlc_t_sphere_theta, sphere_theta(x))
NLC_T_UNARY(nlc_t_sphere_phi, sphere_phi(x))
NLC_T_UNARY(nlc_t_sphere_tan_arg, sphere_tan_arg(x))
extern "C" int nlc_t_sphere_term(const double* theta, const double* phi, double* y, long n, int odd) {
  return run({{theta, n}, {phi, n}}, {{y, n}}, n,
             [odd] __device__(const Ptrs& p, long i) { p.out[0][i] = sphere_term(p.in[0][i], p.in[1][i], odd != 0); });
}
extern "C" int nlc_t_sphere_terms_lin(const double* theta, const double* phi, double* rc, double* rs, long n) {
  return run({{theta, n}, {phi, n}}, {{rc, n}, {rs, n}}, n,
             [] __device__(const Ptrs& p, long i) { sphere_terms_lin(p.in[0][i], p.in[1][i], &p.out[0][i], &p.out[1][i]); });
}
// gru_gates on the four hidden units (i, i + 1, i + 2, i + 3), i a multiple of four: two pairs, as the encoder's accumulator
// registers hold them; a ragged last group is padded with zeros.  Each thread evaluates its element's group and keeps its own h'.
extern "C" int nlc_t_gru_gates(const double* ar, const double* az, const double* ain, const double* ahn, const double* hold, double* h,
                               long n) {
  return run({{ar, n}, {az, n}, {ain, n}, {ahn, n}, {hold, n}}, {{h, n}}, n, [n] __device__(const Ptrs& p, long i) {
    const long g = i & ~3L;
    v4d v[5];
    for (int a = 0; a < 5; ++a)
      for (int k = 0; k < 4; ++k) v[a][k] = g + k < n ? p.in[a][g + k] : 0.0;
    const v4d hn = gru_gates(v[0], v[1], v[2], v[3], v[4]);
    p.out[0][i] = hn[i & 3];
  });
}
// complex numbers interleaved (re, im); n of them
extern "C" int nlc_t_cmul(const double* a, const double* b, double* y, long n) {
  return run({{a, 2 * n}, {b, 2 * n}}, {{y, 2 * n}}, n, [] __device__(const Ptrs& p, long i) {
    const cplx r = cmul(cplx{p.in[0][2 * i], p.in[0][2 * i + 1]}, cplx{p.in[1][2 * i], p.in[1][2 * i + 1]});
    p.out[0][2 * i] = r.re;
    p.out[0][2 * i + 1] = r.im;
  });
}
extern "C" int nlc_t_cdiv(const double* a, const double* b, double* y, long n) {
  return run({{a, 2 * n}, {b, 2 * n}}, {{y, 2 * n}}, n, [] __device__(const Ptrs& p, long i) {
    const cplx r = cdiv(cplx{p.in[0][2 * i], p.in[0][2 * i + 1]}, cplx{p.in[1][2 * i], p.in[1][2 * i + 1]});
    p.out[0][2 * i] = r.re;
    p.out[0][2 * i + 1] = r.im;
  });
}
extern "C" int nlc_t_csqrt(const double* z, double* y, long n) {
  return run({{z, 2 * n}}, {{y, 2 * n}}, n, [] __device__(const Ptrs& p, long i) {
    const cplx r = csqrt_(cplx{p.in[0][2 * i], p.in[0][2 * i + 1]});
    p.out[0][2 * i] = r.re;
    p.out[0][2 * i + 1] = r.im;
  });
}
