// glibc_math_unit.hip — the libm replicas of csrc/glibc_math.h and
// csrc/glibc_math_f64.h as the gfx950 compile of the kernel source runs them,
// function by function against the host pass of the same functions and against
// the host libm.  The functions are the kernels' own: this file includes
// ctcx_decode.hip with CTCX_PART=99 (device functions only) and is built by
// csrc/Makefile with the library's $(FLAGS), so a change of -ffp-contract or of
// the denormal mode there changes this binary too.
//
// Per input, bit for bit (all NaNs one value):
//   (a) the device result, one input per thread, expf's table staged in LDS as
//       the kernels stage it;
//   (b) the host pass of the same header function (widen_* are __device__ only:
//       no host pass exists, (b) is (c) there);
//   (c) the host libm: ::expf ::logf ::log1pf ::exp ::log; for lse the formula of
//       oracle/ctc_oracle.cpp over libm calls; for the widenings plain C++.
//
//   glibc_math_unit.bin        device mode over the sampled sets and bands below
//   glibc_math_unit.bin host   the same sets, (b) against (c) only: no HIP API call
//   glibc_math_unit.bin all    the float functions and expf_t* over all 2^32
//                              patterns (manual run; result recorded in DESIGN.md)
//
// One line per function:
//   name inputs=N subnormal_results=K ... device_vs_host=.. device_vs_libm=.. host_vs_libm=..
// The census counts come from the inputs and from libm's results only.
// Exit status: 1 on a mismatch, 2 on a HIP error (nothing is launched after it).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <limits>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../ctc-beam-search-op_amd/csrc/ctcx_decode.hip"

namespace gm = ctcx::gm;

#define HIP_OK(e)                                                                              \
  do {                                                                                         \
    const hipError_t err_ = (e);                                                               \
    if (err_ != hipSuccess) {                                                                  \
      printf("glibc_math_unit: %s at line %d\n", hipGetErrorString(err_), __LINE__);           \
      fflush(stdout);                                                                          \
      _Exit(2);                                                                                \
    }                                                                                          \
  } while (0)

static uint64_t g_tab[32];   // the host pass's copy of expf's table
static bool g_host_only = false;
static int g_nthr = 1;

// results as bit patterns, all NaNs one value
__host__ __device__ static uint32_t canon(float f) { return f != f ? 0x7fc00000u : gm::f2u(f); }
__host__ __device__ static uint64_t canon(double d) { return d != d ? 0x7ff8000000000000ull : gm::d2u(d); }

// census slots 0..3 of every function: libm's results by class
static void cls(uint32_t r, uint64_t* c) {
  const uint32_t a = r & 0x7fffffffu;
  c[0] += a != 0 && a < 0x00800000u;
  c[1] += a == 0;
  c[2] += a == 0x7f800000u;
  c[3] += a > 0x7f800000u;
}
static void cls(uint64_t r, uint64_t* c) {
  const uint64_t a = r & 0x7fffffffffffffffull;
  c[0] += a != 0 && a < 0x0010000000000000ull;
  c[1] += a == 0;
  c[2] += a == 0x7ff0000000000000ull;
  c[3] += a > 0x7ff0000000000000ull;
}
static const char* const kCls[4] = {"subnormal_results", "zero_results", "inf_results", "nan_results"};
constexpr int kMaxCensus = 16;

// ---- the functions under test ------------------------------------------------
// I / O: input and output as bit patterns; dom: the documented domain; dev: the
// device form (etab: the LDS table); host: (b); libm: (c); census: slots 4.. from
// the input and libm's result r; extra: their names.
struct F32 {
  typedef uint32_t I;
  typedef uint32_t O;
  static bool dom(I) { return true; }
  static void show_in(I u, char* s) { sprintf(s, "%a", gm::u2f(u)); }
  static void show_out(O u, char* s) { sprintf(s, "%a", gm::u2f(u)); }
  static void census(I, O r, uint64_t* c) { cls(r, c); }
  static const char* const* extra(int& n) { n = 0; return nullptr; }
};
struct FExpf : F32 {
  static const char* name() { return "expf"; }
  __device__ static O dev(I u, uint64_t*) { return canon(gm::expf(gm::u2f(u))); }
  static O host(I u) { return canon(gm::expf(gm::u2f(u))); }
  static O libm(I u) { return canon(::expf(gm::u2f(u))); }
};
struct FLogf : F32 {
  static const char* name() { return "logf"; }
  __device__ static O dev(I u, uint64_t*) { return canon(gm::logf(gm::u2f(u))); }
  static O host(I u) { return canon(gm::logf(gm::u2f(u))); }
  static O libm(I u) { return canon(::logf(gm::u2f(u))); }
};
struct FLog1pf : F32 {
  static const char* name() { return "log1pf"; }
  __device__ static O dev(I u, uint64_t*) { return canon(gm::log1pf(gm::u2f(u))); }
  static O host(I u) { return canon(gm::log1pf(gm::u2f(u))); }
  static O libm(I u) { return canon(::log1pf(gm::u2f(u))); }
  // the input range of each return path of s_log1pf.c, from the input alone
  static void census(I u, O r, uint64_t* c) {
    cls(r, c);
    const uint32_t ax = u & 0x7fffffffu;
    const bool neg = u >> 31;
    const float x = gm::u2f(u);
    if (neg && ax >= 0x3f800000u) { c[x == -1.0f ? 4 : 5]++; return; }   // -inf; NaN (x < -1, negative NaNs)
    if (!neg && ax >= 0x7f800000u) { c[6]++; return; }                    // x + x
    if (ax < 0x24800000u) { c[7]++; return; }                             // x
    if (ax < 0x31000000u) { c[8]++; return; }                             // x - x * x * 0.5f
    if (neg ? u <= 0xbe95f61fu : u < 0x3ed413d7u) { c[9]++; return; }     // k = 0, f = x
    uint32_t hu;
    if (u < 0x5a000000u || neg) { c[10]++; hu = gm::f2u(1.0f + x); }      // u = 1 + x, c /= u
    else { c[11]++; hu = u; }                                             // u = x
    hu &= 0x007fffffu;
    c[hu < 0x3504f7u ? 12 : 13]++;                                        // the mantissa split
    if (hu == 0) c[14]++;                                                 // f == 0
    if (hu >= 0x7ffffdu) c[15]++;                                         // hu == 0 with f != 0
  }
  static const char* const* extra(int& n) {
    static const char* const k[] = {"in_minus1", "in_nan", "in_posinfnan", "in_lt2m54", "in_lt2m29", "in_k0", "in_1px",
                                    "in_ge2p53", "in_mant_lo", "in_mant_hi", "in_f0", "in_fsmall"};
    n = 12;
    return k;
  }
};
struct FExpfT : F32 {
  static const char* name() { return "expf_t"; }
  __device__ static O dev(I u, uint64_t* etab) { return canon(gm::expf_t(gm::u2f(u), etab)); }
  static O host(I u) { return canon(gm::expf_t(gm::u2f(u), (const uint64_t*)g_tab)); }
  static O libm(I u) { return canon(::expf(gm::u2f(u))); }
};
struct FExpfNonpos : FExpfT {
  static const char* name() { return "expf_t_nonpos"; }
  static bool dom(I u) { const float x = gm::u2f(u); return x <= 0.0f || x != x; }
  __device__ static O dev(I u, uint64_t* etab) { return canon(gm::expf_t_nonpos(gm::u2f(u), etab)); }
  static O host(I u) { return canon(gm::expf_t_nonpos(gm::u2f(u), (const uint64_t*)g_tab)); }
};
struct FExpfLe0 : FExpfT {
  static const char* name() { return "expf_t_le0"; }
  static bool dom(I u) { return gm::u2f(u) <= 0.0f; }
  __device__ static O dev(I u, uint64_t* etab) { return canon(gm::expf_t_le0(gm::u2f(u), etab)); }
  static O host(I u) { return canon(gm::expf_t_le0(gm::u2f(u), (const uint64_t*)g_tab)); }
};
struct FExpfCore : FExpfT {
  static const char* name() { return "expf_t_core"; }
  static bool dom(I u) { const float x = gm::u2f(u); return x <= 0.0f && x >= gm::kExpfUnder; }
  __device__ static O dev(I u, uint64_t* etab) { return canon(gm::expf_t_core(gm::u2f(u), etab)); }
  static O host(I u) { return canon(gm::expf_t_core(gm::u2f(u), (const uint64_t*)g_tab)); }
};

struct F64 {
  typedef uint64_t I;
  typedef uint64_t O;
  static bool dom(I) { return true; }
  static void show_in(I u, char* s) { sprintf(s, "%a", gm::u2d(u)); }
  static void show_out(O u, char* s) { sprintf(s, "%a", gm::u2d(u)); }
  static const char* const* extra(int& n) { n = 0; return nullptr; }
};
struct FExp : F64 {
  static const char* name() { return "exp"; }
  __device__ static O dev(I u, uint64_t*) { return canon(gm::exp(gm::u2d(u))); }
  static O host(I u) { return canon(gm::exp(gm::u2d(u))); }
  static O libm(I u) { return canon(::exp(gm::u2d(u))); }
  static void census(I u, O r, uint64_t* c) {
    cls(r, c);
    const uint32_t abstop = (uint32_t)(u >> 52) & 0x7ffu;
    c[4] += abstop == 0x408u;   // 512 <= |x| < 1024: e_exp.c's specialcase
    c[5] += abstop < 0x3c9u;                             // |x| < 2^-54
  }
  static const char* const* extra(int& n) {
    static const char* const k[] = {"in_special", "in_lt2m54"};
    n = 2;
    return k;
  }
};
struct FLog : F64 {
  static const char* name() { return "log"; }
  __device__ static O dev(I u, uint64_t*) { return canon(gm::log(gm::u2d(u))); }
  static O host(I u) { return canon(gm::log(gm::u2d(u))); }
  static O libm(I u) { return canon(::log(gm::u2d(u))); }
  static void census(I u, O r, uint64_t* c) {
    cls(r, c);
    c[4] += u - 0x3fee000000000000ull <= 0x308ffffffffffull;                 // the near-1 polynomial
    c[5] += (u << 1) != 0 && (u & 0x7ff0000000000000ull) == 0 && !(u >> 63);  // positive subnormal: rescaled
    c[6] += (u >> 63) && (u << 1) != 0 && (u << 1) <= 0xffe0000000000000ull;  // x < 0: (x - x) / (x - x)
  }
  static const char* const* extra(int& n) {
    static const char* const k[] = {"in_near1", "in_subnormal", "in_negative"};
    n = 3;
    return k;
  }
};

// lse: the formula as oracle/ctc_oracle.cpp states it (float libm even for double)
template <class T>
static T lse_libm(T a, T b) {
  if (a == ctcx::ninf<T>()) return b;
  if (b == ctcx::ninf<T>()) return a;
  return (a > b) ? a + ::log1pf(::expf(b - a)) : b + ::log1pf(::expf(a - b));
}
struct P32 { uint32_t a, b; };
struct P64 { uint64_t a, b; };
struct FLseF {
  typedef P32 I;
  typedef uint32_t O;
  static const char* name() { return "lse_f32"; }
  static bool dom(I) { return true; }
  static void show_in(I p, char* s) { sprintf(s, "(%a, %a)", gm::u2f(p.a), gm::u2f(p.b)); }
  static void show_out(O u, char* s) { sprintf(s, "%a", gm::u2f(u)); }
  __device__ static O dev(I p, uint64_t* etab) {
    return canon(ctcx::lse<float>(gm::u2f(p.a), gm::u2f(p.b), (CTCX_LDS uint64_t*)etab));
  }
  static O host(I p) { return canon(ctcx::lse<float>(gm::u2f(p.a), gm::u2f(p.b), (const uint64_t*)g_tab)); }
  static O libm(I p) { return canon(lse_libm<float>(gm::u2f(p.a), gm::u2f(p.b))); }
  static void census(I p, O r, uint64_t* c) {
    cls(r, c);
    const float a = gm::u2f(p.a), b = gm::u2f(p.b), ni = -__builtin_inff();
    if (a == ni || b == ni) { c[4]++; return; }
    const uint32_t e = gm::f2u(::expf(a > b ? b - a : a - b)) & 0x7fffffffu;
    c[5] += e != 0 && e < 0x00800000u;
    c[6] += e == 0;
    c[7] += a == b;
  }
  static const char* const* extra(int& n) {
    static const char* const k[] = {"in_neginf", "expf_subnormal", "expf_zero", "in_equal"};
    n = 4;
    return k;
  }
};
struct FLseD {
  typedef P64 I;
  typedef uint64_t O;
  static const char* name() { return "lse_f64"; }
  static bool dom(I) { return true; }
  static void show_in(I p, char* s) { sprintf(s, "(%a, %a)", gm::u2d(p.a), gm::u2d(p.b)); }
  static void show_out(O u, char* s) { sprintf(s, "%a", gm::u2d(u)); }
  __device__ static O dev(I p, uint64_t* etab) {
    return canon(ctcx::lse<double>(gm::u2d(p.a), gm::u2d(p.b), (CTCX_LDS uint64_t*)etab));
  }
  static O host(I p) { return canon(ctcx::lse<double>(gm::u2d(p.a), gm::u2d(p.b), (const uint64_t*)g_tab)); }
  static O libm(I p) { return canon(lse_libm<double>(gm::u2d(p.a), gm::u2d(p.b))); }
  static void census(I p, O r, uint64_t* c) {
    cls(r, c);
    const double a = gm::u2d(p.a), b = gm::u2d(p.b), ni = -__builtin_inf();
    if (a == ni || b == ni) { c[4]++; return; }
    const uint32_t e = gm::f2u(::expf(a > b ? b - a : a - b)) & 0x7fffffffu;
    c[5] += e != 0 && e < 0x00800000u;
    c[6] += e == 0;
    c[7] += a == b;
  }
  static const char* const* extra(int& n) { return FLseF::extra(n); }
};

// the widenings: (c) is plain C++, and so is (b) (the functions are __device__ only)
static uint32_t widen_f16_host(uint32_t h) { return gm::f2u((float)__builtin_bit_cast(_Float16, (uint16_t)h)); }
struct FW {
  typedef uint32_t I;
  static bool dom(I) { return true; }
  static void show_in(I u, char* s) { sprintf(s, "0x%08x", u); }
  static const char* const* extra(int& n) {
    static const char* const k[] = {"in_subnormal"};
    n = 1;
    return k;
  }
};
struct FW1 : FW {
  typedef uint32_t O;
  static void show_out(O u, char* s) { sprintf(s, "%a", gm::u2f(u)); }
};
struct FW2 : FW {
  typedef uint64_t O;   // lo | hi << 32
  static void show_out(O u, char* s) { sprintf(s, "(%a, %a)", gm::u2f((uint32_t)u), gm::u2f((uint32_t)(u >> 32))); }
};
static bool f16_sub(uint32_t h) { return (h & 0x7c00u) == 0 && (h & 0x3ffu) != 0; }
static bool bf16_sub(uint32_t h) { return (h & 0x7f80u) == 0 && (h & 0x7fu) != 0; }
struct FWidenF16 : FW1 {
  static const char* name() { return "widen_f16"; }
  __device__ static O dev(I u, uint64_t*) { return canon(ctcx::widen_f16(u)); }
  static O libm(I u) { return canon(gm::u2f(widen_f16_host(u))); }
  static O host(I u) { return libm(u); }
  static void census(I u, O r, uint64_t* c) { cls(r, c); c[4] += f16_sub(u); }
};
struct FWidenBF16 : FW1 {
  static const char* name() { return "widen_bf16"; }
  __device__ static O dev(I u, uint64_t*) { return canon(ctcx::widen_bf16(u)); }
  static O libm(I u) { return canon(gm::u2f(u << 16)); }
  static O host(I u) { return libm(u); }
  static void census(I u, O r, uint64_t* c) { cls(r, c); c[4] += bf16_sub(u); }
};
struct FWiden2F16 : FW2 {
  static const char* name() { return "widen2_f16"; }
  __device__ static O dev(I u, uint64_t*) {
    unsigned lo, hi;
    ctcx::widen2<ctcx::F16>(u, lo, hi);
    return canon(gm::u2f(lo)) | (uint64_t)canon(gm::u2f(hi)) << 32;
  }
  static O libm(I u) {
    return canon(gm::u2f(widen_f16_host(u & 0xffffu))) | (uint64_t)canon(gm::u2f(widen_f16_host(u >> 16))) << 32;
  }
  static O host(I u) { return libm(u); }
  static void census(I u, O r, uint64_t* c) {
    cls((uint32_t)r, c);
    cls((uint32_t)(r >> 32), c);
    c[4] += f16_sub(u & 0xffffu) + f16_sub(u >> 16);
  }
};
struct FWiden2BF16 : FW2 {
  static const char* name() { return "widen2_bf16"; }
  __device__ static O dev(I u, uint64_t*) {
    unsigned lo, hi;
    ctcx::widen2<ctcx::BF16>(u, lo, hi);
    return canon(gm::u2f(lo)) | (uint64_t)canon(gm::u2f(hi)) << 32;
  }
  static O libm(I u) { return canon(gm::u2f(u << 16)) | (uint64_t)canon(gm::u2f(u & 0xffff0000u)) << 32; }
  static O host(I u) { return libm(u); }
  static void census(I u, O r, uint64_t* c) {
    cls((uint32_t)r, c);
    cls((uint32_t)(r >> 32), c);
    c[4] += bf16_sub(u & 0xffffu) + bf16_sub(u >> 16);
  }
};

// one input per thread; expf's table in LDS exactly as the kernels stage it
template <class F>
__global__ __launch_bounds__(256) void unit_kernel(const typename F::I* __restrict__ in,
                                                   typename F::O* __restrict__ out, size_t n) {
  __shared__ uint64_t etab[32];
  const int tid = threadIdx.x;
  if (tid < 32) etab[tid] = gm::exp2f_tab(tid);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + tid;
  if (i < n) out[i] = F::dev(in[i], etab);
}

// ---- input sets ---------------------------------------------------------------
// item i of a set, for i in [i0, i0 + cnt), into dst
template <class I>
struct Set {
  uint64_t n = 0;
  std::function<void(uint64_t, uint64_t, I*)> gen;
};

// consecutive or strided bit patterns
struct Seg { uint64_t start, count, stride; };
template <class I>
static Set<I> seg_set(const std::vector<Seg>& segs) {
  Set<I> s;
  for (const Seg& g : segs) s.n += g.count;
  s.gen = [segs](uint64_t i0, uint64_t cnt, I* dst) {
    uint64_t base = 0;
    for (const Seg& g : segs) {
      if (cnt == 0) break;
      if (i0 < base + g.count) {
        const uint64_t k0 = i0 - base, k1 = std::min(g.count, k0 + cnt);
        for (uint64_t k = k0; k < k1; ++k) *dst++ = (I)(g.start + k * g.stride);
        cnt -= k1 - k0;
        i0 += k1 - k0;
      }
      base += g.count;
    }
  };
  return s;
}
template <class I>
static Set<I> vec_set(std::vector<I>&& v) {
  Set<I> s;
  s.n = v.size();
  auto p = std::make_shared<std::vector<I>>(std::move(v));
  s.gen = [p](uint64_t i0, uint64_t cnt, I* dst) { memcpy(dst, p->data() + i0, cnt * sizeof(I)); };
  return s;
}
static Seg around(uint64_t u, uint64_t w) { return Seg{u - w, 2 * w + 1, 1}; }
static Seg span(uint64_t lo, uint64_t hi) { return Seg{lo, hi - lo + 1, 1}; }   // patterns lo..hi

constexpr uint32_t kUnderBits = 0xc2cff1b4u;   // kExpfUnder
constexpr uint32_t kLnMinNormBits = 0xc2aeac50u;   // the first float below log(2^-126): expf's result is subnormal from here down

// the float functions' common set
static std::vector<Seg> float_segs() {
  std::vector<Seg> s;
  s.push_back(Seg{0, ((1ull << 32) + 96) / 97, 97});   // every 97th pattern
  s.push_back(span(kLnMinNormBits - 64, kUnderBits + 64));   // expf's subnormal-result band
  s.push_back(span(0x00000000u, 0x007fffffu));   // +0 and the positive subnormals
  s.push_back(span(0x80000000u, 0x807fffffu));   // -0 and the negative subnormals
  const uint32_t consts[] = {
      0x42b00000u, 0xc2b00000u, 0x42b17217u,                       // expf: +-88, 0x1.62e42ep6
      0x3ed413d7u, 0xbe95f61fu, 0x31000000u, 0xb1000000u,          // log1pf: sqrt2 - 1, sqrt(1/2) - 1, +-2^-29,
      0x24800000u, 0xa4800000u, 0xbf800000u, 0x5a000000u,          //   +-2^-54, -1, 2^53
      0x3f800000u, 0x3f330000u};                                   // logf: 1, the table's origin
  for (uint32_t c : consts) s.push_back(around(c, 4096));
  // log1pf's mantissa split 0x3504f7 of u: u = x at 2^54, 2^73 and 2^127; u = 1 + x at 2^1, 2^2, 2^5 and 2^20
  for (uint32_t e : {181u, 200u, 254u}) s.push_back(around(e << 23 | 0x3504f7u, 4096));
  for (uint32_t e : {128u, 129u, 132u, 147u}) s.push_back(around(gm::f2u(gm::u2f(e << 23 | 0x3504f7u) - 1.0f), 4096));
  return s;
}

// tools/check_glibc_math_f64.cpp's ten domains as 16 threads draw them (sample k
// from generator k % 16), and the bands around the branch constants
static std::vector<uint64_t> f64_inputs(int fn) {
  constexpr uint64_t n = 2000000;
  constexpr int W = 16;
  const int doms[2][5] = {{0, 1, 2, 3, 4}, {5, 6, 7, 8, 9}};
  std::vector<Seg> bands;
  if (fn == 0) {
    const double c[] = {-0x1.74910d52d3051p9, -1022.0 * 0x1.62e42fefa39efp-1, 512.0, -512.0, 1024.0, -1024.0};
    for (double d : c) bands.push_back(around(gm::d2u(d), 4096));
  } else {
    bands.push_back(around(0x3fee000000000000ull, 4096));                       // the near-1 range's two ends
    bands.push_back(around(0x3fee000000000000ull + 0x308ffffffffffull, 4096));
    bands.push_back(span(0x8000000000000000ull, 0x8000000000001000ull));        // -0 and negative subnormals
    bands.push_back(around(0xbff0000000000000ull, 4096));                       // negative: (x - x) / (x - x)
    bands.push_back(around(0xfff0000000000000ull, 4096));                       // ... and around -inf
  }
  uint64_t nb = 0;
  for (const Seg& g : bands) nb += g.count;
  std::vector<uint64_t> v(5 * n + nb);
  std::vector<std::thread> th;
  for (int w = 0; w < W; ++w)
    th.emplace_back([&, w]() {
      for (int q = 0; q < 5; ++q) {
        const int di = doms[fn][q];
        std::mt19937_64 g(1234567 + 7919 * di + w);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (uint64_t k = w; k < n; k += W) {
          double x;
          switch (di) {
            case 0: x = -50.0 * u01(g); break;
            case 1: x = -750.0 * u01(g); break;
            case 2: x = (u01(g) * 2 - 1) * 0x1p-50; break;
            case 3: x = (u01(g) * 2 - 1) * 1100.0; break;
            case 4: x = gm::u2d(g()); break;
            case 5: x = 1.0 + 8191.0 * u01(g); break;
            case 6: x = 1.0 + (u01(g) * 2 - 1) * 0x1.2p-4; break;
            case 7: x = gm::u2d(g() & 0x000fffffffffffffull); break;
            case 8: x = gm::u2d(g() & 0x7fffffffffffffffull); break;
            default: x = u01(g); break;
          }
          v[q * n + k] = gm::d2u(x);
        }
      }
    });
  for (auto& t : th) t.join();
  seg_set<uint64_t>(bands).gen(0, nb, v.data() + 5 * n);
  return v;
}

// lse: d = every 41st pattern of [kExpfUnder - 1, 0], b = a + d with a cycling
// by index, both argument orders; then the special pairs, both orders
template <class T, class I, class B>
static Set<I> lse_set(const std::vector<T>& as, B bits) {
  const uint32_t dlast = gm::f2u(gm::kExpfUnder - 1.0f);
  const uint64_t nd = (dlast - 0x80000000u) / 41 + 1;
  const T inf = ctcx::pinf<T>(), nan = (T)__builtin_nanf(""), big = std::numeric_limits<T>::max();
  const T sp[][2] = {{-inf, -inf}, {-inf, (T)-1.5}, {-inf, (T)0}, {-inf, inf}, {-inf, nan},
                     {(T)-2.25, (T)-2.25}, {(T)0, (T)0}, {(T)0, -(T)0}, {big, big}, {-big, -big},
                     {nan, (T)-1}, {nan, nan}, {nan, inf},
                     {inf, (T)0}, {inf, inf}, {inf, big},
                     {big, -big}, {(T)1e38f, (T)-3e38f},                         // the difference overflows
                     {(T)0, (T)-87.5}, {(T)0, (T)-95}, {(T)0, (T)-100}, {(T)0, (T)-103.25},   // total 0, subnormal expf
                     {-(T)0, (T)-103.9}, {(T)0, (T)gm::kExpfUnder}, {(T)0, (T)-104}};
  std::vector<std::pair<T, T>> spv;
  for (const auto& p : sp) spv.emplace_back(p[0], p[1]);
  Set<I> s;
  s.n = 2 * (nd + spv.size());
  s.gen = [as, spv, nd, bits](uint64_t i0, uint64_t cnt, I* dst) {
    for (uint64_t i = i0; i < i0 + cnt; ++i) {
      const uint64_t p = i >> 1;
      T a, b;
      if (p < nd) {
        a = as[p % as.size()];
        b = a + (T)gm::u2f((uint32_t)(0x80000000u + 41 * p));
      } else {
        a = spv[p - nd].first;
        b = spv[p - nd].second;
      }
      *dst++ = (i & 1) ? I{bits(b), bits(a)} : I{bits(a), bits(b)};
    }
  };
  return s;
}

// ---- the run -------------------------------------------------------------------
struct Totals { uint64_t inputs = 0, bad = 0; };
// a chunk's inputs and its three sets of results on the host, inputs and results
// on the device: 64 MB each, allocated once
constexpr uint64_t kChunkBytes = 64ull << 20;
static void *g_buf[4], *g_dbuf[2];

// fn(thread, k0, k1) over [0, n) in blocks of 4096, dealt to the threads in turn
template <class Fn>
static void par(uint64_t n, Fn fn) {
  std::vector<std::thread> th;
  for (int w = 0; w < g_nthr; ++w)
    th.emplace_back([=]() {
      for (uint64_t k0 = (uint64_t)w * 4096; k0 < n; k0 += (uint64_t)g_nthr * 4096) fn(w, k0, std::min(n, k0 + 4096));
    });
  for (auto& t : th) t.join();
}

template <class F>
static void run(const Set<typename F::I>& set, Totals& tot) {
  typedef typename F::I I;
  typedef typename F::O O;
  const uint64_t CH = kChunkBytes / (sizeof(I) > sizeof(O) ? sizeof(I) : sizeof(O));   // raw items per chunk
  I* const in = (I*)g_buf[0];
  O *const od = (O*)g_buf[1], *const oh = (O*)g_buf[2], *const ol = (O*)g_buf[3];
  I* const din = (I*)g_dbuf[0];
  O* const dout = (O*)g_dbuf[1];
  struct Acc {
    uint64_t c[kMaxCensus] = {0}, dh = 0, dl = 0, hl = 0;
    uint64_t first[4];   // a few mismatching inputs, to print
    int nfirst = 0;
  };
  Acc sum;
  uint64_t inputs = 0;
  int shown = 0;
  for (uint64_t i0 = 0; i0 < set.n; i0 += CH) {
    const uint64_t raw = std::min(CH, set.n - i0);
    par(raw, [&](int, uint64_t k0, uint64_t k1) { set.gen(i0 + k0, k1 - k0, in + k0); });
    uint64_t m = 0;
    for (uint64_t k = 0; k < raw; ++k)
      if (F::dom(in[k])) in[m++] = in[k];
    if (m == 0) continue;
    if (!g_host_only) {
      HIP_OK(hipMemcpy(din, in, m * sizeof(I), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(unit_kernel<F>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, din, dout, (size_t)m);
      HIP_OK(hipGetLastError());
    }
    // (b) and (c) on the host while the kernel runs
    par(m, [&](int, uint64_t k0, uint64_t k1) {
      for (uint64_t k = k0; k < k1; ++k) {
        oh[k] = F::host(in[k]);
        ol[k] = F::libm(in[k]);
      }
    });
    if (!g_host_only) {
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipMemcpy(od, dout, m * sizeof(O), hipMemcpyDeviceToHost));
    }
    std::vector<Acc> acc(g_nthr);
    par(m, [&](int w, uint64_t k0, uint64_t k1) {
      Acc& a = acc[w];
      for (uint64_t k = k0; k < k1; ++k) {
        F::census(in[k], ol[k], a.c);
        bool bad = oh[k] != ol[k];
        a.hl += bad;
        if (!g_host_only) {
          a.dh += od[k] != oh[k];
          a.dl += od[k] != ol[k];
          bad |= od[k] != oh[k];
        }
        if (bad && a.nfirst < 4) a.first[a.nfirst++] = k;
      }
    });
    for (int w = 0; w < g_nthr; ++w) {
      const Acc& a = acc[w];
      for (int q = 0; q < kMaxCensus; ++q) sum.c[q] += a.c[q];
      sum.dh += a.dh;
      sum.dl += a.dl;
      sum.hl += a.hl;
      for (int q = 0; q < a.nfirst && shown < 4; ++q, ++shown) {
        const uint64_t k = a.first[q];
        char si[96], sd[96], sh[96], sl[96];
        F::show_in(in[k], si);
        F::show_out(oh[k], sh);
        F::show_out(ol[k], sl);
        if (g_host_only) strcpy(sd, "-");
        else F::show_out(od[k], sd);
        printf("  %s %s: device %s host %s libm %s\n", F::name(), si, sd, sh, sl);
      }
    }
    inputs += m;
  }
  printf("%s inputs=%llu", F::name(), (unsigned long long)inputs);
  for (int q = 0; q < 4; ++q) printf(" %s=%llu", kCls[q], (unsigned long long)sum.c[q]);
  int ne;
  const char* const* en = F::extra(ne);
  for (int q = 0; q < ne; ++q) printf(" %s=%llu", en[q], (unsigned long long)sum.c[4 + q]);
  if (g_host_only) printf(" device_vs_host=- device_vs_libm=-");
  else printf(" device_vs_host=%llu device_vs_libm=%llu", (unsigned long long)sum.dh, (unsigned long long)sum.dl);
  printf(" host_vs_libm=%llu\n", (unsigned long long)sum.hl);
  fflush(stdout);
  tot.inputs += inputs;
  tot.bad += sum.dh + sum.dl + sum.hl;
}

int main(int argc, char** argv) {
  const bool all = argc > 1 && !strcmp(argv[1], "all");
  g_host_only = argc > 1 && !strcmp(argv[1], "host");
  if (argc > 1 && !all && !g_host_only) {
    printf("usage: %s [host | all]\n", argv[0]);
    return 2;
  }
  g_nthr = (int)std::thread::hardware_concurrency();
  g_nthr = g_nthr > 16 ? 16 : g_nthr < 1 ? 1 : g_nthr;
  for (int i = 0; i < 32; ++i) g_tab[i] = gm::exp2f_tab(i);
  for (auto& b : g_buf)
    if (!(b = malloc(kChunkBytes))) return 2;
  if (!g_host_only)
    for (auto& b : g_dbuf) HIP_OK(hipMalloc(&b, kChunkBytes));
  Totals tot;
  {
    const Set<uint32_t> fs = seg_set<uint32_t>(all ? std::vector<Seg>{Seg{0, 1ull << 32, 1}} : float_segs());
    run<FExpf>(fs, tot);
    run<FLogf>(fs, tot);
    if (all) {
      run<FLog1pf>(fs, tot);
    } else {
      std::vector<Seg> s = float_segs();
      s.push_back(Seg{0, 0x3f800000u / 13 + 1, 13});   // every 13th pattern of [0, 1]: lse's whole argument range
      run<FLog1pf>(seg_set<uint32_t>(s), tot);
    }
    run<FExpfT>(fs, tot);
    run<FExpfNonpos>(fs, tot);
    run<FExpfLe0>(fs, tot);
    run<FExpfCore>(fs, tot);
  }
  if (!all) {
    run<FExp>(vec_set(f64_inputs(0)), tot);
    run<FLog>(vec_set(f64_inputs(1)), tot);
    const std::vector<float> af = {0.0f, -0.5f, -3.75f, -1e-3f, -88.5f, -1e4f, -1e30f};
    std::vector<double> ad(af.begin(), af.end());
    ad.push_back(-1e300);
    ad.push_back(-0x1.23456789abcdep1);   // more than 24 mantissa bits
    run<FLseF>(lse_set<float, P32>(af, [](float x) { return gm::f2u(x); }), tot);
    run<FLseD>(lse_set<double, P64>(ad, [](double x) { return gm::d2u(x); }), tot);
    std::vector<Seg> h = {Seg{0, 65536, 1}};
    run<FWidenF16>(seg_set<uint32_t>(h), tot);
    run<FWidenBF16>(seg_set<uint32_t>(h), tot);
    // widen2: every pattern in each half of the word, the other half scrambled
    std::vector<uint32_t> w2;
    for (uint32_t p = 0; p < 65536; ++p) w2.push_back(p | ((p * 40503u + 12345u) & 0xffffu) << 16);
    for (uint32_t p = 0; p < 65536; ++p) w2.push_back(p << 16 | ((p * 40503u + 12345u) & 0xffffu));
    run<FWiden2F16>(vec_set(std::vector<uint32_t>(w2)), tot);
    run<FWiden2BF16>(vec_set(std::move(w2)), tot);
  }
  printf("glibc_math_unit: %llu mismatches over %llu inputs\n", (unsigned long long)tot.bad,
         (unsigned long long)tot.inputs);
  return tot.bad ? 1 : 0;
}
