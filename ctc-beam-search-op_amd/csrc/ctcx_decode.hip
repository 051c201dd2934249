// ctcx_decode.hip — MI355X (gfx950) kernels for CTC beam search with per-beam
// best-alignment tracking.  Drop-in replacement for the reference CPU path
//   CTCExtBeamSearchDecoderOp<T>::Compute   (kernels/..._kernels.cc:20-95)
//   CTCExtBeamSearchDecoder<T>::Step/TopPaths (util/ctc_ext_beam_search_decoder.h:66-261)
//   BeamEntry / TopN / LogSumExp             (util/ctc_beam_entry.h, util/ctc_loss_util.h)
//
// Kernels (launch order; DESIGN.md has the roofline of each):
//   ctcx_row_norm     one wave per 64 (t, b) rows, staged through LDS in 64-class
//                     tiles (coalesced loads); one thread per row then sums in
//                     class order: softmax normaliser, glibc-exact expf sum
//                     (decoder.h:72-80).
//   ctcx_beam_decode  one wave64 workgroup per batch item, persistent over t.
//                     Beam state lives in LDS; per frame it writes one 8-byte
//                     record per surviving beam (prefix back-link + alignment
//                     backpointers) to HBM.
//   ctcx_traceback    one thread per (item, path, {decoded, alignment}): walks
//                     the records backwards (LabelSeq / AlignmentLabelSeq).
//   ctcx_scan         per (path, kind) exclusive scan of sequence lengths.
//   ctcx_pack         int64 SparseTensor components (StoreAllDecodedSequences).
//   ctcx_dense_prologue, ctcx_pack_dense   the enqueue-only path: lengths and
//                     table checked on the device, padded [B][P][Tmax] outputs.
//
// The beam update per frame has two exact implementations:
//   * the FAST path (exact_step, whole wave): beams sit at LDS slots; offers are
//     scored 64 per chunk and the accepted ones are pushed, in offer order,
//     into an LDS replica of gtl::TopN's libstdc++ heap (wave-parallel sift:
//     one ballot finds the path, a second the stop), so evictions and the
//     sort_heap Extract order of tied totals are the reference's.
//   * the LITERAL path (literal_step, one lane): the reference's TopN state
//     machine verbatim over slot ids (ctcx_topn.h), for the frames the fast
//     path does not model: a non-finite logit or total, the beam filling up in
//     the middle of the grow loop (TopN then peeks lazily), and a beam that
//     holds one entry twice (reachable with -inf logits, decoder.h:142 +
//     189-199).  Such a frame is replayed from the untouched frame-start state.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#ifdef CTCX_STREAM
#include <stddef.h>
#include <string.h>
#endif

#include <type_traits>
#include <utility>

#include "ctcx_kernels.h"
#include "ctcx_topn.h"
#include "ctcx_regsort.h"
#include "glibc_math.h"
#include "glibc_math_f64.h"

namespace ctcx {

// branch / entry flag bits
constexpr int F_ROOT = 1;    // this node is the root (empty prefix)
constexpr int F_PROOT = 2;   // this node's parent is the root
constexpr int F_HB = 4;      // has a blank-ending alignment candidate
constexpr int F_HN = 8;      // has a label-ending alignment candidate
// per-frame branch state bits
constexpr int S_EVICT = 1;   // pushed this frame, then evicted from the beam
constexpr int S_DEACT = 2;   // deactivated (oldp reset): grows no children
constexpr int kDeactRec = 1 << 30;   // exact_step chunk record: deactivation (else eviction)

template <typename T> __host__ __device__ __forceinline__ T ninf();
template <> __host__ __device__ __forceinline__ float ninf<float>() { return -__builtin_inff(); }
template <> __host__ __device__ __forceinline__ double ninf<double>() { return -__builtin_inf(); }
template <typename T> __host__ __device__ __forceinline__ T pinf();
template <> __host__ __device__ __forceinline__ float pinf<float>() { return __builtin_inff(); }
template <> __host__ __device__ __forceinline__ double pinf<double>() { return __builtin_inf(); }

// util/ctc_loss_util.h:29-41 — float libm (expf, log1pf) even for T=double.
// etab: expf's 2^(i/32) table (a copy in LDS: lanes that run the recursion
// in parallel take divergent table indices, and the switch form would branch
// once per case)
template <typename T, class P>
__host__ __device__ __forceinline__ T lse(T a, T b, P etab) {
  if (a == ninf<T>()) return b;
  if (b == ninf<T>()) return a;
  return (a > b) ? a + (T)gm::log1pf(gm::expf_t((float)(b - a), etab))
                 : b + (T)gm::log1pf(gm::expf_t((float)(a - b), etab));
}

__device__ __forceinline__ float bcast(float v, int k) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}
__device__ __forceinline__ double bcast(double v, int k) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int bcast(int v, int k) { return __builtin_amdgcn_readlane(v, k); }

// Wave-uniform values that come out of LDS or VALU: readfirstlane moves them to
// SGPRs so the loops and branches they control stay scalar (no exec masking).
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double uni(double v) { return bcast(v, 0); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)(uint32_t)uni((int)(v >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)v);
}

template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = (w < v) ? w : v;
  }
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = (w > v) ? w : v;
  }
  return v;
}

// Wave reductions without LDS traffic (for NaN-free data; the order of the
// comparisons differs from wave_max's): a prefix max/min/sum inside each row
// of 16 lanes by DPP row shifts, then the four row results by readlane.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v, float ident) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, ident),
                                                               __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v, int ident) {
  return __builtin_amdgcn_update_dpp(ident, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  const float I = -__builtin_inff();
  float w;
  w = dpp_f<0x111>(v, I); v = w > v ? w : v;   // row_shr:1
  w = dpp_f<0x112>(v, I); v = w > v ? w : v;   // row_shr:2
  w = dpp_f<0x114>(v, I); v = w > v ? w : v;   // row_shr:4
  w = dpp_f<0x118>(v, I); v = w > v ? w : v;   // row_shr:8
  const float a = bcast(v, 15), b = bcast(v, 31), c = bcast(v, 47), d = bcast(v, 63);
  const float ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}
__device__ __forceinline__ double wave_max_dpp(double v) { return wave_max(v); }
// The maximum over each 16-lane DPP row, landing on the row's lane 15, by
// v_max_f32_dpp (row_shr 1, 2, 4, 8; a lane without a source keeps its own
// value); v must not be NaN.  As asm: the compiler's form moves the shifted
// value, canonicalizes it and then takes the max (four instructions a step).
// s_nop 1: a VGPR written by a VALU is read by a DPP two states later.
__device__ __forceinline__ float row16_fmax_dpp(float v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf"
      : "+v"(v));
  return v;
}
// the same by v_max_f32 (IEEE maxNum: a NaN operand loses; of +0 and -0
// either may come back) -- for maxima whose zero sign nothing reads (the row
// facts' maxima: compared, or subtracted from values as a softmax maximum)
__device__ __forceinline__ float wave_fmax_dpp(float v) {
  const float I = -__builtin_inff();
  v = __builtin_fmaxf(v, dpp_f<0x111>(v, I));   // row_shr:1
  v = __builtin_fmaxf(v, dpp_f<0x112>(v, I));   // row_shr:2
  v = __builtin_fmaxf(v, dpp_f<0x114>(v, I));   // row_shr:4
  v = __builtin_fmaxf(v, dpp_f<0x118>(v, I));   // row_shr:8
  const float a = bcast(v, 15), b = bcast(v, 31), c = bcast(v, 47), d = bcast(v, 63);
  return __builtin_fmaxf(__builtin_fmaxf(a, b), __builtin_fmaxf(c, d));
}
__device__ __forceinline__ unsigned wave_min_dpp(unsigned v) {
  const int I = -1;   // 0xffffffff
  int x = (int)v, w;
  w = dpp_i<0x111>(x, I); x = (unsigned)w < (unsigned)x ? w : x;
  w = dpp_i<0x112>(x, I); x = (unsigned)w < (unsigned)x ? w : x;
  w = dpp_i<0x114>(x, I); x = (unsigned)w < (unsigned)x ? w : x;
  w = dpp_i<0x118>(x, I); x = (unsigned)w < (unsigned)x ? w : x;
  const unsigned a = (unsigned)bcast(x, 15), b = (unsigned)bcast(x, 31), c = (unsigned)bcast(x, 47),
                 d = (unsigned)bcast(x, 63);
  const unsigned ab = a < b ? a : b, cd = c < d ? c : d;
  return ab < cd ? ab : cd;
}
__device__ __forceinline__ int wave_sum_dpp(int x) {
  x += dpp_i<0x111>(x, 0);
  x += dpp_i<0x112>(x, 0);
  x += dpp_i<0x114>(x, 0);
  x += dpp_i<0x118>(x, 0);
  return bcast(x, 15) + bcast(x, 31) + bcast(x, 47) + bcast(x, 63);
}

// "first-pushed maximum" of a std::priority_queue with a strict '<' comparer
// (ctc_beam_entry.h:65-73): only a strictly greater push replaces the top.
template <typename T>
struct Best {
  T p;
  uint32_t bp;
  bool ok;
  __host__ __device__ __forceinline__ void push(T prob, uint32_t b) {
    if (!ok || prob > p) { p = prob; bp = b; ok = true; }
  }
};

// One TopN element: the entry's total travels with its slot id.
template <typename T> struct HE;
template <> struct __attribute__((aligned(8))) HE<float> { float v; int s; };
template <> struct __attribute__((aligned(16))) HE<double> { double v; int s; int pad; };

typedef unsigned u32x2 __attribute__((ext_vector_type(2), may_alias));
typedef unsigned u32x4 __attribute__((ext_vector_type(4), may_alias));

// Half-precision inputs (DecodeParams::xfmt): 2-byte elements in memory,
// widened to float where a kernel reads them -- exact for both formats, so
// everything downstream sees the values of the widened float tensor.
//   fp16: the hardware convert (v_cvt_f32_f16; f16 denormals are never
//         flushed, subnormals widen to their exact float value)
//   bf16: the bits, 16 to the left
struct F16 { uint16_t u; };
struct BF16 { uint16_t u; };
__device__ __forceinline__ float widen_f16(unsigned h) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}
__device__ __forceinline__ float widen_bf16(unsigned h) { return __uint_as_float(h << 16); }
// element j of a row of E, as T (E = T: the element itself)
template <typename T, typename E>
__device__ __forceinline__ T ldw(const E* p, int64_t j) {
  if constexpr (std::is_same<E, F16>::value) return widen_f16(p[j].u);
  else if constexpr (std::is_same<E, BF16>::value) return widen_bf16(p[j].u);
  else return p[j];
}
// a 32-bit word holding halves 2i (low) and 2i + 1 (high), as two floats' bits
template <typename E>
__device__ __forceinline__ void widen2(unsigned w, unsigned& lo, unsigned& hi) {
  if constexpr (std::is_same<E, F16>::value) {
    lo = __float_as_uint(widen_f16(w & 0xffffu));
    hi = __float_as_uint(widen_f16(w >> 16));
  } else {
    lo = w << 16;
    hi = w & 0xffff0000u;
  }
}

// The decode kernel's row stage for half-precision rows: C 2-byte elements
// at xr, widened into the LDS row (C float bit patterns, 16-byte aligned).
// Rows of whole 16-byte pieces (C % 8 == 0, xr 16-byte aligned: the base and
// both byte strides are then multiples of 16) move as 8 halves per load, a
// batch of loads in flight per thread before the first LDS write; any other
// row (an odd C leaves every other row start 2-byte aligned) element by element.
// NT threads (the block) share the row.
template <typename E>
__device__ __forceinline__ void stage_row_half_t(CTCX_LDS unsigned* row, const uint16_t* xr, int C, int tid,
                                                 int NT) {
  if ((C & 7) == 0 && ((((uintptr_t)xr) | (uintptr_t)row) & 15) == 0) {
    const u32x4* x8 = (const u32x4*)xr;
    CTCX_LDS u32x4* r4 = (CTCX_LDS u32x4*)row;
    const int C8 = C >> 3;
    constexpr int kRB = 4;
    for (int q0 = 0; q0 < C8; q0 += kRB * NT) {
      u32x4 v[kRB];
#pragma unroll
      for (int u = 0; u < kRB; ++u) {
        const int q = q0 + u * NT + tid;
        if (q < C8) v[u] = x8[q];
      }
#pragma unroll
      for (int u = 0; u < kRB; ++u) {
        const int q = q0 + u * NT + tid;
        if (q < C8) {
          u32x4 a, b;
          unsigned l, h;
          widen2<E>(v[u][0], l, h); a[0] = l; a[1] = h;
          widen2<E>(v[u][1], l, h); a[2] = l; a[3] = h;
          widen2<E>(v[u][2], l, h); b[0] = l; b[1] = h;
          widen2<E>(v[u][3], l, h); b[2] = l; b[3] = h;
          r4[2 * q] = a;
          r4[2 * q + 1] = b;
        }
      }
    }
  } else {
    for (int j = tid; j < C; j += NT) row[j] = __float_as_uint(ldw<float>((const E*)xr, j));
  }
}
// One out-of-line function for every decode kernel, as literal_step is: the
// kernels' float path keeps its code (a uniform branch and a call are all the
// frame loop gains), and the instantiations do not each carry a copy.
__device__ __attribute__((noinline)) void stage_row_half(CTCX_LDS unsigned* row, const uint16_t* xr, int C,
                                                         bool f16, int tid, int NT) {
  if (f16) stage_row_half_t<F16>(row, xr, C, tid, NT);
  else stage_row_half_t<BF16>(row, xr, C, tid, NT);
}

// Heap element loads/stores as single 8-byte (float) / 16-byte (double) LDS
// accesses; a pair of siblings is one 16-byte (two for double) access.
// (vector elements are copied to scalars before __builtin_bit_cast: clang
// bit-casts an ext-vector element lvalue from element 0's bits)
__host__ __device__ __forceinline__ HE<float> he_ld(const CTCX_LDS HE<float>* he, int i) {
  const u32x2 q = *(const CTCX_LDS u32x2*)(he + i);
  const unsigned x = q.x, y = q.y;
  return HE<float>{__builtin_bit_cast(float, x), (int)y};
}
__host__ __device__ __forceinline__ void he_st(CTCX_LDS HE<float>* he, int i, HE<float> e) {
  u32x2 q;
  q.x = __builtin_bit_cast(unsigned, e.v);
  q.y = (unsigned)e.s;
  *(CTCX_LDS u32x2*)(he + i) = q;
}
__host__ __device__ __forceinline__ void he_ld2(const CTCX_LDS HE<float>* he, int i, HE<float>& a, HE<float>& b) {
  const u32x4 q = *(const CTCX_LDS u32x4*)(he + i);   // i even: 16-byte aligned
  const unsigned x = q.x, y = q.y, z = q.z, w = q.w;
  a = HE<float>{__builtin_bit_cast(float, x), (int)y};
  b = HE<float>{__builtin_bit_cast(float, z), (int)w};
}
__device__ __forceinline__ HE<double> he_ld(const CTCX_LDS HE<double>* he, int i) {
  const u32x4 q = *(const CTCX_LDS u32x4*)(he + i);
  const unsigned x = q.x, y = q.y, z = q.z;
  return HE<double>{__builtin_bit_cast(double, ((uint64_t)y << 32) | x), (int)z, 0};
}
__device__ __forceinline__ void he_st(CTCX_LDS HE<double>* he, int i, HE<double> e) {
  const uint64_t u = __builtin_bit_cast(uint64_t, e.v);
  u32x4 q;
  q.x = (unsigned)u; q.y = (unsigned)(u >> 32); q.z = (unsigned)e.s; q.w = 0;
  *(CTCX_LDS u32x4*)(he + i) = q;
}
__device__ __forceinline__ void he_ld2(const CTCX_LDS HE<double>* he, int i, HE<double>& a, HE<double>& b) {
  a = he_ld(he, i);
  b = he_ld(he, i + 1);
}

template <typename T>
struct Ctx {
  // branch arrays, double-buffered by frame parity: [buf][i]
  CTCX_LDS T* ot[2]; CTCX_LDS T* ob[2]; CTCX_LDS T* ol[2]; CTCX_LDS T* cb[2]; CTCX_LDS T* cn[2];
  CTCX_LDS int* lab[2]; CTCX_LDS int* par[2]; CTCX_LDS int* flg[2];
  CTCX_LDS int* head; CTCX_LDS int* sib; CTCX_LDS int* bst; CTCX_LDS int* newpos;
  // entries (fast: beam slots; literal: node slots), capacity enc = 3W+2
  CTCX_LDS T* et; CTCX_LDS T* eb; CTCX_LDS T* el; CTCX_LDS T* ecb; CTCX_LDS T* ecn;
  CTCX_LDS uint32_t* ebpb; CTCX_LDS uint32_t* ebpn; CTCX_LDS uint32_t* ekind;
  CTCX_LDS int* elab; CTCX_LDS int* eflg;
  CTCX_LDS int* heap; CTCX_LDS int* tops; CTCX_LDS int* freel; CTCX_LDS int* sorted;
  // per branch position: the first position holding the same entry (the
  // reference's beam can hold one BeamEntry twice, see literal_step)
  CTCX_LDS int* alias;
  CTCX_LDS T* row;
  CTCX_LDS int* misc;
  // prefix identity: 128-bit hash of each branch's label prefix, [buf][i];
  // htab maps the hash of a frame's new leaves to position
  CTCX_LDS uint64_t* ha[2]; CTCX_LDS uint64_t* hb[2];
  CTCX_LDS int* htab;
  CTCX_LDS uint64_t* bloom;   // per branch: label bits (l & 63) of children evicted this frame
  CTCX_LDS HE<T>* he;  // TopN elements_, position p at he[p + 1]
  CTCX_LDS uint64_t* etab;   // expf's 2^(i/32) table (gm::exp2f_tab), for lse
  // beam-scorer state (a stateful scorer only): per branch [buf][i], per entry
  CTCX_LDS T* est[2]; CTCX_LDS T* eest;
  const T* sctab;      // the scorer's table (global memory)
  // large C: this frame's row facts from ctcx_row_prep (RowHdr)
  T rxmax, rxout;
  int rbad, rns;
  int W, C, blank, enc, hts, wcap;
  int hdum;            // he index of lane 0's dummy store slot
  int tabdead;         // HW kernels: a score-table wait gave up (never in a correct run)
#ifdef CTCX_PHASES
  uint64_t* prof;      // this item's phase counters (diagnostics build; null: off)
#endif
};
// the helper wave's phase counters (diagnostics build): lane 0 of wave 1 adds
#ifdef CTCX_PHASES
#define CTCX_HPC_(cx, i, v)                                                                             \
  do {                                                                                                  \
    if ((cx).prof && threadIdx.x == 64)                                                                 \
      __hip_atomic_fetch_add((cx).prof + (i), (uint64_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
  } while (0)
#if defined(CTCX_PHASE_TIES) || defined(CTCX_PHASE_EXTT) || defined(CTCX_PHASE_BIRTH)   // (the helper's counters carry those diagnostics only)
#define CTCX_HPC(cx, i, v) do { } while (0)
#else
#define CTCX_HPC(cx, i, v) CTCX_HPC_(cx, i, v)
#endif
#define CTCX_HTIME() __builtin_amdgcn_s_memtime()
#else
#define CTCX_HPC(cx, i, v) do { } while (0)
#define CTCX_HTIME() 0ull
#endif

// Per-64-label block maxima of the logit row, right after the row (large C).
template <typename T>
__host__ __device__ __forceinline__ CTCX_LDS T* row_bmax(const Ctx<T>& cx) {
  return (CTCX_LDS T*)((CTCX_LDS char*)cx.row + (((size_t)cx.C * sizeof(T) + 15) & ~(size_t)15));
}
// Large C, after the block maxima: the compacted chunk's offers (64 x (branch
// << 16 | label index)), then the label-index bitmap of the children of one
// branch (bit x of word x >> 6) and its per-window summary (bit a of word
// a >> 6: window a holds a child).  Layout as in decode_lds_bytes.
template <typename T>
__host__ __device__ __forceinline__ CTCX_LDS uint32_t* row_cq(const Ctx<T>& cx) {
  const size_t nblk = (size_t)(cx.C + 63) / 64;
  return (CTCX_LDS uint32_t*)((CTCX_LDS char*)row_bmax(cx) + ((nblk * sizeof(T) + 15) & ~(size_t)15));
}
template <typename T>
__host__ __device__ __forceinline__ CTCX_LDS uint64_t* row_cbm(const Ctx<T>& cx) {
  return (CTCX_LDS uint64_t*)(row_cq(cx) + 64);
}
// ... then the row's top set (float rows): values, label indices, kTopK each
template <typename T>
__host__ __device__ __forceinline__ CTCX_LDS float* row_topx(const Ctx<T>& cx) {
  const int nw = (cx.C - 1 + 63) / 64;
  return (CTCX_LDS float*)(row_cbm(cx) + nw + (nw + 63) / 64);
}

// Frame-parity buffer select without indexing the pointer pair, so Ctx stays
// in registers (a runtime index into a member array would force it to scratch).
template <typename P>
__host__ __device__ __forceinline__ P sel(P const (&a)[2], int b) { return b ? a[1] : a[0]; }

// Prefix hashing (stands in for the reference's trie, ctc_beam_entry.h:114-122
// and 248-269): a node's identity is its label prefix; h(prefix + [l]) =
// mix(h(prefix), l), two independent 64-bit chains.  For a fixed label each
// chain step is a bijection, so siblings and same-label children of distinct
// parents never collide; an accidental collision needs 2^-128 luck.
__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
__host__ __device__ __forceinline__ void hmix(uint64_t a, uint64_t b, int l, uint64_t& oa, uint64_t& ob) {
  const uint64_t x = (uint64_t)(uint32_t)l + 1ull;
  oa = fmix64(a ^ (x * 0x9E3779B97F4A7C15ull));
  ob = fmix64(b + x * 0xD6E8FEB86659FD93ull + 0x632BE59BD9B4E019ull);
}
constexpr uint64_t kRootHa = 0x243F6A8885A308D3ull, kRootHb = 0x13198A2E03707344ull;

// The parent's prefix hash from a node's own (hmix is invertible: fmix64 and
// both label steps are bijections), so it need not be stored per branch.
__host__ __device__ constexpr uint64_t inv_odd64(uint64_t a) {
  uint64_t x = a;                                    // correct to 3 bits (a odd)
  for (int i = 0; i < 6; ++i) x *= 2ull - a * x;     // Newton: doubles the bits
  return x;
}
__host__ __device__ __forceinline__ uint64_t fmix64_inv(uint64_t k) {
  k ^= k >> 33; k *= inv_odd64(0xc4ceb9fe1a85ec53ull);
  k ^= k >> 33; k *= inv_odd64(0xff51afd7ed558ccdull);
  k ^= k >> 33;
  return k;
}
__host__ __device__ __forceinline__ void hmix_inv(uint64_t oa, uint64_t ob, int l, uint64_t& a, uint64_t& b) {
  const uint64_t x = (uint64_t)(uint32_t)l + 1ull;
  a = fmix64_inv(oa) ^ (x * 0x9E3779B97F4A7C15ull);
  b = fmix64_inv(ob) - x * 0xD6E8FEB86659FD93ull - 0x632BE59BD9B4E019ull;
}
static_assert(inv_odd64(0xff51afd7ed558ccdull) * 0xff51afd7ed558ccdull == 1ull, "inverse");
static_assert(inv_odd64(0xc4ceb9fe1a85ec53ull) * 0xc4ceb9fe1a85ec53ull == 1ull, "inverse");

// LDS layout for a beam of up to Wcap (the kernel's compile-time capacity, or
// the runtime W for the WC = 0 instantiations).  Every array sits at an offset
// that depends on Wcap only -- the C-sized logit row comes last -- so with a
// compile-time Wcap all of them are instruction immediates instead of ~45
// pointer SGPRs.  decode_lds_bytes (ctcx_kernels.h) mirrors this sum.
template <typename T>
__host__ __device__ __forceinline__ void carve(Ctx<T>& cx, CTCX_LDS char* base, int Wcap, int W, int C, bool scored,
                                               bool inplace) {
  // inplace (large C, decode_inplace): one buffer of branch arrays, updated in
  // place by the commit.  The caller passes a compile-time value, so every
  // offset stays an immediate.
  const size_t ENC = 3 * (size_t)Wcap + 2;
  const int nbuf = inplace ? 1 : 2;
  auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  CTCX_LDS char* p = base;
  for (int b = 0; b < nbuf; ++b) {
    CTCX_LDS T* q = (CTCX_LDS T*)p;
    cx.ot[b] = q; cx.ob[b] = q + Wcap; cx.ol[b] = q + 2 * Wcap; cx.cb[b] = q + 3 * Wcap; cx.cn[b] = q + 4 * Wcap;
    p += a16(5 * (size_t)Wcap * sizeof(T));
  }
  for (int b = 0; b < nbuf; ++b) {
    CTCX_LDS int* q = (CTCX_LDS int*)p;
    cx.lab[b] = q; cx.par[b] = q + Wcap; cx.flg[b] = q + 2 * Wcap;
    p += a16(3 * (size_t)Wcap * 4);
  }
  {
    CTCX_LDS int* q = (CTCX_LDS int*)p;
    cx.head = q; cx.sib = q + Wcap; cx.bst = q + 2 * Wcap; cx.newpos = q + 3 * Wcap;
    p += a16(4 * (size_t)Wcap * 4);
  }
  {
    CTCX_LDS T* q = (CTCX_LDS T*)p;
    cx.et = q; cx.eb = q + ENC; cx.el = q + 2 * ENC; cx.ecb = q + 3 * ENC; cx.ecn = q + 4 * ENC;
    p += a16(5 * ENC * sizeof(T));
  }
  {
    CTCX_LDS uint32_t* q = (CTCX_LDS uint32_t*)p;
    cx.ebpb = q; cx.ebpn = q + ENC; cx.ekind = q + 2 * ENC;
    cx.elab = (CTCX_LDS int*)(q + 3 * ENC); cx.eflg = (CTCX_LDS int*)(q + 4 * ENC);
    p += a16(5 * ENC * 4);
  }
  cx.heap = (CTCX_LDS int*)p; p += a16(((size_t)Wcap + 1) * 4);
  cx.tops = (CTCX_LDS int*)p; p += a16(((size_t)Wcap + 1) * 4);
  cx.sorted = (CTCX_LDS int*)p; p += a16((size_t)Wcap * 4);
  cx.alias = (CTCX_LDS int*)p; p += a16((size_t)Wcap * 4);
  cx.misc = (CTCX_LDS int*)p; p += 64;
  cx.etab = (CTCX_LDS uint64_t*)p; p += 32 * 8;
  for (int b = 0; b < nbuf; ++b) {
    CTCX_LDS uint64_t* q = (CTCX_LDS uint64_t*)p;
    cx.ha[b] = q; cx.hb[b] = q + Wcap;
    p += 2 * (size_t)Wcap * 8;
  }
  cx.hts = htab_size(Wcap);
  cx.htab = (CTCX_LDS int*)p;
  // the free list / slot map (ENC ints, literal_step and the last frame's
  // TopPaths) shares the room of the hash table and the bloom (>= 16 Wcap
  // bytes): neither is live while it is (the commit rebuilds the table, the
  // next frame's roll clears the bloom)
  cx.freel = (CTCX_LDS int*)p;
  p += a16(4 * (size_t)cx.hts);
  cx.bloom = (CTCX_LDS uint64_t*)p;
  p += a16(8 * (size_t)Wcap);
  // TopN elements: positions [0, max(Wcap, 128 or 256)] (the mask-form sift
  // reads child positions up to 128, or 256 for beams of 129..256, +inf
  // sentinels past the heap), then one dummy store slot per lane
  cx.he = (CTCX_LDS HE<T>*)p;
  cx.hdum = (Wcap > 256 ? Wcap : Wcap > 128 ? 256 : 128) + 2;   // the two-node form reads positions up to 256
  p += ((size_t)cx.hdum + 64) * sizeof(HE<T>);
  cx.est[0] = cx.est[1] = cx.eest = nullptr;
  if (scored) {
    cx.est[0] = (CTCX_LDS T*)p; cx.est[1] = cx.est[0] + (nbuf - 1) * Wcap; cx.eest = cx.est[0] + nbuf * Wcap;
    p += a16(((size_t)nbuf * Wcap + ENC) * sizeof(T));
  }
  if (nbuf == 1) {   // both frame parities name the one buffer
    cx.ot[1] = cx.ot[0]; cx.ob[1] = cx.ob[0]; cx.ol[1] = cx.ol[0]; cx.cb[1] = cx.cb[0]; cx.cn[1] = cx.cn[0];
    cx.lab[1] = cx.lab[0]; cx.par[1] = cx.par[0]; cx.flg[1] = cx.flg[0];
    cx.ha[1] = cx.ha[0]; cx.hb[1] = cx.hb[0];
  }
  cx.row = (CTCX_LDS T*)p;
  cx.wcap = Wcap;
  cx.W = W; cx.C = C; cx.enc = (int)ENC;
}

// ---------------------------------------------------------------------------
// Beam scorer hook (util/ctc_beam_scorer.h:31-65), a compile-time policy.  The
// decoder calls InitializeState on the root (decoder.h:226), ExpandState when a
// child is (re)created in the grow loop (:171) and GetStateExpansionScore on the
// previous-frame score it extends (recursion :103, :114; grow :176, :182).
// ExpandStateEnd / GetStateEndExpansionScore are never called by this decoder
// (TopPaths, :230-261, does not), so the policies have no such members.
// A state is one T per beam (the cached expansion score, as the reference's
// comment suggests).  Scores must be log-probabilities (<= 0): the exact
// skipping in exact_step bounds a child's score by its parent's total.

// BaseBeamScorer, the scorer the reference op uses (kernels.cc:260): identity.
template <typename T>
struct BaseBeamScorer {
  static constexpr bool kStateful = false;
  __host__ __device__ static T expand(const Ctx<T>&, T, int, int) { return T(0); }
  __host__ __device__ static T score(T, T prev) { return prev; }
};

// A bigram expansion score: ExpandState caches table[from_label + 1][to_label]
// (row 0: expansions of the root, label -1); GetStateExpansionScore adds it.
template <typename T>
struct BigramBeamScorer {
  static constexpr bool kStateful = true;
  __host__ __device__ static T expand(const Ctx<T>& cx, T, int from_label, int to_label) {
    return cx.sctab[(int64_t)(from_label + 1) * cx.C + to_label];
  }
  __host__ __device__ static T score(T state, T prev) { return prev + state; }
};

// Alignment candidate "from S.kind" for a receiver (ctc_beam_entry.h:190-228).
// restart: the base probability when S has no candidate of that kind.
template <typename T>
__host__ __device__ __forceinline__ void cand_from(const Ctx<T>& cx, int buf, int src, int kind, T p, T restart,
                                          Best<T>& best) {
  const int f = sel(cx.flg, buf)[src];
  const bool has = (f & (kind == 0 ? F_HB : F_HN)) != 0;
  const T base = has ? (kind == 0 ? sel(cx.cb, buf)[src] : sel(cx.cn, buf)[src]) : restart;
  best.push(base + p, has ? (((uint32_t)src << 1) | (uint32_t)kind) : kBpRestart);
}

// Recursion for the branch at position i (decoder.h:95-143) into its entry e
// (e == i, except for a second occurrence of an entry the beam holds twice,
// whose entry is its first occurrence's).  Reads the frame-start branch arrays
// and the entry's current newp (rolled = oldp, except in literal mode where a
// parent processed earlier, or an earlier occurrence, may have changed it).
template <typename T, class SC>
__host__ __device__ __forceinline__ void recurse_branch(const Ctx<T>& cx, int buf, int i, int e, T norm,
                                                        bool literal) {
  const T NI = ninf<T>();
  const int f = sel(cx.flg, buf)[i];
  const int L = sel(cx.lab, buf)[i];
  const bool isroot = (f & F_ROOT) != 0;
  const T o_t = sel(cx.ot, buf)[i];
  const bool fresh = (o_t == NI);
  // restart base for a from-blank candidate with receiver i
  const T rs_blank = (isroot || ((f & F_PROOT) && fresh)) ? T(0) : NI;
  T nl = cx.el[e];
  Best<T> bn{T(0), kBpNone, false}, bb{T(0), kBpNone, false};
  if (!isroot) {
    const T xl = cx.row[L];
    const T p = xl - norm;
    const int P = sel(cx.par, buf)[i];
    const bool pactive = (P >= 0) && (!literal || cx.et[P] != NI);
    if (pactive) {
      const bool same = (L == sel(cx.lab, buf)[P]);
      T prev = same ? sel(cx.ob, buf)[P] : sel(cx.ot, buf)[P];
      if constexpr (SC::kStateful) prev = SC::score(sel(cx.est, buf)[i], prev);
      nl = lse(nl, prev, cx.etab) + xl - norm;
      cand_from(cx, buf, P, 0, p, rs_blank, bn);
      if (!same) cand_from(cx, buf, P, 1, p, NI, bn);
      cand_from(cx, buf, i, 1, p, NI, bn);
    } else {
      nl += xl - norm;
      cand_from(cx, buf, i, 1, p, NI, bn);
    }
  }
  const T xb = cx.row[cx.blank];
  const T nbk = o_t + xb - norm;
  const T pb = xb - norm;
  // new candidates pushed by an earlier occurrence of the same entry are kept
  // (first-pushed maximum across both visits)
  const int ef = cx.eflg[e];
  if (ef & F_HB) { bb.ok = true; bb.p = cx.ecb[e]; bb.bp = cx.ebpb[e]; }
  if (ef & F_HN) {
    Best<T> prior{cx.ecn[e], cx.ebpn[e], true};
    if (bn.ok) prior.push(bn.p, bn.bp);
    bn = prior;
  }
  cand_from(cx, buf, i, 0, pb, rs_blank, bb);
  cand_from(cx, buf, i, 1, pb, NI, bb);
  cx.eb[e] = nbk;
  cx.el[e] = nl;
  cx.et[e] = lse(nbk, nl, cx.etab);
  cx.ecb[e] = bb.p; cx.ebpb[e] = bb.bp;
  cx.ecn[e] = bn.p; cx.ebpn[e] = bn.bp;
  cx.eflg[e] = (bb.ok ? F_HB : 0) | (bn.ok ? F_HN : 0);
  cx.ekind[e] = ((uint32_t)e << 1);
  cx.elab[e] = L;
  if constexpr (SC::kStateful) cx.eest[e] = sel(cx.est, buf)[i];
}

// ---------------------------------------------------------------------------
// Exact TopN heap operations on LDS (position p of gtl::TopN::elements_ lives
// at he[p + 1], so the two children of node h, positions 2h+1 and 2h+2, are
// one 16-byte aligned pair).  Values travel with the slot id, exactly as the
// reference compares BeamEntry* through their newp.total.

// libstdc++ __adjust_heap + __push_heap, one lane, on positions [0, len).
template <typename T>
__host__ __device__ void lane_adjust_heap(CTCX_LDS HE<T>* he, int hole, int len, HE<T> value) {
  const int top = hole;
  int second = hole;
  while (second < (len - 1) / 2) {
    second = 2 * (second + 1);
    HE<T> l, r;
    he_ld2(he, second, l, r);          // positions second-1, second
    if (r.v > l.v) { second--; r = l; }
    he_st(he, hole + 1, r);
    hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) {
    second = 2 * (second + 1);
    he_st(he, hole + 1, he_ld(he, second));
    hole = second - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top) {
    const HE<T> pe = he_ld(he, parent + 1);
    if (!(pe.v > value.v)) break;
    he_st(he, hole + 1, pe);
    hole = parent;
    parent = (hole - 1) / 2;
  }
  he_st(he, hole + 1, value);
}

// std::make_heap over [0, len).  Parents at one depth own disjoint subtrees,
// so each level's sift-downs run in parallel lanes (deepest level first, the
// order libstdc++ visits them in).
template <typename T>
__device__ void wave_make_heap(CTCX_LDS HE<T>* he, int len) {
  if (len < 2) return;
  const int last = (len - 2) / 2;
  const int dmax = 31 - __builtin_clz((unsigned)(last + 1));
  for (int d = dmax; d >= 0; --d) {
    const int lo = (1 << d) - 1;
    const int hi = min((1 << (d + 1)) - 2, last);
    for (int i = lo + (int)threadIdx.x; i <= hi; i += 64) lane_adjust_heap(he, i, len, he_ld(he, i + 1));
  }
}

// Ancestors of 1-based heap node J (J >> 1, J >> 2, ..., 1, i.e. 0-based
// positions (J >> k) - 1): anc has a bit at each ancestor's position and req
// the direction that ancestor's min child must take for J to be on its min
// path (1 = right, i.e. J's bit just below the ancestor's prefix is 1).
// Lane constants: the compiler hoists them out of every loop.
__device__ __forceinline__ void anc_bits(unsigned J, unsigned& anc, unsigned& req) {
  // fixed trip count, no branches: straight-line in the lane id, so hoisted
  anc = 0;
  req = 0;
#pragma unroll
  for (int k = 1; k <= 6; ++k) {   // J <= 64: at most 6 ancestors, all below position 32
    const unsigned a = J >> k;
    const unsigned pos = (a - 1u) & 31u;
    const unsigned on = a != 0u ? 1u : 0u;
    anc |= on << pos;
    req |= (on & (J >> (k - 1))) << pos;
  }
}
template <int NW>
__device__ __forceinline__ void anc_bits_wide(unsigned J, uint64_t (&anc)[NW], uint64_t (&req)[NW]) {
#pragma unroll
  for (int w = 0; w < NW; ++w) { anc[w] = 0; req[w] = 0; }
#pragma unroll
  for (int k = 1; k <= 8; ++k) {   // J <= 256
    const unsigned a = J >> k;
    const unsigned pos = a - 1u;
    const uint64_t on = a != 0u ? 1ull : 0ull;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const uint64_t here = ((pos >> 6) == (unsigned)w) ? on : 0ull;
      anc[w] |= here << (pos & 63u);
      req[w] |= (here & (uint64_t)(J >> (k - 1))) << (pos & 63u);
    }
  }
}

// Per-lane constants of the sift over a heap of `len` elements (lane j owns
// nodes j + 64 r).  Computed once per length: the push loop's length is fixed.
template <int RN>
struct HeapGeo {
  int nint;                          // nodes with at least one child (uniform)
  int dum;                           // he index of this lane's dummy store slot
  int pair[RN];                      // he index of the child pair of node min(j, nint - 1)
  unsigned has_r[RN];                // that node has a right child
  unsigned off[RN];                  // node j has no children (not on any sift path)
  unsigned leaf_l[RN], leaf_r[RN];   // its left / right child has no children
  unsigned anc[RN], req[RN];         // RN == 1: ancestor bits / required directions
  uint64_t anc_w[RN][RN > 1 ? RN / 2 : 1], req_w[RN][RN > 1 ? RN / 2 : 1];
};

template <int RN>
__device__ __forceinline__ HeapGeo<RN> heap_geo(int len, int dum_base) {
  HeapGeo<RN> g;
  const int lane = threadIdx.x;
  len = uni(len);
  g.nint = len / 2;
  g.dum = dum_base + lane;
  const int imax = g.nint > 0 ? g.nint - 1 : 0;
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    const int j = r * 64 + lane;
    const int i = min(j, imax);
    g.pair[r] = 2 * i + 2;
    g.has_r[r] = (2 * i + 2 < len) ? 1u : 0u;
    g.off[r] = (j >= g.nint) ? 1u : 0u;
    g.leaf_l[r] = (2 * j + 1 >= g.nint) ? 1u : 0u;
    g.leaf_r[r] = (2 * j + 2 >= g.nint) ? 1u : 0u;
    if (RN == 1) anc_bits((unsigned)j + 1u, g.anc[r], g.req[r]);
    else anc_bits_wide<(RN > 1 ? RN / 2 : 1)>((unsigned)j + 1u, g.anc_w[r], g.req_w[r]);
  }
  return g;
}

// __adjust_heap(0, len, v) for the whole wave.  The hole descends along the
// smaller child (right on ties) to a leaf and v then rises while its parent is
// strictly greater; since values along that path are non-decreasing, v stops
// at the first node of the root's min-child path whose min child is > v (or
// whose min child is a leaf, which v then takes), and every path node above
// the stop takes its min child.  A single wave pays a pipeline round trip for
// every VALU -> scalar hand-off, so the path is found lane-parallel instead of
// by walking it: every lane loads the child pair of its node(s) (one LDS
// batch), one ballot gives the min-child directions of all nodes, each lane
// checks with its precomputed ancestor masks that every ancestor of its node
// points toward it (its node is then on the path), and a second ballot +
// find-first-set yields the stop.  Every lane then stores unconditionally --
// to its real target or to its dummy slot -- so no exec-mask blocks.  If
// vpos >= 0 v is read from position vpos in the same LDS batch (pop_heap).
// Returns the new root.
template <typename T, int RN>
struct HeapPairs {
  HE<T> L[RN], R[RN];
};

// The sift's LDS reads (every lane's child pair), split off so that the push
// loop can issue them before it selects the next event: they depend only on
// the previous sift's stores, and their latency then overlaps the selection.
template <typename T, int RN>
__device__ __forceinline__ void heap_pairs(CTCX_LDS HE<T>* he, const HeapGeo<RN>& g, HeapPairs<T, RN>& hp) {
#pragma unroll
  for (int r = 0; r < RN; ++r) he_ld2(he, g.pair[r], hp.L[r], hp.R[r]);
}

template <typename T, int RN>
__device__ __forceinline__ HE<T> wave_adjust_heap_p(CTCX_LDS HE<T>* he, const HeapGeo<RN>& g, HE<T> v,
                                                    const HeapPairs<T, RN>& hp);

template <typename T, int RN>
__device__ __forceinline__ HE<T> wave_adjust_heap(CTCX_LDS HE<T>* he, const HeapGeo<RN>& g, HE<T> v,
                                                  int vpos = -1) {
  if (vpos >= 0) v = he_ld(he, uni(vpos) + 1);
  HeapPairs<T, RN> hp;
  heap_pairs<T, RN>(he, g, hp);
  return wave_adjust_heap_p<T, RN>(he, g, v, hp);
}

template <typename T, int RN>
__device__ __forceinline__ HE<T> wave_adjust_heap_p(CTCX_LDS HE<T>* he, const HeapGeo<RN>& g, HE<T> v,
                                                    const HeapPairs<T, RN>& hp) {
  const int lane = threadIdx.x;
  const HE<T>* L = hp.L;
  const HE<T>* R = hp.R;
  T cv[RN];
  int cs[RN];
  unsigned pk[RN];
  uint64_t bm[RN];
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    const bool pick_r = g.has_r[r] && !(R[r].v > L[r].v);
    bm[r] = __ballot(pick_r);
    pk[r] = pick_r ? 1u : 0u;
    cv[r] = pick_r ? R[r].v : L[r].v;
    cs[r] = pick_r ? R[r].s : L[r].s;
  }
  const T c0 = bcast(cv[0], 0);
  const int s0 = bcast(cs[0], 0);
  uint64_t cm[RN];
  unsigned offp[RN], gtv[RN];
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    unsigned mis;   // nonzero: some ancestor's min child is not the one toward this node
    if (RN == 1) {
      mis = ((unsigned)bm[0] ^ g.req[r]) & g.anc[r];   // ancestors of nodes < 64 are < 32
    } else {
      mis = 0;
#pragma unroll
      for (int w = 0; w < (RN > 1 ? RN / 2 : 1); ++w)
        mis |= ((bm[w] ^ g.req_w[r][w]) & g.anc_w[r][w]) != 0ull ? 1u : 0u;
    }
    offp[r] = mis | g.off[r];
    gtv[r] = (cv[r] > v.v) ? 1u : 0u;
    const unsigned leaf = pk[r] ? g.leaf_r[r] : g.leaf_l[r];
    cm[r] = __ballot((offp[r] | ((gtv[r] | leaf) ^ 1u)) == 0u);
  }
  int kk = -1;
#pragma unroll
  for (int r = RN - 1; r >= 0; --r)
    if (cm[r]) kk = r * 64 + (int)__builtin_ctzll(cm[r]);
  if (kk < 0) {                       // no internal nodes: v is the root
    he_st(he, lane == 0 ? 1 : g.dum, v);
  } else {
#pragma unroll
    for (int r = 0; r < RN; ++r) {
      const int j = r * 64 + lane;
      const bool up = offp[r] == 0u && (j < kk || (j == kk && gtv[r] == 0u));
      he_st(he, up ? j + 1 : g.dum, HE<T>{cv[r], cs[r]});
      he_st(he, j == kk ? (gtv[r] ? j : 2 * j + 1 + (int)pk[r]) + 1 : g.dum, v);
    }
  }
  HE<T> res;
  const bool keep = (g.nint == 0) || (c0 > v.v);
  res.v = keep ? v.v : c0;
  res.s = keep ? v.s : s0;
  return res;
}

// The HEAP_SORTED push, __adjust_heap(0, W, v) with the same decisions as
// wave_adjust_heap_p, but without a scalar hand-off on its dependency chain:
// the stop needs no find-first-set -- a path node is the stop iff it meets the
// stop condition and none of its ancestors (a mask test against the second
// ballot) does -- and the new root comes back in VGPRs (fv, fs: uniform
// values), so the next event's compare reads it without a VALU -> SALU trip.
// Requires g.nint > 0 (W >= 2).
template <typename T, int RN>
__device__ __forceinline__ void wave_push_heap_v(CTCX_LDS HE<T>* he, const HeapGeo<RN>& g, T vv, int vs,
                                                 const HeapPairs<T, RN>& hp, T& fv, int& fs) {
  const int lane = threadIdx.x;
  if (g.nint == 0) {   // a heap of one: v is the root (uniform branch)
    he_st(he, lane == 0 ? 1 : g.dum, HE<T>{vv, vs});
    fv = vv;
    fs = vs;
    return;
  }
  const HE<T>* L = hp.L;
  const HE<T>* R = hp.R;
  T cv[RN];
  int cs[RN];
  unsigned pk[RN];
  uint64_t bm[RN];
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    const bool pick_r = g.has_r[r] && !(R[r].v > L[r].v);
    bm[r] = __ballot(pick_r);
    pk[r] = pick_r ? 1u : 0u;
    cv[r] = pick_r ? R[r].v : L[r].v;
    cs[r] = pick_r ? R[r].s : L[r].s;
  }
  const T c0 = bcast(cv[0], 0);
  const int s0 = bcast(cs[0], 0);
  uint64_t cm[RN];
  bool onp[RN], gtv[RN], cnd[RN];
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    unsigned mis;
    if (RN == 1) {
      mis = ((unsigned)bm[0] ^ g.req[r]) & g.anc[r];
    } else {
      mis = 0;
#pragma unroll
      for (int w = 0; w < (RN > 1 ? RN / 2 : 1); ++w)
        mis |= ((bm[w] ^ g.req_w[r][w]) & g.anc_w[r][w]) != 0ull ? 1u : 0u;
    }
    onp[r] = (mis | g.off[r]) == 0u;
    gtv[r] = cv[r] > vv;
    const unsigned leaf = pk[r] ? g.leaf_r[r] : g.leaf_l[r];
    cnd[r] = gtv[r] || leaf != 0u;
    cm[r] = __ballot(onp[r] && cnd[r]);
  }
#pragma unroll
  for (int r = 0; r < RN; ++r) {
    bool above;   // a proper ancestor on the path already meets the stop condition
    if (RN == 1) {
      above = ((unsigned)cm[0] & g.anc[r]) != 0u;
    } else {
      above = false;
#pragma unroll
      for (int w = 0; w < (RN > 1 ? RN / 2 : 1); ++w) above |= (cm[w] & g.anc_w[r][w]) != 0ull;
    }
    const int j = r * 64 + lane;
    const bool live = onp[r] && !above;
    const bool up = live && !gtv[r];   // takes its min child (above the stop, or the stop with v below it)
    const bool isk = live && cnd[r];   // the stop: v lands here or in its min child's position
    he_st(he, up ? j + 1 : g.dum, HE<T>{cv[r], cs[r]});
    he_st(he, isk ? (gtv[r] ? j : 2 * j + 1 + (int)pk[r]) + 1 : g.dum, HE<T>{vv, vs});
  }
  const bool keep = c0 > vv;
  fv = keep ? vv : c0;
  fs = keep ? vs : s0;
}

// ---------------------------------------------------------------------------
// The same sift for heaps of up to 128 elements (one node with children per
// lane), written as lane-mask algebra: every per-node predicate is a 64-bit
// mask in SGPRs (a ballot), combined on the scalar unit and turned back into a
// per-lane select by inverse_ballot, which the compiler lowers to a
// v_cndmask on the mask itself.  One wave issues one instruction per ~4
// cycles, and the mask form needs about half the instructions of the
// bool-per-lane form above, with the same decisions.
//
// No per-length geometry: every position at or past the heap's length holds
// a +inf sentinel (heap_sentinels; pop_heap sets each vacated position), so
//   * a node without a right child never picks it (+inf > left),
//   * a lane whose node has no children sees a min child of +inf: on the
//     min-child path it is a leaf, the stop, and v lands on it -- exactly where
//     __adjust_heap's hole would end;
// and the only leaves that are not lanes are the children of nodes 31..63
// (positions >= 64), a constant mask.
// Lane `lane` of `old` takes the uniform `val` (a v_writelane; this toolchain
// has no builtin for it, and an asm one would need M0 on gfx950's constant
// bus): one scalar shift and one v_cndmask on the resulting lane mask.
__device__ __forceinline__ int writelane(int old, int val, int lane) {
  return __builtin_amdgcn_inverse_ballot_w64(1ull << lane) ? val : old;
}
__device__ __forceinline__ float writelane(float old, float val, int lane) {
  return __builtin_amdgcn_inverse_ballot_w64(1ull << lane) ? val : old;
}

__device__ __forceinline__ uint64_t lowmask(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

struct HeapM {
  unsigned anc, req;        // ancestor bits of node j and the directions toward it
  int aj, al, ar, dum;      // he indices: node j, its left and right child, this lane's dummy slot
};

__device__ __forceinline__ HeapM heap_m(int dum_base) {
  HeapM g;
  const unsigned j = threadIdx.x;
  anc_bits(j + 1u, g.anc, g.req);
  g.aj = (int)j + 1;
  g.al = 2 * (int)j + 2;
  g.ar = 2 * (int)j + 3;
  g.dum = dum_base + (int)j;
  return g;
}

// +inf at positions [from, to] (to = 128: he[from + 1 .. 129], every child
// position a lane can read in the one-node-per-lane form; 256 in the two-node form)
template <typename T>
__device__ __forceinline__ void heap_sentinels(CTCX_LDS HE<T>* he, int from, int to = 128) {
  for (int q = from + (int)threadIdx.x; q <= to; q += 64) he_st(he, q + 1, HE<T>{pinf<T>(), -1});
}

template <typename T>
__device__ __forceinline__ void pairs_m(const CTCX_LDS HE<T>* he, const HeapM& g, HE<T>& L, HE<T>& R) {
  he_ld2(he, g.al, L, R);
}

// __adjust_heap(0, len, v) for len in [2, 128] with the sentinels in place:
// stores the moves; returns the old root's min child (c0, s0) and whether v
// stayed at the root (keep: the new root is then v, else c0).
template <typename T>
__device__ __forceinline__ void push_m(CTCX_LDS HE<T>* he, const HeapM& g, T vv, int vs, HE<T> L, HE<T> R,
                                       T& c0, int& s0, bool& keep) {
  const uint64_t pickR = __ballot(!(R.v > L.v));   // min child on the right (ties: right)
  const bool pr = __builtin_amdgcn_inverse_ballot_w64(pickR);
  const T cv = pr ? R.v : L.v;
  const int cs = pr ? R.s : L.s;
  // on the root's min-child path: every ancestor's min child points here
  const uint64_t onp = __ballot((((unsigned)pickR ^ g.req) & g.anc) == 0u);
  const uint64_t gt = __ballot(cv > vv);
  // stop: min child > v, or the min child is a leaf that is not a lane
  // (children of nodes >= 32; node 31's right child)
  const uint64_t cnd = gt | 0xffffffff00000000ull | (pickR & 0x80000000ull);
  const uint64_t cm = onp & cnd;
  const uint64_t live = onp & ~__ballot((((unsigned)cm) & g.anc) != 0u);   // at or above the stop
  const bool up = __builtin_amdgcn_inverse_ballot_w64(live & ~gt);   // takes its min child
  const bool isk = __builtin_amdgcn_inverse_ballot_w64(live & cnd);  // the stop: v lands here or in its min child
  const bool vg = __builtin_amdgcn_inverse_ballot_w64(gt);
  he_st(he, up ? g.aj : g.dum, HE<T>{cv, cs});
  he_st(he, isk ? (vg ? g.aj : (pr ? g.ar : g.al)) : g.dum, HE<T>{vv, vs});
  c0 = uni(cv);
  s0 = uni(cs);
  keep = (gt & 1ull) != 0ull;
}

// The same sift for heaps of 129..256 elements: lane j owns node j (group 0)
// and node j + 64 (group 1).  Every ancestor of a group-1 node is in group 0
// (its parent is node 31..63), and every child of a group-1 node is a leaf
// that is not a lane, so group 1 adds one ballot per predicate and its own
// pair of stores; the stop is still unique (path nodes are ancestors of one
// another).  Sentinels at positions [len, 256].
struct HeapM2 {
  HeapM g;              // group 0 (the one-node form's geometry)
  uint64_t anc1, req1;  // node j + 64: its ancestors (all in group 0) and the directions toward it
};

__device__ __forceinline__ HeapM2 heap_m2(int dum_base) {
  HeapM2 m;
  m.g = heap_m(dum_base);
  uint64_t a[1], r[1];
  anc_bits_wide<1>(threadIdx.x + 65u, a, r);
  m.anc1 = a[0];
  m.req1 = r[0];
  return m;
}

template <typename T>
__device__ __forceinline__ void pairs_m2(const CTCX_LDS HE<T>* he, const HeapM2& g, HE<T> (&L)[2], HE<T> (&R)[2]) {
  he_ld2(he, g.g.al, L[0], R[0]);
  he_ld2(he, g.g.al + 128, L[1], R[1]);
}

template <typename T>
__device__ __forceinline__ void push_m2(CTCX_LDS HE<T>* he, const HeapM2& g, T vv, int vs, const HE<T> (&L)[2],
                                        const HE<T> (&R)[2], T& c0, int& s0, bool& keep) {
  const uint64_t pR0 = __ballot(!(R[0].v > L[0].v)), pR1 = __ballot(!(R[1].v > L[1].v));
  const bool pr0 = __builtin_amdgcn_inverse_ballot_w64(pR0), pr1 = __builtin_amdgcn_inverse_ballot_w64(pR1);
  const T cv0 = pr0 ? R[0].v : L[0].v, cv1 = pr1 ? R[1].v : L[1].v;
  const int cs0 = pr0 ? R[0].s : L[0].s, cs1 = pr1 ? R[1].s : L[1].s;
  const uint64_t onp0 = __ballot((((unsigned)pR0 ^ g.g.req) & g.g.anc) == 0u);
  const uint64_t onp1 = __ballot(((pR0 ^ g.req1) & g.anc1) == 0ull);
  const uint64_t gt0 = __ballot(cv0 > vv), gt1 = __ballot(cv1 > vv);
  // group 0's one child that is not a lane: node 63's right child (position 128)
  const uint64_t cnd0 = gt0 | (pR0 & 0x8000000000000000ull);
  const uint64_t cm0 = onp0 & cnd0;
  const uint64_t live0 = onp0 & ~__ballot((((unsigned)cm0) & g.g.anc) != 0u);
  const uint64_t live1 = onp1 & ~__ballot((cm0 & g.anc1) != 0ull);
  const bool up0 = __builtin_amdgcn_inverse_ballot_w64(live0 & ~gt0);
  const bool isk0 = __builtin_amdgcn_inverse_ballot_w64(live0 & cnd0);
  const bool vg0 = __builtin_amdgcn_inverse_ballot_w64(gt0);
  const bool up1 = __builtin_amdgcn_inverse_ballot_w64(live1 & ~gt1);
  const bool isk1 = __builtin_amdgcn_inverse_ballot_w64(live1);
  const bool vg1 = __builtin_amdgcn_inverse_ballot_w64(gt1);
  he_st(he, up0 ? g.g.aj : g.g.dum, HE<T>{cv0, cs0});
  he_st(he, isk0 ? (vg0 ? g.g.aj : (pr0 ? g.g.ar : g.g.al)) : g.g.dum, HE<T>{vv, vs});
  he_st(he, up1 ? g.g.aj + 64 : g.g.dum, HE<T>{cv1, cs1});
  he_st(he, isk1 ? (vg1 ? g.g.aj + 64 : (pr1 ? g.g.ar + 128 : g.g.al + 128)) : g.g.dum, HE<T>{vv, vs});
  c0 = uni(cv0);
  s0 = uni(cs0);
  keep = (gt0 & 1ull) != 0ull;
}

// The mask-form sift for RN = 1 (one node per lane) or 2 (two), one interface.
template <int RN> struct MaskGeo { using type = HeapM; };
template <> struct MaskGeo<2> { using type = HeapM2; };
template <int RN>
__device__ __forceinline__ typename MaskGeo<RN>::type mask_geo(int dum_base) {
  if constexpr (RN == 2) return heap_m2(dum_base);
  else return heap_m(dum_base);
}
template <typename T, int RN>
struct MPairs {
  HE<T> L[RN == 2 ? 2 : 1], R[RN == 2 ? 2 : 1];
};
template <typename T, int RN>
__device__ __forceinline__ void mpairs(const CTCX_LDS HE<T>* he, const typename MaskGeo<RN>::type& g,
                                       MPairs<T, RN>& p) {
  if constexpr (RN == 2) pairs_m2(he, g, p.L, p.R);
  else pairs_m(he, g, p.L[0], p.R[0]);
}
template <typename T, int RN>
__device__ __forceinline__ void mpush(CTCX_LDS HE<T>* he, const typename MaskGeo<RN>::type& g, T vv, int vs,
                                      const MPairs<T, RN>& p, T& c0, int& s0, bool& keep) {
  if constexpr (RN == 2) push_m2(he, g, vv, vs, p.L, p.R, c0, s0, keep);
  else push_m<T>(he, g, vv, vs, p.L[0], p.R[0], c0, s0, keep);
}

// std::make_heap over [0, len), len in [2, 129], in the mask form: one sift
// per level for all of the level's nodes at once (their subtrees are
// disjoint), each the push_m sift started at the lane's ancestor of that
// depth instead of the root -- one LDS read batch, the ballots and one store
// batch per level, where wave_make_heap walks every sift down and back up one
// dependent LDS round trip per step (28 down and as many up at len = 129).
// Same result: below a node being sifted both subtrees are heaps already, so
// the values along its min-child path do not decrease, and __adjust_heap's
// hole-to-a-leaf-then-__push_heap leaves v at the first path node whose min
// child is > v, or in a min child that is a leaf (push_m's argument, per
// subtree).  A node without children sees +inf sentinels and keeps its value,
// as does the missing right child of an even length: positions [len, 128]
// must hold the sentinels.  Lanes past the level's nodes store to their dummies.
// ROOT_MIN: position 0 holds -inf and every other value is above it (the
// evicted front of a full beam), so the root's sift is left out: the hole
// would run down to a leaf and -inf rise back to the root, moving every path
// node up and down again.
template <typename T, bool ROOT_MIN>
__device__ __forceinline__ void wave_make_heap_m(CTCX_LDS HE<T>* he, const HeapM& g, int len) {
  const unsigned J = threadIdx.x + 1u;                       // this lane's node, 1-based
  const int dj = 31 - (int)__builtin_clz(J);                 // its depth
  const int last = (len - 2) / 2;                            // the last node with a child
#pragma unroll
  for (int d = 6; d >= (ROOT_MIN ? 1 : 0); --d) {
    const int lo = (1 << d) - 1;                             // the level's first position
    if (lo > last) continue;                                 // (uniform) no node of this level has a child
    const bool in = dj >= d;                                 // in the subtree of a node of this level
    const int r1 = in ? (int)(J >> (dj - d)) : 1;            // that node (he index: position + 1)
    // ancestors inside the subtree (positions >= lo; every ancestor of a lane's node is below 32)
    const unsigned ancd = lo >= 32 ? 0u : (g.anc & ~((1u << lo) - 1u));
    HE<T> L, R;
    he_ld2(he, g.al, L, R);
    const HE<T> v = he_ld(he, r1);
    const uint64_t pickR = __ballot(!(R.v > L.v));           // min child on the right (ties: right)
    const bool pr = __builtin_amdgcn_inverse_ballot_w64(pickR);
    const T cv = pr ? R.v : L.v;
    const int cs = pr ? R.s : L.s;
    // on its level node's min-child path: every ancestor in the subtree points here
    const uint64_t onp = __ballot(in && (((unsigned)pickR ^ g.req) & ancd) == 0u);
    const uint64_t gt = __ballot(cv > v.v);
    const uint64_t cnd = gt | 0xffffffff00000000ull | (pickR & 0x80000000ull);   // (push_m's stop)
    const uint64_t cm = onp & cnd;
    const uint64_t live = onp & ~__ballot((((unsigned)cm) & ancd) != 0u);        // at or above its path's stop
    const bool up = __builtin_amdgcn_inverse_ballot_w64(live & ~gt);             // takes its min child
    const bool isk = __builtin_amdgcn_inverse_ballot_w64(live & cnd);            // the stop
    const bool vg = __builtin_amdgcn_inverse_ballot_w64(gt);
    he_st(he, up ? g.aj : g.dum, HE<T>{cv, cs});
    he_st(he, isk ? (vg ? g.aj : (pr ? g.ar : g.al)) : g.dum, v);
  }
}

// The HEAP_SORTED event loop for float beams of up to 128 (exact_step), as one
// hand-scheduled asm block: the same selections, bookkeeping and push_m sift as
// the C++ loop it replaces, in ~42 instructions per accepted offer (the
// compiled loop took ~85, with the uniform state spilled into VGPR lanes).
// The stop is found per lane, as in extract_fwd_f32, and on the vector unit
// alone: a lane is live iff it is on the root's min-child path and no proper
// ancestor has gt (ancestors of a lane are below 32: gt's low word) -- one
// v_and_or of the gt mask into the path test and one v_cmp.  The other way to
// stop, a min child that is not a lane, needs no term there: lanes 32..63
// are nobody's ancestor, and the one lane below lane 31 is lane 63, its left
// child, which the path test drops when lane 31 picks right.  The lanes that
// take their min child are live & ~gt (two selects: gt ? dummy : node, then
// live ? that : dummy).  The stop is not formed as a mask: a live lane writes
// v to its node (gt), else to its min child where that is not a lane (alx,
// arx: the child's address in the lanes whose child on that side is past
// position 63, the dummy elsewhere), else to its dummy -- and only one live
// lane has such a place, since every deeper path node has it above itself.
// No SALU instruction stands between gt and the stores: in
// tools/push_unit.hip the loop with the stop found by s_ff1 takes 333 cycles
// per push, the same per-lane test fed from a scalar stop-condition word 345,
// this form 281, and 277 / 274 with two / four copies of the push body per
// loop trip (CTCX_PUSH_COPIES, four: only the last copy branches back, each
// copy has its own evicted-branch stub to return to).  The same programme
// priced the order below: the new front and the next selection's compare
// after the stores and the read (before them: +8 cycles), and CTCX_BAT_A
// and a select between the v_cmp that writes live and the selects that read
// it (with CTCX_BAT_A after the read and one instruction in that gap: +16).
// tests/test_cpu_push_stop.py is the rule on the host against the
// first-set-bit form and libstdc++.  It
// runs until no live lane wants in (returns 0) or the next wanted lane k
// re-offers a branch child (returns 1: the caller decides that event).  It is
// software-pipelined: the next push's child pairs are read right after the
// stores, and the new front and the next event's selection run in the shadow
// of that read.
//   state (SGPR): NC / RB / done lane masks, the front (fv, fs), the bump
//   pointer, the eviction-record count; (VGPR): myslot, evr, bat.
//   he addresses are LDS byte addresses: node j (aj), its child pair (al, ar),
//   the lane's dummy slot (dum).
// Hazards: every VALU-written SGPR is read by a VALU two or more instructions
// later (or behind an s_nop); DS operand registers are rewritten only after
// the s_waitcnt lgkmcnt(0) that retires their instruction; lane selects come
// from SALU.  Temporaries: s84..s99, vcc, v232..v243 (clobbered).
// The bottom each lane's branch turn sees (bat; decoder.h:151-159) is
// refreshed after each push in every later turn's lane (CTCX_BAT_A/B/C: a
// compare, a move and a select, spread over the push).
#define CTCX_BAT_A "v_cmp_lt_i32_e64 vcc, %[k], %[sl]\n\t"   /* turns starting after lane k see the new bottom */
#define CTCX_BAT_B "v_mov_b32_e32 v242, %[fv]\n\t"
#define CTCX_BAT_C "v_cndmask_b32_e32 %[bat], %[bat], v242, vcc\n\t"
#ifdef CTCX_PHASES
#define CTCX_EVCNT "s_add_u32 %[cnt], %[cnt], 1\n\t"   // diagnostics builds: count the pushes
#else
#define CTCX_EVCNT ""
#endif
// the push's min child (value, slot), its path mask, and the two node stores
#define CTCX_HEV_CV "v237"
#define CTCX_HEV_CS "v238"
#define CTCX_HEV_BT "v239"
#define CTCX_HEV_STORES "ds_write2_b32 v239, v237, v238 offset1:1\n\tds_write2_b32 v236, v240, v241 offset1:1\n\t"
// One push and the next selection; N is the copy's label suffix.  It ends with
// SCC = (the next wanted lane k re-offers a branch child).
#define CTCX_HEV_PUSH(N)                                                                                     \
      ".Lev_tail" N "_%=:\n\t"                                                                               \
      "s_lshl_b64 s[80:81], -2, %[k]\n\t"                  /* lanes after k */                              \
      "v_readlane_b32 s84, %[s], %[k]\n\t"                 /* v = offer k's score */                        \
      "s_mov_b32 s85, %[fs]\n\t"                           /* slot = the front's */                         \
      "s_cmp_lt_i32 %[fs], %[nb]\n\t"                                                                        \
      "s_cbranch_scc1 .Lev_evb" N "_%=\n"                                                                    \
      ".Lev_slot" N "_%=:\n\t"                                                                               \
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[my]\n\t"        /* an entry accepted in this chunk is the evicted front */ \
      "s_mov_b32 m0, %[k]\n\t"                                                                               \
      "v_cndmask_b32_e64 %[my], %[my], -1, s[90:91]\n\t"                                                     \
      "v_writelane_b32 %[my], s85, m0\n\t"                 /* lane k: its entry's slot */                   \
      CTCX_EVCNT                                                                                             \
      "s_waitcnt lgkmcnt(0)\n\t"                                                                             \
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         /* pickR = !(R > L) */                           \
      "v_mov_b64_e32 v[240:241], s[84:85]\n\t"                                                               \
      "v_cndmask_b32_e64 " CTCX_HEV_CV ", v232, v234, s[92:93]\n\t"   /* cv */                              \
      "v_cndmask_b32_e64 " CTCX_HEV_CS ", v233, v235, s[92:93]\n\t"   /* cs */                              \
      "v_bitop3_b32 " CTCX_HEV_BT ", s92, %[req], %[anc] bitop3:0x28\n\t"  /* (pickR ^ req) & anc */        \
      "v_cmp_lt_f32_e64 s[96:97], s84, " CTCX_HEV_CV "\n\t"           /* gt: min child > v */               \
      "v_cndmask_b32_e64 v236, %[alx], %[arx], s[92:93]\n\t"/* the min child's address where v may land there */\
      "v_readfirstlane_b32 s86, " CTCX_HEV_CV "\n\t"       /* c0: the root's min child */                    \
      "v_and_or_b32 " CTCX_HEV_BT ", s96, %[anc], " CTCX_HEV_BT "\n\t"/* off the path, or below a gt */      \
      "v_readfirstlane_b32 s87, " CTCX_HEV_CS "\n\t"                                                         \
      "v_cmp_eq_u32_e64 s[94:95], 0, " CTCX_HEV_BT "\n\t"  /* live: path nodes at or above the stop */       \
      "v_cndmask_b32_e64 v236, v236, %[aj], s[96:97]\n\t"  /* v lands on the stop (gt) or in its min child */\
      "v_cndmask_b32_e64 v243, %[aj], %[dum], s[96:97]\n\t"/* no gt: the node takes its min child */         \
      CTCX_BAT_A                                                                                             \
      "v_cndmask_b32_e64 " CTCX_HEV_BT ", %[dum], v243, s[94:95]\n\t"/* up */                                \
      "v_cndmask_b32_e64 v236, %[dum], v236, s[94:95]\n\t" /* the stop */                                    \
      CTCX_HEV_STORES                                                                                        \
      "ds_read_b128 v[232:235], %[al]\n\t"                 /* the next push's child pairs */                 \
      "s_bitcmp1_b32 s96, 0\n\t"                           /* keep: v stays at the root */                   \
      "s_cselect_b32 %[fv], s84, s86\n\t"                  /* the new front */                               \
      "s_cselect_b32 %[fs], s85, s87\n\t"                                                                    \
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"         /* next: s > front */                             \
      CTCX_BAT_B                                                                                             \
      CTCX_BAT_C                                                                                             \
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"                                                              \
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"                                                               \
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"         /* next m */                                     \
      "s_cbranch_scc0 .Lev_exit_%=\n\t"                                                                      \
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"                                                                     \
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
// into the next copy, unless k is rare
#define CTCX_HEV_NEXT "s_cbranch_scc1 .Lev_rare_%=\n"
// the evicted front is a branch's entry: a fresh slot; record the eviction; a
// live re-offer of that branch is now wanted (back to the copy it left)
#define CTCX_HEV_EVB(N)                                                                                      \
      ".Lev_evb" N "_%=:\n\t"                                                                                \
      "s_mov_b32 s85, %[nfree]\n\t"                                                                          \
      "s_add_u32 %[nfree], %[nfree], 1\n\t"                                                                  \
      "s_mov_b32 m0, %[nv]\n\t"                                                                              \
      "s_add_u32 %[nv], %[nv], 1\n\t"                                                                        \
      "v_writelane_b32 %[evr], %[fs], m0\n\t"                                                                \
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[c]\n\t"                                                           \
      "s_and_b64 s[90:91], s[90:91], %[lb]\n\t"                                                              \
      "s_or_b64 %[rb], %[rb], s[90:91]\n\t"                                                                  \
      "s_branch .Lev_slot" N "_%=\n"
#ifndef CTCX_PUSH_COPIES
#define CTCX_PUSH_COPIES 4
#endif
#if CTCX_PUSH_COPIES == 1
#define CTCX_HEV_BODY CTCX_HEV_PUSH("0")
#define CTCX_HEV_EVBS CTCX_HEV_EVB("0")
#elif CTCX_PUSH_COPIES == 2
#define CTCX_HEV_BODY CTCX_HEV_PUSH("0") CTCX_HEV_NEXT CTCX_HEV_PUSH("1")
#define CTCX_HEV_EVBS CTCX_HEV_EVB("0") CTCX_HEV_EVB("1")
#elif CTCX_PUSH_COPIES == 4
#define CTCX_HEV_BODY                                                                                        \
  CTCX_HEV_PUSH("0") CTCX_HEV_NEXT CTCX_HEV_PUSH("1") CTCX_HEV_NEXT CTCX_HEV_PUSH("2") CTCX_HEV_NEXT CTCX_HEV_PUSH("3")
#define CTCX_HEV_EVBS CTCX_HEV_EVB("0") CTCX_HEV_EVB("1") CTCX_HEV_EVB("2") CTCX_HEV_EVB("3")
#else
#error "CTCX_PUSH_COPIES: 1, 2 or 4"
#endif
__device__ __forceinline__ int heap_events_f32(float s, int c, int sl, unsigned anc, unsigned req, unsigned aj,
                                               unsigned al, unsigned ar, unsigned dum, int& myslot, int& evr,
                                               float& bat, uint64_t& NC, uint64_t& RB, uint64_t& done, uint64_t LB,
                                               float& fv, int& fs, int& nfree, int& nv, int nb, int& k, int& cnt) {
  int st;
  // where v lands in a min child that is not a lane (the children of lanes
  // 32..63, lane 31's right child: al - aj is 8 * (lane + 1)); any other min
  // child is on the path itself and not the stop: the dummy
  const unsigned alx = al - aj > 8u * 32u ? al : dum, arx = al - aj > 8u * 31u ? ar : dum;
  // every scalar operand provably uniform (the asm's "s" constraints)
  NC = uni64(NC); RB = uni64(RB); done = uni64(done); LB = uni64(LB);
  fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv); nb = uni(nb); cnt = uni(cnt);
  asm volatile(
      "s_mov_b32 %[st], 0\n\t"
      "s_not_b64 s[80:81], %[done]\n\t"                    // lanes still to come
      // select the first event
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"          // s > front
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"         // m (SCC: m != 0)
      "s_cbranch_scc0 .Lev_exit_%=\n\t"
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
      "s_cbranch_scc1 .Lev_rare_%=\n\t"
      "ds_read_b128 v[232:235], %[al]\n"                   // its child pairs (L.v, L.s, R.v, R.s)
      // event k (v = s84, slot = s85): its bookkeeping, then its push, then
      // the next selection; only the last copy branches back
      CTCX_HEV_BODY
      "s_cbranch_scc0 .Lev_tail0_%=\n\t"                   // the next push, unless k is rare
      "s_branch .Lev_rare_%=\n"
      CTCX_HEV_EVBS
      ".Lev_rare_%=:\n\t"
      "s_mov_b32 %[st], 1\n"
      ".Lev_exit_%=:\n\t"
      "s_not_b64 %[done], s[80:81]\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [my] "+v"(myslot), [evr] "+v"(evr), [bat] "+v"(bat), [nc] "+s"(NC), [rb] "+s"(RB), [done] "+s"(done),
        [fv] "+s"(fv), [fs] "+s"(fs), [nfree] "+s"(nfree), [nv] "+s"(nv), [k] "=&s"(k), [st] "=&s"(st), [cnt] "+s"(cnt)
      : [s] "v"(s), [c] "v"(c), [sl] "v"(sl), [anc] "v"(anc), [req] "v"(req), [aj] "v"(aj), [al] "v"(al),
        [alx] "v"(alx), [arx] "v"(arx), [dum] "v"(dum), [lb] "s"(LB), [nb] "s"(nb)
      : "memory", "vcc", "m0", "s80", "s81", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93",
        "s94", "s95", "s96", "s97", "s98", "s99", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",
        "v240", "v241", "v242", "v243");
  return st;
}

// heap_events_f32 for beams of 129..256 (the push_m2 sift: lane j owns node j,
// group 0, and node j + 64, group 1).  Group 1 adds a second child-pair read
// (offset 1024 B), its own min-child pick, path test (its ancestors are all in
// group 0, so the test reads group 0's pick mask), gt and pair of stores.  The
// stop is the shallowest group-0 path node meeting its stop condition (gt, or
// node 63's min child being position 128, not a lane); when there is none the
// path's group-1 node is the stop (its children are never lanes).  The stop
// mask is live0 & cnd0, which is empty then (s_ff1 gives -1: -2 << 63 = 0).
// Temporaries: s84..s99, vcc, three compiler-chosen SGPR pairs (p1: group 1's
// pick, g1: its gt, o1: its path, then live1), v232..v253 (clobbered).
__device__ __forceinline__ int heap_events_m2_f32(float s, int c, int sl, unsigned anc, unsigned req, unsigned an1l,
                                                  unsigned an1h, unsigned rq1l, unsigned rq1h, unsigned aj,
                                                  unsigned al, unsigned ar, unsigned aj1, unsigned al1, unsigned ar1,
                                                  unsigned dum, int& myslot, int& evr, float& bat, uint64_t& NC,
                                                  uint64_t& RB, uint64_t& done, uint64_t LB, float& fv, int& fs,
                                                  int& nfree, int& nv, int nb, int& k, int& cnt) {
  int st;
  uint64_t p1, g1, o1;
  const uint64_t k63 = 0x8000000000000000ull;
  NC = uni64(NC); RB = uni64(RB); done = uni64(done); LB = uni64(LB);
  fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv); nb = uni(nb); cnt = uni(cnt);
  asm volatile(
      "s_mov_b32 %[st], 0\n\t"
      "s_not_b64 s[80:81], %[done]\n\t"                    // lanes still to come
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"          // s > front
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"         // m (SCC: m != 0)
      "s_cbranch_scc0 .Lem_exit_%=\n\t"
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
      "s_cbranch_scc1 .Lem_rare_%=\n\t"
      "ds_read_b128 v[232:235], %[al]\n\t"                 // group 0 child pairs
      "ds_read_b128 v[244:247], %[al] offset:1024\n"       // group 1 child pairs
      ".Lem_tail_%=:\n\t"
      "s_lshl_b64 s[80:81], -2, %[k]\n\t"                  // lanes after k
      "v_readlane_b32 s84, %[s], %[k]\n\t"                 // v = offer k's score
      "s_mov_b32 s85, %[fs]\n\t"                           // slot = the front's
      "s_cmp_lt_i32 %[fs], %[nb]\n\t"
      "s_cbranch_scc1 .Lem_evb_%=\n"
      ".Lem_slot_%=:\n\t"
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[my]\n\t"        // an entry accepted in this chunk is the evicted front
      "s_mov_b32 m0, %[k]\n\t"
      "v_cndmask_b32_e64 %[my], %[my], -1, s[90:91]\n\t"
      "v_writelane_b32 %[my], s85, m0\n\t"                 // lane k: its entry's slot
      CTCX_EVCNT
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         // pR0 = !(R > L)
      "v_cmp_ngt_f32_e64 %[p1], v246, v244\n\t"            // pR1
      "v_mov_b64_e32 v[240:241], s[84:85]\n\t"
      "v_cndmask_b32_e64 v237, v232, v234, s[92:93]\n\t"   // cv0
      "v_cndmask_b32_e64 v238, v233, v235, s[92:93]\n\t"   // cs0
      "v_bitop3_b32 v239, s92, %[req], %[anc] bitop3:0x28\n\t"
      "v_cmp_lt_f32_e64 s[96:97], s84, v237\n\t"           // gt0
      "v_readfirstlane_b32 s86, v237\n\t"                  // c0: the root's min child
      "v_cmp_eq_u32_e64 s[94:95], 0, v239\n\t"             // onp0
      "v_readfirstlane_b32 s87, v238\n\t"
      "v_bitop3_b32 v248, s92, %[rq1l], %[an1l] bitop3:0x28\n\t"
      "v_bitop3_b32 v249, s93, %[rq1h], %[an1h] bitop3:0x28\n\t"
      "v_or_b32_e32 v248, v248, v249\n\t"
      "v_cndmask_b32_e64 v250, v244, v246, %[p1]\n\t"      // cv1
      "v_cndmask_b32_e64 v251, v245, v247, %[p1]\n\t"      // cs1
      "v_cndmask_b32_e64 v236, %[al], %[ar], s[92:93]\n\t" // group 0's min-child address
      "v_cmp_eq_u32_e64 %[o1], 0, v248\n\t"                // onp1
      "v_cmp_lt_f32_e64 %[g1], s84, v250\n\t"              // gt1
      "v_cndmask_b32_e64 v236, v236, %[aj], s[96:97]\n\t"  // v lands on the stop (gt) or its min child
      "v_cndmask_b32_e64 v253, %[al1], %[ar1], %[p1]\n\t"
      "s_and_b64 s[98:99], s[92:93], %[k63]\n\t"
      "s_or_b64 s[98:99], s[98:99], s[96:97]\n\t"          // cnd0
      "s_bitcmp1_b32 s96, 0\n\t"                           // keep: v stays at the root
      "s_cselect_b32 %[fv], s84, s86\n\t"                  // the new front
      "s_cselect_b32 %[fs], s85, s87\n\t"
      CTCX_BAT_A
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"         // next: s > front
      "v_cndmask_b32_e64 v253, v253, %[aj1], %[g1]\n\t"
      "s_and_b64 s[90:91], s[94:95], s[98:99]\n\t"         // cm0
      "s_cmp_eq_u64 s[90:91], 0\n\t"
      "s_cselect_b64 %[o1], %[o1], 0\n\t"                  // live1: the path's group-1 node, when group 0 has no stop
      "s_ff1_i32_b64 s86, s[90:91]\n\t"                    // the stop (-1: in group 1)
      CTCX_BAT_B
      "s_lshl_b64 s[90:91], -2, s86\n\t"
      "s_andn2_b64 s[94:95], s[94:95], s[90:91]\n\t"       // live0
      "s_andn2_b64 s[90:91], s[94:95], s[96:97]\n\t"       // up0
      "s_and_b64 s[94:95], s[94:95], s[98:99]\n\t"         // stop0 = live0 & cnd0
      "v_cndmask_b32_e64 v239, %[dum], %[aj], s[90:91]\n\t"
      "s_andn2_b64 s[90:91], %[o1], %[g1]\n\t"             // up1
      "v_cndmask_b32_e64 v236, %[dum], v236, s[94:95]\n\t"
      "v_cndmask_b32_e64 v253, %[dum], v253, %[o1]\n\t"    // group 1's stop is its live node
      "v_cndmask_b32_e64 v252, %[dum], %[aj1], s[90:91]\n\t"
      "ds_write2_b32 v239, v237, v238 offset1:1\n\t"
      "ds_write2_b32 v236, v240, v241 offset1:1\n\t"
      "ds_write2_b32 v252, v250, v251 offset1:1\n\t"
      "ds_write2_b32 v253, v240, v241 offset1:1\n\t"
      "ds_read_b128 v[232:235], %[al]\n\t"                 // the next push's child pairs
      "ds_read_b128 v[244:247], %[al] offset:1024\n\t"
      CTCX_BAT_C
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"         // next m
      "s_cbranch_scc0 .Lem_exit_%=\n\t"
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
      "s_cbranch_scc0 .Lem_tail_%=\n\t"                    // the next push, unless k is rare
      "s_branch .Lem_rare_%=\n"
      ".Lem_evb_%=:\n\t"
      "s_mov_b32 s85, %[nfree]\n\t"
      "s_add_u32 %[nfree], %[nfree], 1\n\t"
      "s_mov_b32 m0, %[nv]\n\t"
      "s_add_u32 %[nv], %[nv], 1\n\t"
      "v_writelane_b32 %[evr], %[fs], m0\n\t"
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[c]\n\t"
      "s_and_b64 s[90:91], s[90:91], %[lb]\n\t"
      "s_or_b64 %[rb], %[rb], s[90:91]\n\t"
      "s_branch .Lem_slot_%=\n"
      ".Lem_rare_%=:\n\t"
      "s_mov_b32 %[st], 1\n"
      ".Lem_exit_%=:\n\t"
      "s_not_b64 %[done], s[80:81]\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [my] "+v"(myslot), [evr] "+v"(evr), [bat] "+v"(bat), [nc] "+s"(NC), [rb] "+s"(RB), [done] "+s"(done),
        [fv] "+s"(fv), [fs] "+s"(fs), [nfree] "+s"(nfree), [nv] "+s"(nv), [k] "=&s"(k), [st] "=&s"(st),
        [cnt] "+s"(cnt), [p1] "=&s"(p1), [g1] "=&s"(g1), [o1] "=&s"(o1)
      : [s] "v"(s), [c] "v"(c), [sl] "v"(sl), [anc] "v"(anc), [req] "v"(req), [an1l] "v"(an1l), [an1h] "v"(an1h),
        [rq1l] "v"(rq1l), [rq1h] "v"(rq1h), [aj] "v"(aj), [al] "v"(al), [ar] "v"(ar), [aj1] "v"(aj1),
        [al1] "v"(al1), [ar1] "v"(ar1), [dum] "v"(dum), [lb] "s"(LB), [nb] "s"(nb), [k63] "s"(k63)
      : "memory", "vcc", "m0", "s80", "s81", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93",
        "s94", "s95", "s96", "s97", "s98", "s99", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",
        "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253");
  return st;
}

// The same event loop over one half of a 128-offer window (exact_step's
// window path): the current half's offers are s/c/sl/myslot/bat and its lane
// masks, the other half's appear only in the bookkeeping -- an evicted front
// can be an entry the other half accepted (myo), and while the first half runs
// (OTHER) a branch eviction makes the second half's re-offer of it wanted (rbo)
// and its turns still to start see every new front (bato).  sl is
// window-relative (0..127); hoff is the half's first window position.
#define CTCX_HEV2_ASM(EVB_OTHER, BAT_OTHER, MYO_CMP, MYO_SET)                                                \
  asm volatile(                                                                                              \
      "s_mov_b32 %[st], 0\n\t"                                                                               \
      "s_mov_b32 s99, -1\n\t"                              /* cnd's high word: lanes 32..63 always stop */   \
      "s_not_b64 s[80:81], %[done]\n\t"                     /* lanes still to come */                        \
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"                                                           \
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"                                                              \
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"                                                               \
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"                                                           \
      "s_cbranch_scc0 .Lew_exit_%=\n\t"                                                                      \
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"                                                                     \
      "s_bitcmp1_b64 %[lb], %[k]\n\t"                                                                        \
      "s_cbranch_scc1 .Lew_rare_%=\n\t"                                                                      \
      "ds_read_b128 v[232:235], %[al]\n"                                                                     \
      ".Lew_tail_%=:\n\t"                                                                                    \
      "s_lshl_b64 s[80:81], -2, %[k]\n\t"                   /* lanes after k */                              \
      "v_readlane_b32 s84, %[s], %[k]\n\t"                                                                   \
      "s_mov_b32 s85, %[fs]\n\t"                                                                             \
      "s_cmp_lt_i32 %[fs], %[nb]\n\t"                                                                        \
      "s_cbranch_scc0 .Lew_slot_%=\n\t"                    /* the front is a new child's entry */         \
      /* the evicted front is a branch's entry: a fresh slot, the eviction */                                 \
      /* recorded, a live re-offer of that branch now wanted */                                                \
      "s_mov_b32 s85, %[nfree]\n\t"                                                                          \
      "s_add_u32 %[nfree], %[nfree], 1\n\t"                                                                  \
      "s_mov_b32 m0, %[nv]\n\t"                                                                              \
      "s_add_u32 %[nv], %[nv], 1\n\t"                                                                        \
      "v_writelane_b32 %[evr], %[fs], m0\n\t"                                                                \
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[c]\n\t"                                                           \
      "s_and_b64 s[90:91], s[90:91], %[lb]\n\t"                                                              \
      "s_or_b64 %[rb], %[rb], s[90:91]\n\t" EVB_OTHER                                                        \
      ".Lew_slot_%=:\n\t"                                                                                    \
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[my]\n\t" MYO_CMP                                                  \
      "s_mov_b32 m0, %[k]\n\t"                                                                               \
      "v_cndmask_b32_e64 %[my], %[my], -1, s[90:91]\n\t" MYO_SET                                             \
      "v_writelane_b32 %[my], s85, m0\n\t" CTCX_EVCNT                                                        \
      "s_waitcnt lgkmcnt(0)\n\t"                                                                             \
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"                                                           \
      "v_mov_b64_e32 v[240:241], s[84:85]\n\t"                                                                          \
      "v_cndmask_b32_e64 v237, v232, v234, s[92:93]\n\t"                                                     \
      "v_cndmask_b32_e64 v238, v233, v235, s[92:93]\n\t"                                                     \
      "v_bitop3_b32 v239, s92, %[req], %[anc] bitop3:0x28\n\t"   /* (pickR ^ req) & anc */                 \
      "v_cmp_lt_f32_e64 s[96:97], s84, v237\n\t"                                                             \
      "v_cndmask_b32_e64 v236, %[al], %[ar], s[92:93]\n\t"       /* the min child's address */             \
      "v_readfirstlane_b32 s86, v237\n\t"                                                                    \
      "v_cmp_eq_u32_e64 s[94:95], 0, v239\n\t"                                                               \
      "v_readfirstlane_b32 s87, v238\n\t"                                                                    \
      "v_cndmask_b32_e64 v236, v236, %[aj], s[96:97]\n\t"        /* v lands here if it is the stop */      \
      "s_and_b32 s98, s92, %[k31]\n\t"                                                                       \
      "s_bitcmp1_b32 s96, 0\n\t"                                                                             \
      "s_cselect_b32 %[fv], s84, s86\n\t"                                                                    \
      "s_cselect_b32 %[fs], s85, s87\n\t"                                                                    \
      "s_or_b32 s98, s98, s96\n\t"                         /* cnd: gt, or a min child that is not a lane */  \
      "v_cmp_lt_i32_e64 vcc, %[k], %[sl]\n\t"                                                                \
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"                                                           \
      "s_and_b64 s[90:91], s[94:95], s[98:99]\n\t"                                                           \
      "s_ff1_i32_b64 s86, s[90:91]\n\t"                                                                      \
      "v_mov_b32_e32 v242, %[fv]\n\t"                                                                        \
      "s_lshl_b64 s[90:91], -2, s86\n\t"                                                                     \
      "s_andn2_b64 s[94:95], s[94:95], s[90:91]\n\t"                                                         \
      "s_andn2_b64 s[90:91], s[94:95], s[96:97]\n\t"                                                         \
      "s_lshl_b64 s[94:95], 1, s86\n\t"                                                                      \
      "v_cndmask_b32_e64 v239, %[dum], %[aj], s[90:91]\n\t"                                                  \
      "v_cndmask_b32_e64 v236, %[dum], v236, s[94:95]\n\t"                                                   \
      "ds_write2_b32 v239, v237, v238 offset1:1\n\t"                                                         \
      "ds_write2_b32 v236, v240, v241 offset1:1\n\t"                                                         \
      "ds_read_b128 v[232:235], %[al]\n\t"                                                                   \
      "v_cndmask_b32_e32 %[bat], %[bat], v242, vcc\n\t" BAT_OTHER                                           \
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"                                                              \
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"                                                               \
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"                                                           \
      "s_cbranch_scc0 .Lew_exit_%=\n\t"                                                                      \
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"                                                                     \
      "s_bitcmp1_b64 %[lb], %[k]\n\t"                                                                        \
      "s_cbranch_scc0 .Lew_tail_%=\n\t"                     /* the next push, unless k is rare */            \
      ".Lew_rare_%=:\n\t"                                                                                    \
      "s_mov_b32 %[st], 1\n"                                                                                 \
      ".Lew_exit_%=:\n\t"                                                                                    \
      "s_not_b64 %[done], s[80:81]\n\t"                                                                      \
      "s_waitcnt lgkmcnt(0)"                                                                                 \
      : [my] "+v"(myslot), [myo] "+v"(myo), [evr] "+v"(evr), [bat] "+v"(bat), [bato] "+v"(bato),            \
        [nc] "+s"(NC), [rb] "+s"(RB), [rbo] "+s"(RBo), [done] "+s"(done), [fv] "+s"(fv), [fs] "+s"(fs),     \
        [nfree] "+s"(nfree), [nv] "+s"(nv), [k] "=&s"(k), [st] "=&s"(st), [cnt] "+s"(cnt)                    \
      : [s] "v"(s), [c] "v"(c), [sl] "v"(sl), [co] "v"(co), [slo] "v"(slo), [anc] "v"(anc), [req] "v"(req),  \
        [aj] "v"(aj), [al] "v"(al), [ar] "v"(ar), [dum] "v"(dum), [lb] "s"(LB), [lbo] "s"(LBo), [nb] "s"(nb), \
        [k31] "s"(k31)                                                                                       \
      : "memory", "vcc", "s80", "s81", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93",  \
        "s94", "s95", "s96", "s97", "s98", "s99", "m0", "v232", "v233", "v234", "v235", "v236", "v237",       \
        "v238", "v239", "v240", "v241", "v242", "v243", "v244")

template <bool OTHER>
__device__ __forceinline__ int heap_events2_f32(float s, int c, int sl, int co, int slo, unsigned anc, unsigned req,
                                                unsigned aj, unsigned al, unsigned ar, unsigned dum, int& myslot,
                                                int& myo, int& evr, float& bat, float& bato, uint64_t& NC,
                                                uint64_t& RB, uint64_t& RBo, uint64_t& done, uint64_t LB,
                                                uint64_t LBo, float& fv, int& fs, int& nfree, int& nv, int nb,
                                                int hoff, int& k, int& cnt) {
  int st;
  const unsigned k31 = 0x80000000u;
  // every scalar operand provably uniform (the asm's "s" constraints)
  NC = uni64(NC); RB = uni64(RB); RBo = uni64(RBo); done = uni64(done); LB = uni64(LB); LBo = uni64(LBo);
  fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv); nb = uni(nb); cnt = uni(cnt);
  (void)hoff;   // sl / slo arrive relative to the half (turn start - hoff)
  if constexpr (OTHER)
    CTCX_HEV2_ASM("v_cmp_eq_u32_e64 s[90:91], %[fs], %[co]\n\t"
                  "s_and_b64 s[90:91], s[90:91], %[lbo]\n\t"
                  "s_or_b64 %[rbo], %[rbo], s[90:91]\n\t",
                  "v_cmp_lt_i32_e64 s[86:87], %[k], %[slo]\n\t"
                  "v_mov_b32_e32 v244, %[fv]\n\t"
                  "s_nop 1\n\t"
                  "v_cndmask_b32_e64 %[bato], %[bato], v244, s[86:87]\n\t",
                  "", "");   // the second half has accepted nothing yet: no myo to invalidate
  else
    CTCX_HEV2_ASM("", "", "v_cmp_eq_u32_e64 s[86:87], %[fs], %[myo]\n\t",
                  "v_cndmask_b32_e64 %[myo], %[myo], -1, s[86:87]\n\t");
  return st;
}

// sort_heap for float beams of up to 128 (exact_step's Extract), pops
// pop_heap(len) for len = hi down to lo + 1 as one hand-scheduled asm loop:
// the front goes to position len - 1 -- recorded as lane (len - 1 - base) of
// srt instead of stored, no later sift reads it -- position len - 1 becomes a
// +inf sentinel, and e[len - 1] sifts from the root over len - 1 elements
// (the push_m sift).  Temporaries: s84..s99, v232..v251 (clobbered); DS
// operand registers are rewritten only after the s_waitcnt that retires them.
__device__ __forceinline__ void extract_f32(unsigned heb, int hi, int lo, int base, unsigned anc, unsigned req,
                                            unsigned aj, unsigned al, unsigned ar, unsigned dum, int& srt, int& fs) {
  const unsigned k31 = 0x80000000u;
  // every scalar operand provably uniform (the asm's "s" constraints)
  heb = (unsigned)uni((int)heb); hi = uni(hi); lo = uni(lo); base = uni(base); fs = uni(fs);
  asm volatile(
      "s_mov_b32 s84, %[hi]\n\t"
      "s_cmp_le_i32 s84, %[lo]\n\t"
      "s_cbranch_scc1 .Lx_end_%=\n\t"
      "s_mov_b64 s[90:91], 1\n\t"                          // lane 0
      "s_mov_b32 s99, -1\n\t"                              // cnd's high word: lanes 32..63 always stop
      "v_mov_b32_e32 v242, 0x7f800000\n\t"                 // the sentinel (+inf, -1)
      "v_mov_b32_e32 v243, -1\n\t"
      "s_lshl_b32 s85, s84, 3\n\t"
      "s_add_u32 s85, s85, %[heb]\n\t"
      "v_mov_b32_e32 v236, s85\n\t"                        // he[len]: position len - 1 (-8 B per pop)
      "s_sub_u32 s86, s84, 1\n\t"
      "s_sub_u32 m0, s86, %[base]\n"                       // its lane in srt (-1 per pop)
      ".Lx_top_%=:\n\t"
      "ds_read_b64 v[238:239], v236\n\t"                   // e[len - 1] (every lane: broadcast)
      "v_cndmask_b32_e64 v241, %[dum], v236, s[90:91]\n\t"
      "v_writelane_b32 %[srt], %[fs], m0\n\t"              // the front: position len - 1
      "ds_write_b64 v241, v[242:243]\n\t"                  // lane 0: the sentinel
      "ds_read_b128 v[232:235], %[al]\n\t"                 // child pairs
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         // pickR
      "v_readfirstlane_b32 s87, v239\n\t"                  // v's slot
      "v_subrev_u32_e32 v236, 8, v236\n\t"
      "v_cndmask_b32_e64 v248, v232, v234, s[92:93]\n\t"   // cv
      "v_cndmask_b32_e64 v249, v233, v235, s[92:93]\n\t"   // cs
      "v_bitop3_b32 v251, s92, %[req], %[anc] bitop3:0x28\n\t"
      "v_cmp_lt_f32_e64 s[96:97], v238, v248\n\t"          // gt: min child > v
      "v_cndmask_b32_e64 v250, %[al], %[ar], s[92:93]\n\t" // the min child's address
      "v_readfirstlane_b32 s86, v249\n\t"                  // s0
      "v_cmp_eq_u32_e64 s[94:95], 0, v251\n\t"             // onp
      "v_cndmask_b32_e64 v250, v250, %[aj], s[96:97]\n\t"  // v lands here if it is the stop
      "s_and_b32 s98, s92, %[k31]\n\t"
      "s_or_b32 s98, s98, s96\n\t"                         // cnd (low word)
      "s_and_b64 s[88:89], s[94:95], s[98:99]\n\t"         // cm
      "s_ff1_i32_b64 s88, s[88:89]\n\t"                    // the stop
      "s_lshl_b64 s[88:89], -2, s88\n\t"
      "s_andn2_b64 s[94:95], s[94:95], s[88:89]\n\t"       // live
      "s_andn2_b64 s[88:89], s[94:95], s[96:97]\n\t"       // up
      "s_and_b64 s[80:81], s[94:95], s[98:99]\n\t"         // the stop
      "v_cndmask_b32_e64 v247, %[dum], %[aj], s[88:89]\n\t"
      "v_cndmask_b32_e64 v250, %[dum], v250, s[80:81]\n\t"
      "ds_write2_b32 v247, v248, v249 offset1:1\n\t"
      "ds_write2_b32 v250, v238, v239 offset1:1\n\t"
      "s_bitcmp1_b32 s96, 0\n\t"                           // keep: v stays at the root
      "s_cselect_b32 %[fs], s87, s86\n\t"
      "s_sub_u32 s84, s84, 1\n\t"
      "s_sub_u32 m0, m0, 1\n\t"
      "s_cmp_gt_i32 s84, %[lo]\n\t"
      "s_cbranch_scc1 .Lx_top_%=\n"
      ".Lx_end_%=:\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [srt] "+v"(srt), [fs] "+s"(fs)
      : [heb] "s"(heb), [hi] "s"(hi), [lo] "s"(lo), [base] "s"(base), [anc] "v"(anc), [req] "v"(req), [aj] "v"(aj),
        [al] "v"(al), [ar] "v"(ar), [dum] "v"(dum), [k31] "s"(k31)
      : "memory", "m0", "s80", "s81", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94",
        "s95", "s96", "s97", "s98", "s99", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240",
        "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251");
}

// extract_f32 with the heap in registers for the whole call (beams up to 128;
// the two-node kernels keep extract_f32).  extract_f32 ends every pop with two
// node stores and begins the next with a read of the same lines and a wait for
// it (~99 cycles on the serial chain), yet every value that read returns was
// in some lane's registers before the stores went out, and nothing else reads
// `he` while wave 0 pops (the helper ranks a copy).  Here P = v[232:235] holds
// lane j's child pair (L.v, L.s, R.v, R.s): read from `he` once at entry,
// carried from pop to pop, written back once at exit with the root, so `he`
// is what extract_f32 leaves at every call boundary (dummy slots aside).
// One pop:
//   * e[len - 1] is a child of lane (len - 2) / 2: two v_readlane of P (the
//     loop is unrolled by two, the side is the parity of len), and that lane's
//     entry becomes the sentinel;
//   * every lane publishes what its node holds after the sift if the path
//     reaches it: v where its min child is > v (gt: v lands there), else its
//     min child (it moves up) -- lane 0's pair is the new root: the front --
//     and then lane 0, whose node is nobody's child, publishes v;
//   * every lane fetches the published pair of its min child's lane (two
//     ds_bpermute: no LDS) -- lanes whose min child is not a lane (lanes
//     32..63, lane 31 on the right) fetch lane 0's, v;
//   * the lanes that take their min child (up: on the root's min-child path,
//     no proper ancestor meeting the stop condition, no gt) put the fetched
//     pair in P on the min child's side: the child moved up, or v landed
//     there.  Nothing else changes: a child on the path has its parent on it.
//     Without the stores nothing needs the stop's lane, so up is a per-lane
//     test against the stop-condition mask (ancestors of a lane are below 32:
//     its low word), not a scalar s_ff1 chain.
// The fetch goes out as soon as gt is known and its latency overlaps the rest
// of the mask algebra.  tests/test_cpu_heap_forward.py is this rule on the
// host against libstdc++; tools/heap_fwd_unit.hip runs both loops on the GPU.
// Temporaries: s80..s81, s85..s95, s98, vcc, m0, v232..v251 (clobbered).
#define CTCX_XFWD_POP(XV, XS, NEXTLANE)                                                                     \
      "s_lshl_b64 s[80:81], 1, s90\n\t"                    /* the lane e[len - 1] is a child of */         \
      "v_readlane_b32 s86, " XV ", s90\n\t"                /* v = e[len - 1] */                            \
      "v_readlane_b32 s87, " XS ", s90\n\t"                                                                  \
      "v_cndmask_b32_e64 " XV ", " XV ", v242, s[80:81]\n\t" /* vacated: the sentinel */                   \
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         /* pickR = !(R > L) */                          \
      "v_cndmask_b32_e64 " XS ", " XS ", v243, s[80:81]\n\t"                                                 \
      "v_writelane_b32 %[srt], %[fs], m0\n\t"              /* the front: position len - 1 */               \
      "v_mov_b64_e32 v[238:239], s[86:87]\n\t"                                                               \
      "v_cndmask_b32_e64 v248, v232, v234, s[92:93]\n\t"   /* cv */                                        \
      "v_cmp_lt_f32_e32 vcc, s86, v248\n\t"                /* gt: min child > v */                         \
      "v_cndmask_b32_e64 v249, v233, v235, s[92:93]\n\t"   /* cs */                                        \
      "v_cndmask_b32_e64 v237, v246, v247, s[92:93]\n\t"   /* the min child's lane (x 4) */                \
      "v_cndmask_b32_e32 v240, v248, v238, vcc\n\t"        /* published: v (gt) or the min child */        \
      "v_cndmask_b32_e32 v241, v249, v239, vcc\n\t"                                                          \
      "s_and_b32 s98, s92, %[k31]\n\t"                                                                       \
      "v_bitop3_b32 v244, s92, %[req], %[anc] bitop3:0x28\n\t"  /* (pickR ^ req) & anc */                  \
      "v_readfirstlane_b32 %[fs], v241\n\t"                /* the root's: the new front */                 \
      "v_writelane_b32 v240, s86, 0\n\t"                   /* lane 0 publishes v */                        \
      "v_writelane_b32 v241, s87, 0\n\t"                                                                     \
      "s_or_b32 s98, s98, vcc_lo\n\t"                      /* the stop condition, lanes 0..31 */           \
      "ds_bpermute_b32 v250, v237, v240\n\t"               /* the min child's published pair */            \
      "ds_bpermute_b32 v251, v237, v241\n\t"                                                                 \
      "v_and_or_b32 v245, s98, %[anc], v244\n\t"           /* off the path, or below the stop */           \
      "s_sub_u32 m0, m0, 1\n\t" NEXTLANE                                                                     \
      "v_cmp_eq_u32_e64 s[94:95], 0, v245\n\t"             /* live: path nodes at or above the stop */     \
      "s_andn2_b64 s[94:95], s[94:95], vcc\n\t"            /* up: takes its min child */                   \
      "s_and_b64 s[80:81], s[94:95], s[92:93]\n\t"         /* ... the right one */                         \
      "s_andn2_b64 s[88:89], s[94:95], s[92:93]\n\t"       /* ... the left one */                          \
      "s_waitcnt lgkmcnt(0)\n\t"                                                                             \
      "v_cndmask_b32_e64 v232, v232, v250, s[88:89]\n\t"                                                     \
      "v_cndmask_b32_e64 v233, v233, v251, s[88:89]\n\t"                                                     \
      "v_cndmask_b32_e64 v234, v234, v250, s[80:81]\n\t"                                                     \
      "v_cndmask_b32_e64 v235, v235, v251, s[80:81]\n\t"                                                     \
      "s_cmp_ge_i32 m0, s85\n\t"
__device__ __forceinline__ void extract_fwd_f32(unsigned heb, int hi, int lo, int base, unsigned anc, unsigned req,
                                                unsigned aj, unsigned al, unsigned dum, int& srt, int& fs) {
  const unsigned k31 = 0x80000000u;
  // every scalar operand provably uniform (the asm's "s" constraints)
  heb = (unsigned)uni((int)heb); hi = uni(hi); lo = uni(lo); base = uni(base); fs = uni(fs);
  asm volatile(
      "s_cmp_le_i32 %[hi], %[lo]\n\t"
      "s_cbranch_scc1 .Lxf_end_%=\n\t"
      "ds_read_b128 v[232:235], %[al]\n\t"                 // P: the child pairs
      "v_mov_b32_e32 v242, 0x7f800000\n\t"                 // the sentinel (+inf, -1)
      "v_mov_b32_e32 v243, -1\n\t"
      "s_sub_u32 s86, %[hi], 1\n\t"
      "s_sub_u32 m0, s86, %[base]\n\t"                     // position len - 1's lane in srt (-1 per pop)
      "s_sub_u32 s85, %[lo], %[base]\n\t"                  // the last pop's
      "s_sub_u32 s90, %[hi], 2\n\t"
      "s_lshr_b32 s90, s90, 1\n\t"                         // the lane position len - 1 is a child of (-1 per two pops)
      // the lane (x 4) a fetch reads: the left and the right child's, lane 0
      // where the child is not a lane
      "v_sub_u32_e32 v247, %[al], %[aj]\n\t"               // 8 * lane + 8
      "s_mov_b32 s80, 0x7fffffff\n\t"
      "s_mov_b32 s81, 0\n\t"
      "v_add_u32_e32 v246, -4, v247\n\t"
      "v_cndmask_b32_e64 v247, 0, v247, s[80:81]\n\t"      // right: lanes 0..30
      "s_mov_b32 s80, -1\n\t"
      "v_cndmask_b32_e64 v246, 0, v246, s[80:81]\n\t"      // left: lanes 0..31
      "s_bitcmp1_b32 %[hi], 0\n\t"                         // len odd: e[len - 1] is a right child
      "s_waitcnt lgkmcnt(0)\n\t"
      "s_cbranch_scc0 .Lxf_odd_%=\n"
      ".Lxf_even_%=:\n\t"
      CTCX_XFWD_POP("v234", "v235", "")
      "s_cbranch_scc0 .Lxf_done_%=\n"
      ".Lxf_odd_%=:\n\t"
      CTCX_XFWD_POP("v232", "v233", "s_sub_u32 s90, s90, 1\n\t")
      "s_cbranch_scc1 .Lxf_even_%=\n"
      // back to he: the pairs, and the root (v if it stayed there, else its min child)
      ".Lxf_done_%=:\n\t"
      "v_readfirstlane_b32 s91, v248\n\t"
      "v_mov_b32_e32 v236, %[dum]\n\t"
      "s_add_u32 s88, %[heb], 8\n\t"
      "s_bitcmp1_b32 vcc_lo, 0\n\t"                        // keep: v stayed at the root
      "s_cselect_b32 s86, s86, s91\n\t"
      "v_mov_b32_e32 v239, %[fs]\n\t"
      "v_writelane_b32 v236, s88, 0\n\t"                   // lane 0: the root (the others: dummies)
      "v_mov_b32_e32 v238, s86\n\t"
      "ds_write_b128 %[al], v[232:235]\n\t"
      "ds_write_b64 v236, v[238:239]\n"
      ".Lxf_end_%=:\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [srt] "+v"(srt), [fs] "+s"(fs)
      : [heb] "s"(heb), [hi] "s"(hi), [lo] "s"(lo), [base] "s"(base), [anc] "v"(anc), [req] "v"(req), [aj] "v"(aj),
        [al] "v"(al), [dum] "v"(dum), [k31] "s"(k31)
      : "memory", "vcc", "m0", "s80", "s81", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94",
        "s95", "s98", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243",
        "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251");
}

// extract_f32 over the two-group heap (beams 129..256: the push_m2 sift), for
// pops that leave more than 128 elements (len > 129); below that the heap
// fits the one-group form and extract_f32 takes over on the same layout (the
// vacated positions up to 256 hold sentinels).  Group 1's pick, path test
// (against group 0's pick mask), gt and stores as in heap_events_m2_f32.
// Temporaries: s84..s99, v232..v255 (clobbered) and compiler-chosen registers
// (p1, g1, o1: SGPR pairs; t0, t1, c1v, c1s, a1, u1: VGPRs, the last four DS
// operands, rewritten only after the s_waitcnt that retires them).
__device__ __forceinline__ void extract_m2_f32(unsigned heb, int hi, int lo, int base, unsigned anc, unsigned req,
                                               unsigned an1l, unsigned an1h, unsigned rq1l, unsigned rq1h,
                                               unsigned aj, unsigned al, unsigned ar, unsigned aj1, unsigned al1,
                                               unsigned ar1, unsigned dum, int& srt, int& fs) {
  const uint64_t k63 = 0x8000000000000000ull;
  uint64_t p1, g1, o1;
  unsigned t0, t1, c1v, c1s, a1, u1;
  heb = (unsigned)uni((int)heb); hi = uni(hi); lo = uni(lo); base = uni(base); fs = uni(fs);
  asm volatile(
      "s_mov_b32 s84, %[hi]\n\t"
      "s_cmp_le_i32 s84, %[lo]\n\t"
      "s_cbranch_scc1 .Ly_end_%=\n\t"
      "s_mov_b64 s[90:91], 1\n\t"                          // lane 0
      "v_mov_b32_e32 v242, 0x7f800000\n\t"                 // the sentinel (+inf, -1)
      "v_mov_b32_e32 v243, -1\n\t"
      "s_lshl_b32 s85, s84, 3\n\t"
      "s_add_u32 s85, s85, %[heb]\n\t"
      "v_mov_b32_e32 v236, s85\n\t"                        // he[len]: position len - 1 (-8 B per pop)
      "s_sub_u32 s86, s84, 1\n\t"
      "s_sub_u32 m0, s86, %[base]\n"                       // its lane in srt (-1 per pop)
      ".Ly_top_%=:\n\t"
      "ds_read_b64 v[238:239], v236\n\t"                   // e[len - 1] (every lane: broadcast)
      "v_cndmask_b32_e64 v241, %[dum], v236, s[90:91]\n\t"
      "v_writelane_b32 %[srt], %[fs], m0\n\t"              // the front: position len - 1
      "ds_write_b64 v241, v[242:243]\n\t"                  // lane 0: the sentinel
      "ds_read_b128 v[232:235], %[al]\n\t"                 // group 0 child pairs
      "ds_read_b128 v[252:255], %[al] offset:1024\n\t"     // group 1 child pairs
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         // pR0
      "v_cmp_ngt_f32_e64 %[p1], v254, v252\n\t"            // pR1
      "v_readfirstlane_b32 s87, v239\n\t"                  // v's slot
      "v_subrev_u32_e32 v236, 8, v236\n\t"
      "v_cndmask_b32_e64 v248, v232, v234, s[92:93]\n\t"   // cv0
      "v_cndmask_b32_e64 v249, v233, v235, s[92:93]\n\t"   // cs0
      "v_bitop3_b32 v251, s92, %[req], %[anc] bitop3:0x28\n\t"
      "v_cmp_lt_f32_e64 s[96:97], v238, v248\n\t"          // gt0: min child > v
      "v_cndmask_b32_e64 v250, %[al], %[ar], s[92:93]\n\t" // group 0's min-child address
      "v_cmp_eq_u32_e64 s[94:95], 0, v251\n\t"             // onp0
      "v_readfirstlane_b32 s86, v249\n\t"                  // s0
      "v_bitop3_b32 %[t0], s92, %[rq1l], %[an1l] bitop3:0x28\n\t"
      "v_bitop3_b32 %[t1], s93, %[rq1h], %[an1h] bitop3:0x28\n\t"
      "v_cndmask_b32_e64 v250, v250, %[aj], s[96:97]\n\t"
      "v_or_b32_e32 %[t0], %[t0], %[t1]\n\t"
      "v_cndmask_b32_e64 %[c1v], v252, v254, %[p1]\n\t"    // cv1
      "v_cndmask_b32_e64 %[c1s], v253, v255, %[p1]\n\t"    // cs1
      "v_cndmask_b32_e64 %[a1], %[al1], %[ar1], %[p1]\n\t"
      "v_cmp_eq_u32_e64 %[o1], 0, %[t0]\n\t"               // onp1
      "v_cmp_lt_f32_e64 %[g1], v238, %[c1v]\n\t"           // gt1
      "s_and_b64 s[98:99], s[92:93], %[k63]\n\t"
      "s_or_b64 s[98:99], s[98:99], s[96:97]\n\t"          // cnd0
      "s_and_b64 s[88:89], s[94:95], s[98:99]\n\t"         // cm0
      "s_cmp_eq_u64 s[88:89], 0\n\t"
      "s_cselect_b64 %[o1], %[o1], 0\n\t"                  // live1
      "s_ff1_i32_b64 s88, s[88:89]\n\t"                    // the stop (-1: in group 1)
      "v_cndmask_b32_e64 %[a1], %[a1], %[aj1], %[g1]\n\t"
      "s_lshl_b64 s[88:89], -2, s88\n\t"
      "s_andn2_b64 s[94:95], s[94:95], s[88:89]\n\t"       // live0
      "s_andn2_b64 s[88:89], s[94:95], s[96:97]\n\t"       // up0
      "s_and_b64 s[98:99], s[94:95], s[98:99]\n\t"         // stop0 = live0 & cnd0
      "v_cndmask_b32_e64 v247, %[dum], %[aj], s[88:89]\n\t"
      "s_andn2_b64 s[88:89], %[o1], %[g1]\n\t"             // up1
      "v_cndmask_b32_e64 v250, %[dum], v250, s[98:99]\n\t"
      "v_cndmask_b32_e64 %[a1], %[dum], %[a1], %[o1]\n\t"  // group 1's stop is its live node
      "v_cndmask_b32_e64 %[u1], %[dum], %[aj1], s[88:89]\n\t"
      "ds_write2_b32 v247, v248, v249 offset1:1\n\t"
      "ds_write2_b32 v250, v238, v239 offset1:1\n\t"
      "ds_write2_b32 %[u1], %[c1v], %[c1s] offset1:1\n\t"
      "ds_write2_b32 %[a1], v238, v239 offset1:1\n\t"
      "s_bitcmp1_b32 s96, 0\n\t"                           // keep: v stays at the root
      "s_cselect_b32 %[fs], s87, s86\n\t"
      "s_sub_u32 s84, s84, 1\n\t"
      "s_sub_u32 m0, m0, 1\n\t"
      "s_cmp_gt_i32 s84, %[lo]\n\t"
      "s_cbranch_scc1 .Ly_top_%=\n"
      ".Ly_end_%=:\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [srt] "+v"(srt), [fs] "+s"(fs), [p1] "=&s"(p1), [g1] "=&s"(g1), [o1] "=&s"(o1), [t0] "=&v"(t0),
        [t1] "=&v"(t1), [c1v] "=&v"(c1v), [c1s] "=&v"(c1s), [a1] "=&v"(a1), [u1] "=&v"(u1)
      : [heb] "s"(heb), [hi] "s"(hi), [lo] "s"(lo), [base] "s"(base), [anc] "v"(anc), [req] "v"(req),
        [an1l] "v"(an1l), [an1h] "v"(an1h), [rq1l] "v"(rq1l), [rq1h] "v"(rq1h), [aj] "v"(aj), [al] "v"(al),
        [ar] "v"(ar), [aj1] "v"(aj1), [al1] "v"(al1), [ar1] "v"(ar1), [dum] "v"(dum), [k63] "s"(k63)
      : "memory", "m0", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97",
        "s98", "s99", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242",
        "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255");
}

// peek_bottom() in the UNORDERED state: the first minimum moves to the front.
// Returns the new front.
template <typename T>
__device__ HE<T> wave_first_min_to_front(CTCX_LDS HE<T>* he, int n) {
  const int lane = threadIdx.x;
  T mv = pinf<T>();
  int mi = 0x7fffffff, ms = 0;
  for (int i = lane; i < n; i += 64) {
    const HE<T> e = he_ld(he, i + 1);
    if (e.v < mv) { mv = e.v; mi = i; ms = e.s; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const T ov = __shfl_xor(mv, o);
    const int oi = __shfl_xor(mi, o);
    const int os = __shfl_xor(ms, o);
    if (ov < mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; ms = os; }
  }
  mi = uni(mi);
  if (mi != 0 && lane == 0) {
    const HE<T> a = he_ld(he, 1);
    he_st(he, 1, he_ld(he, mi + 1));
    he_st(he, mi + 1, a);
  }
  HE<T> f;
  f.v = uni(mv);
  f.s = uni(ms);
  return f;
}

// ---------------------------------------------------------------------------
// EXACT fast path for one frame (whole wave): the reference's Step with its
// TopN replayed operation for operation (so ties resolve as in the
// reference), offers scored and filtered in parallel.  Returns 0 on success,
// else the reason the frame goes to literal_step: 1 = a non-finite logit or
// total, 2 = the beam fills up in the middle of the grow loop (the reference
// then peeks lazily; rare: only while the beam is still filling).
// On success cx.sorted[0..*n_out) holds the Extract() order and, for the last
// frame, cx.tops[0..min(P, leaves)) the TopPaths() selection as positions.
// Large C: move the child bitmap and its window summary from branch ob's
// children to branch nb_'s (-1: none).  The children of a branch are the
// branches whose parent it is (the child list head/sib is built from par);
// every erase is issued before any record (one wave: LDS keeps that order).
template <typename T>
__device__ __forceinline__ void cq_children(const Ctx<T>& cx, int buf, int nb, int ob, int nb_) {
  CTCX_LDS uint64_t* cbm = row_cbm(cx);
  CTCX_LDS uint64_t* cwin = cbm + (cx.C - 1 + 63) / 64;
  if (ob >= 0) {
    for (int k = (int)(threadIdx.x & 63); k < nb; k += 64) {   // (also run by the two-wave kernels' helper)
      const int pk = sel(cx.par, buf)[k];
      const int lk = sel(cx.lab, buf)[k];
      if (pk == ob) {
        const int x = lk - (lk > cx.blank ? 1 : 0);
        cbm[x >> 6] = 0ull;
        cwin[x >> 12] = 0ull;
      }
    }
  }
  if (nb_ >= 0) {
    for (int k = (int)(threadIdx.x & 63); k < nb; k += 64) {
      const int pk = sel(cx.par, buf)[k];
      const int lk = sel(cx.lab, buf)[k];
      if (pk == nb_) {
        const int x = lk - (lk > cx.blank ? 1 : 0);
        __hip_atomic_fetch_or(&cbm[x >> 6], 1ull << (x & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_or(&cwin[x >> 12], 1ull << ((x >> 6) & 63), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
}
constexpr int kGatherWin = 8;   // kept 64-label windows per batch of row reads in the gather

// ---------------------------------------------------------------------------
// Helper wave (HW kernels: float, beams <= 128, C <= 64, the base scorer).
// The decode workgroup has two waves on two SIMDs of the CU.  Wave 0 decodes
// (the TopN pushes and the sort_heap extract: the frame's dependent chain);
// wave 1 takes the frame's order-independent work off it:
//   * the roll, the recursion and the commit are split over both waves;
//   * during the grow, wave 1 scores the frame's offers ahead of wave 0 into
//     a ring of chunk slots in LDS (the score table): chunk c holds offers
//     [64c, 64c + 64) in (branch, label index) order, per lane its score, its
//     branch's total, the packed (branch, label, label index, branch child),
//     and the child's label-ending alignment candidate (value, back-pointer).
//     All of it depends only on the frame-start state (branch arrays, child
//     lists, the row), which nothing changes during the grow.  What events
//     change -- a branch deactivated, a branch child evicted -- wave 0 reads
//     itself (bst) when it takes a window's two chunks.
// Hand-over: wave 1 publishes its chunk count (hready, a release store after
// the slot's writes), wave 0 its consumed count (dcons, after the slot's
// reads are issued: one wave's LDS operations execute in order) and, when the
// grow ends, gdone; a full ring or an unpublished chunk is waited out with
// s_sleep.  Every wait is bounded (a bound hit never happens in a correct run;
// it ends the wait instead of hanging the CU).
// A barrier for code only wave 0 runs in HW kernels (one wave: its LDS
// operations execute in order, so a compiler fence is enough), else the
// workgroup barrier.
// Two-wave kernels: which wave this is, as a wave-UNIFORM value (the
// compiler cannot know that threadIdx.x >= 64 is uniform per wave).  Every
// split between the decoding wave and the helper goes through it: a branch on
// threadIdx.x is compiled as divergent control flow (both sides in one
// sequence under exec masks); a uniform branch gives each wave its own scalar
// path (cfg3 decode 149.4 -> 147.3 ms with the score table, same box).
__device__ __forceinline__ bool helper_wave() { return __builtin_amdgcn_readfirstlane((int)threadIdx.x) >= 64; }
template <bool HW>
__device__ __forceinline__ void wsync() {
  if constexpr (HW) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}
#ifndef CTCX_TAB_SLOTS
#define CTCX_TAB_SLOTS 16
#endif
#ifndef CTCX_SLEEP
#define CTCX_SLEEP 1
#endif
constexpr int kTabSlots = CTCX_TAB_SLOTS;   // chunk slots in the ring
// A hand-over wait gives up after ~1 s of the constant 100 MHz clock
// (s_memrealtime), whatever the shader clock or the SIMD's other work: only a
// real deadlock reaches it (a frame's whole chain is ~100 us).  The clock is
// first read after 256 rounds (the common short waits never touch it), then
// every 256 rounds.
#ifndef CTCX_WAIT_TICKS
#define CTCX_WAIT_TICKS 100000000ull
#endif
__device__ __forceinline__ bool wait_expired(int spin, uint64_t& t0) {
  if ((spin & 255) != 255) return false;
  const uint64_t now = __builtin_amdgcn_s_memrealtime();
  if (spin == 255) t0 = now;
  return now - t0 > (uint64_t)(CTCX_WAIT_TICKS);
}
struct Tab {
  CTCX_LDS u32x4* a;    // [slot][lane]: score, branch total, packed, candidate back-pointer
  CTCX_LDS float* p;    // [slot][lane]: candidate value
};
__host__ __device__ inline size_t tab_lds_bytes() { return (size_t)kTabSlots * 64 * 20; }
__device__ __forceinline__ Tab tab_carve(CTCX_LDS char* p) {
  Tab t;
  t.a = (CTCX_LDS u32x4*)p;
  t.p = (CTCX_LDS float*)(p + (size_t)kTabSlots * 64 * 16);
  return t;
}
// Per-phase cycle counters of the diagnostics build (CTCX_PHASES), one set per
// item in HBM: wave 0's lane 0 adds each sample with a global atomic that
// returns nothing (the wave never waits on it), so the counters cost the
// decode no registers across its loops (round 5 kept 24 of them in SGPR
// pairs, which moved the hot loops' register allocation and inflated the
// "glue" they measured).  A null pointer compiles every use away.
struct PhaseCtr {
  uint64_t* p;
  struct Ref {
    uint64_t* a;
    __device__ __forceinline__ void operator+=(uint64_t v) const {
      if (threadIdx.x == 0) __hip_atomic_fetch_add(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void operator=(uint64_t v) const {
      if (threadIdx.x == 0) __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  __device__ __forceinline__ explicit operator bool() const { return p != nullptr; }
  __device__ __forceinline__ Ref operator[](int i) const { return Ref{p + i}; }
};

// control words in misc[8..11]; kCtlDead (sticky for the kernel): a wait ran
// out of time, every later wait returns at once, wave 0 ends every grow
// without reading the table or queue, and the item reports it (ItemOut.pad)
constexpr int kCtlReady = 8, kCtlCons = 9, kCtlDone = 10, kCtlDead = 11;
__device__ __forceinline__ int ctl_ld(CTCX_LDS int* m, int k) {
  return uni(__hip_atomic_load(&m[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// packed: branch (bits 0-6), label (7-12), label index (13-18), branch child + 1 (19-26), valid (27)
__device__ __forceinline__ unsigned tab_pack(int i, int l, int li, int cw, bool v) {
  return (unsigned)i | ((unsigned)l << 7) | ((unsigned)li << 13) | ((unsigned)(cw + 1) << 19) | (v ? 1u << 27 : 0u);
}

template <typename T>
__device__ __forceinline__ void help_score_chunks(const Ctx<T>& cx, Tab tb, int buf, int nb, T norm) {
  static_assert(sizeof(T) == 4, "the score table holds float rows");
  const int lane = threadIdx.x & 63;
  const T NI = ninf<T>();
  const int Cm1 = cx.C - 1, blank = cx.blank;
  const float rcp = 1.0f / (float)Cm1;
  const int nch = (nb * Cm1 + 63) >> 6;
  CTCX_LDS int* m = cx.misc;
  if (ctl_ld(m, kCtlDead) != 0) return;
  for (int c = 0; c < nch; ++c) {
    uint64_t tw = 0;
    for (int spin = 0;; ++spin) {   // the grow still running, and a free slot
      if (ctl_ld(m, kCtlDone) != 0) return;
      if (wait_expired(spin, tw)) {
        __hip_atomic_store(&m[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
      }
      const int cons = ctl_ld(m, kCtlCons);
      c = c > cons ? c : cons;   // chunks wave 0 has passed are never read
      if (c < cons + kTabSlots) break;
      __builtin_amdgcn_s_sleep(CTCX_SLEEP);
    }
    if (c >= nch) return;
    const int o = 64 * c + lane;
    int q = (int)((float)o * rcp);
    q -= (q * Cm1 > o) ? 1 : 0;
    q += ((q + 1) * Cm1 <= o) ? 1 : 0;
    const bool v = q < nb;
    const int i = v ? q : 0;
    const int li = v ? o - q * Cm1 : 0;
    const int l = li + (li >= blank ? 1 : 0);
    const int bl = sel(cx.lab, buf)[i];
    const int bflg = sel(cx.flg, buf)[i];
    const T bt = sel(cx.ot, buf)[i];
    const T bob = sel(cx.ob, buf)[i];
    const int hd = cx.head[i];
    const T bcb = sel(cx.cb, buf)[i], bcn = sel(cx.cn, buf)[i];
    const T xl = cx.row[l];
    const T p = xl - norm;
    const T sc = p + ((l == bl) ? bob : bt);
    // the branch child the offer re-offers (GetChild finds it), if any
    int cw = -1;
    for (int k = v ? hd : -1; __ballot(k >= 0);) {
      int nk = -1;
      if (k >= 0) {
        const int lk = sel(cx.lab, buf)[k];
        const int sk = cx.sib[k];
        if (lk == l) cw = k;
        else nk = sk;
      }
      k = nk;
    }
    const bool recv_fresh = cw >= 0 ? (sel(cx.ot, buf)[cw] == NI) : true;
    const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
    Best<T> cd{T(0), kBpNone, false};
    cd.push(((bflg & F_HB) ? bcb : rs_blank) + p, (bflg & F_HB) ? (((uint32_t)i << 1) | 0u) : kBpRestart);
    if (l != bl) cd.push(((bflg & F_HN) ? bcn : NI) + p, (bflg & F_HN) ? (((uint32_t)i << 1) | 1u) : kBpRestart);
    const int slot = (c % kTabSlots) * 64 + lane;
    u32x4 e;
    e.x = __builtin_bit_cast(unsigned, (float)sc);
    e.y = __builtin_bit_cast(unsigned, (float)bt);
    e.z = tab_pack(i, l, li, cw, v);
    e.w = cd.bp;
    tb.a[slot] = e;
    tb.p[slot] = (float)cd.p;
    __hip_atomic_store(&m[kCtlReady], c + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// large C, the beam full: one compacted chunk.  The offers of the span from
// (i0, li0) on that can have an effect are gathered, in offer order, into cq
// (up to 64): a new child whose score can beat the bottom ((x_l - norm) + ot
// > bottom bounds the score; bottom only rises, so an offer failing it now
// fails at its turn too) and every re-offer of a branch child (evicted now,
// or by an event of this chunk before it).  The rest of the span is rejected
// by the reference without effect.  Branch turns are checked here at the
// given bottom (closed now: closed at its turn, the grow ends after this
// chunk: gstop) and again in the chunk at the bottom its turn sees (sl, bat).
// Any bottom at or below the true one gives a correct chunk (a superset of
// the offers that can have an effect): the two-wave kernels' helper gathers
// with the last bottom wave 0 published.  cbr: the branch whose children the
// child bitmap holds (row_cbm), kept across chunks.
template <typename T>
__device__ __forceinline__ void gather_chunk(const Ctx<T>& cx, int buf, int nb, T norm, T pmax, T bottom, int tsn,
                                             T txo, int& i0, int& li0, int& cbr, bool& gstop,
                                             CTCX_LDS uint32_t* cq, int& cqn, PhaseCtr pc, int cap = 64) {
  const int lane = threadIdx.x & 63;
  const T NI = ninf<T>();
  const int Cm1 = cx.C - 1;
  const int blank = cx.blank;
  [[maybe_unused]] CTCX_LDS T* bmax = row_bmax(cx);
    CTCX_LDS uint64_t* cbm = row_cbm(cx);
    CTCX_LDS uint64_t* cwin = cbm + (Cm1 + 63) / 64;
    cqn = 0;
    // the branch scan (lane j: branch sb + j) and a branch's window scan
    // (lane w: window wa0 + w) hold for the whole gather: no event moves the
    // bottom before the chunk runs
    int sb = -1, wa0 = -1;
    uint64_t hitM = 0, brkM = 0, chM = 0, wkM = 0;
    T otb = NI, ot0 = NI;
    bool enter = true;   // at the gather's start or a branch's first offer
    const uint64_t tg0 = pc ? __builtin_amdgcn_s_memtime() : 0;
    const T tsx = lane < tsn ? (T)row_topx(cx)[lane] : NI;                          // S in label-index order:
    const int tsl = lane < tsn ? ((CTCX_LDS int*)(row_topx(cx) + kTopK))[lane] : Cm1;   // lane j its j-th
    while (cqn < cap) {
      const uint64_t te0 = pc ? __builtin_amdgcn_s_memtime() : 0;
      if (enter) {
        // the next branch with a turn closed (stop), or with something to
        // gather (pmax + ot > bottom, or children)
        int res = 0;   // 0: at a branch to gather from, 1: a turn is closed, 2: past the last branch
        for (;;) {
          if (sb < 0 || i0 >= sb + 64) {
            sb = i0;
            const int ib = i0 + lane;
            bool brk = false, skp = true, ch = false;
            otb = NI;
            if (ib < nb) {
              otb = sel(cx.ot, buf)[ib];
              ch = cx.head[ib] >= 0;
              brk = (lane > 0 || li0 == 0) && !(otb > bottom);
              skp = !(pmax + otb > bottom) && !ch;
            }
            hitM = __ballot(brk || !skp);
            brkM = __ballot(brk);
            chM = __ballot(ch);
          }
          const uint64_t m = hitM & ~lowmask(i0 - sb);
          if (m == 0) {
            i0 = sb + 64;
            li0 = 0;
            if (i0 >= nb) { res = 2; break; }
            continue;
          }
          const int k = (int)__builtin_ctzll(m);
          if (sb + k > i0) li0 = 0;
          i0 = sb + k;
          if ((brkM >> k) & 1ull) res = 1;
          ot0 = bcast(otb, k);
          const int nbr = ((chM >> k) & 1ull) ? i0 : -1;
          if (nbr != cbr) {
            cq_children(cx, buf, nb, cbr, nbr);
            cbr = nbr;
          }
          break;
        }
        if (pc) pc[20] += __builtin_amdgcn_s_memtime() - te0;
        if (res == 1) gstop = true;
        if (res != 0) break;
        if (pc) pc[21] += 1;
        enter = false;
        wa0 = -1;
      }
      if (tsn > 0 && !(((txo - norm) + ot0) > bottom)) {
        if (pc) pc[22] += 1;
        if (li0 == 0 && cbr != i0) {
          // a run of branches i0, i0 + 1, ... (lane L: branch i0 + L) each
          // with every candidate in S, no branch children and an open turn
          // (branch i0's was checked by the branch scan): each takes one
          // ballot of its S offers that beat the bound, in branch order,
          // while they fit the chunk -- the same decisions and entries as
          // the per-branch path below, without its branch selection
          const int ib = i0 + lane;
          const bool vb = ib < nb;
          const T otL = vb ? sel(cx.ot, buf)[ib] : NI;
          const bool okL = vb && (otL > bottom) && cx.head[ib] < 0 && !(((txo - norm) + otL) > bottom);
          const uint64_t badM = ~__ballot(okL || lane == 0);
          const int R = badM ? (int)__builtin_ctzll(badM) : 64;   // run length (>= 1)
          const T sxv = tsx - norm;                                // S lane j: x_j - norm
          int L = 0;
          for (; L < R; ++L) {
            const T ob = bcast(otL, L);
            const bool h = lane < tsn && ((sxv + ob) > bottom);
            const uint64_t hM = __ballot(h);
            const int nh = __builtin_popcountll(hM);
            if (nh > cap - cqn) break;
            if (h) {
              const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hM >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)hM, 0u));
              cq[cqn + r] = ((uint32_t)(i0 + L) << 16) | (uint32_t)tsl;
            }
            cqn += nh;
          }
          if (L > 0) {
            i0 += L;
            li0 = 0;
            enter = true;
            if (i0 >= nb) break;
            continue;
          }
        }
        // every candidate of branch i0 is in S: its offers from li0 on that
        // beat the bound, merged in label order with its children (from the
        // bitmap, ascending); a branch that does not fit the chunk's room
        // starts the next chunk (or, first in the chunk, goes by windows)
        const bool hot = tsl >= li0 && (((tsx - norm) + ot0) > bottom);
        const uint64_t hotM = __ballot(hot);
        const int nh = __builtin_popcountll(hotM);
        int padd = 0, nch = 0;
        if (cbr == i0) {
          for (int q = 0; q * 64 < (Cm1 + 63) / 64; ++q) {
            uint64_t wq = uni64(cwin[q]);
            while (wq) {
              const int a = q * 64 + (int)__builtin_ctzll(wq);
              wq &= wq - 1ull;
              uint64_t bits = uni64(cbm[a]);
              if (a * 64 < li0) bits &= ~lowmask(li0 - a * 64);
              while (bits) {
                const int xc = a * 64 + (int)__builtin_ctzll(bits);
                bits &= bits - 1ull;
                if (__ballot(hot && tsl == xc)) continue;   // also a hot offer of S
                const int pos = cqn + __builtin_popcountll(hotM & __ballot(tsl < xc)) + nch;
                if (lane == 0 && pos < cap) cq[pos] = ((uint32_t)i0 << 16) | (uint32_t)xc;
                padd += (tsl > xc) ? 1 : 0;
                ++nch;
              }
            }
          }
        }
        if (pc) pc[23] += __builtin_amdgcn_s_memtime() - te0;
        if (nh + nch <= cap - cqn) {
          if (hot) {
            const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hotM >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((unsigned)hotM, 0u));
            cq[cqn + r + padd] = ((uint32_t)i0 << 16) | (uint32_t)tsl;
          }
          cqn += nh + nch;
          ++i0;
          li0 = 0;
          enter = true;
          if (i0 >= nb) break;
          continue;
        }
        if (cqn > 0) break;
      }
      // branch i0's aligned 64-label windows from li0 on (lane w: window
      // wa0 + w): one whose labels' block maxima bound every score
      // (xb - norm) + ot0 <= bottom and that holds no child is passed over
      const uint64_t tw0 = pc ? __builtin_amdgcn_s_memtime() : 0;
      if (pc) pc[17] += 1;
      if (wa0 < 0 || (li0 >> 6) >= wa0 + 64) {
        wa0 = li0 >> 6;
        const int lw = (wa0 + lane) * 64;
        bool keep = false;
        if (lw < Cm1) {
          const int le = (lw + 64 < Cm1 ? lw + 64 : Cm1) - 1;
          const int la = lw + (lw >= blank ? 1 : 0);
          const int lb = le + (le >= blank ? 1 : 0);
          const T ba = bmax[la >> 6], bb = bmax[lb >> 6];
          const T xb = ba > bb ? ba : bb;
          const int a = wa0 + lane;
          keep = (((xb - norm) + ot0) > bottom) || (((cwin[a >> 6] >> (a & 63)) & 1ull) != 0);
        }
        wkM = __ballot(keep);
      }
      uint64_t m = wkM & ~lowmask((li0 >> 6) - wa0);
      int nli0;
      if (m == 0) {
        nli0 = (wa0 + 64) * 64;
      } else {
        // up to kGatherWin kept windows per batch of row reads: the exact
        // per-label bound, and the children
        int aw[kGatherWin];
        T xv[kGatherWin];
        uint64_t cw[kGatherWin];
#pragma unroll
        for (int j = 0; j < kGatherWin; ++j) {
          aw[j] = -1;
          if (m) {
            aw[j] = wa0 + (int)__builtin_ctzll(m);
            m &= m - 1ull;
          }
        }
#pragma unroll
        for (int j = 0; j < kGatherWin; ++j) {
          xv[j] = NI;
          cw[j] = 0ull;
          if (aw[j] >= 0) {
            const int x = aw[j] * 64 + lane;
            const int xc = x < Cm1 ? x : Cm1 - 1;
            xv[j] = cx.row[xc + (xc >= blank ? 1 : 0)];
            cw[j] = cbm[aw[j]];
          }
        }
        nli0 = -1;
        int endw = 0;
#pragma unroll
        for (int j = 0; j < kGatherWin; ++j) {
          if (aw[j] >= 0 && nli0 < 0 && cqn < cap) {
            const int wb = aw[j] * 64;
            const int x = wb + lane;
            const bool hot = x >= li0 && x < Cm1 &&
                             ((((xv[j] - norm) + ot0) > bottom) || (((cw[j] >> lane) & 1ull) != 0));
            uint64_t hotM = __ballot(hot);
            const int rank =
                (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hotM >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hotM, 0u));
            if (__builtin_popcountll(hotM) > cap - cqn) {   // the chunk fills here
              hotM = __ballot(hot && rank < cap - cqn);
              nli0 = wb + 64 - __builtin_clzll(hotM);
            }
            if ((hotM >> lane) & 1ull) cq[cqn + rank] = ((uint32_t)i0 << 16) | (uint32_t)x;
            cqn += __builtin_popcountll(hotM);
            endw = wb + 64;
          }
        }
        if (nli0 < 0) nli0 = endw;
      }
      li0 = nli0;
      if (pc) pc[18] += __builtin_amdgcn_s_memtime() - tw0;
      if (li0 >= Cm1) {
        ++i0;
        li0 = 0;
        enter = true;
        if (i0 >= nb) break;
      }
    }
  if (pc) pc[16] += __builtin_amdgcn_s_memtime() - tg0;
}

// The gather queue of the two-wave large-C kernels: wave 1 gathers the
// frame's compacted chunks (gather_chunk, with the last bottom wave 0
// published: a superset of the offers that can have an effect, see there)
// into a ring of kQSlots chunks; wave 0 takes them in order and runs their
// events.  A chunk with cqn = 0 ends the frame's grow (gstop: a closed turn).
// Hand-over as for the score table (kCtlReady / kCtlCons / kCtlDone), plus
// wave 0's bottom after every chunk (kCtlBot, float bits).
#ifndef CTCX_QSLOTS
#define CTCX_QSLOTS 4
#endif
constexpr int kQSlots = CTCX_QSLOTS;   // chunks the helper may gather ahead of wave 0
constexpr int kCtlBot = 12;
// The scored form (SQ kernels: beams <= 128, any C): the helper also scores
// each gathered offer, as the score table does, so wave 0 reads a chunk's
// offers ready to push (per lane: score, branch total, packed (branch |
// (branch child + 1) << 8 | label << 16), the child's label-ending candidate
// (back-pointer; value in p)).  Wave 0 reads only what events change (bst).
struct GQ {
  CTCX_LDS uint32_t* e;     // [slot][64]: (branch << 16) | label index (unscored)
  CTCX_LDS int* h;          // [slot][4]: cqn, span start (branch, label index), gstop
  CTCX_LDS u32x4* a;        // [slot][64]: scored offers (SQ)
  CTCX_LDS float* p;        // [slot][64]: their candidate values (SQ)
  int sm;                   // slots - 1 (a power of two)
};
// Scored slots per kernel: four for beams <= 128; one for beams of 129..256,
// whose layout must stay under half a CU (cfg5: 80.1 KB of the 80 KB, a
// scored slot 1.3 KB) -- with one slot the helper gathers chunk c + 1 while
// wave 0 runs chunk c (wave 0 has read the slot before it publishes kCtlCons)
__host__ __device__ constexpr int sq_slots(int wcap) { return wcap <= 128 ? kQSlots : 1; }
__host__ __device__ inline size_t gq_lds_bytes(bool scored, int slots = kQSlots) {
  return (size_t)slots * ((scored ? 64 * 20 : 64 * 4) + 16);
}
// The frame boundary of the scored queue's small-C kernels (SQ && !BIG: float,
// beams <= 128, C <= 64, base scorer), off wave 0's chain (DESIGN, round 16):
// CTCX_ROW_PREFETCH: the helper, idle once its ranks are out, loads row t + 1
// and its normaliser into a second row buffer while wave 0 extracts, and names
// the frame in kPfRowT; frame t + 1's row stage then only switches buffers.
// CTCX_EARLY_CHUNK0: with the beam full the helper goes from the row test
// straight into the gather, so the frame's first chunk is scored beside wave
// 0's recursion (from a bottom of -inf: any bottom at or below the true one
// gives a correct chunk), and wave 0 rolls and recurses its 128 branches alone.
#ifndef CTCX_ROW_PREFETCH
#define CTCX_ROW_PREFETCH 1
#endif
#ifndef CTCX_EARLY_CHUNK0
#define CTCX_EARLY_CHUNK0 1
#endif
constexpr bool kRowPrefetch = CTCX_ROW_PREFETCH != 0;
constexpr bool kEarlyChunk0 = CTCX_EARLY_CHUNK0 != 0;
// the second row buffer, then four words: the frame it holds (kPfRowT; -1:
// none) and that row's normaliser (kPfNorm).  After the gather queue, so
// decode_lds_bytes (and with it ctcext_max_beam_width) is what it was.
[[maybe_unused]] constexpr int kPfRowT = 0, kPfNorm = 1;
__host__ __device__ constexpr size_t sq_rowpf_bytes(int64_t C) {
  return (kRowPrefetch && C <= 64) ? ((((size_t)C * 4) + 15) & ~(size_t)15) + 16 : 0;
}
// CTCX_EARLY_RECURSE (the same kernels; DESIGN, round 17): once its ranks are
// out and row t + 1 is in the second row buffer, the helper computes frame
// t + 1's recursion while wave 0 extracts.  The recursion of the branch at
// position k needs that branch's words, its parent's and the row, not k: the
// helper works on the final beam as wave 0 publishes it for the ranks (entry
// j of the heap's copy: total xv[j], slot alias[j]), reads every source by
// slot, and stages the recursion's nine result words per j (both endings, the
// total, both candidates with their back-pointers, the flags, the label),
// back-pointers as (j << 1) | kind.  The commit, which knows each slot's
// position, moves the staged words to e*[position] after its last read of
// e*[sorted[.]], and the next frame's wave 0 skips recurse_wave0.
// The staging area follows the second row buffer (so decode_lds_bytes and
// ctcext_max_beam_width are what they were): four words (kErT: the frame the
// staged words are for, -1: none), then ten planes of wcap words (kErNbk ..
// kErLab: those nine words; kErPos: the position of entry j, written by the
// commit).  During the hand-over the gather queue's offer plane (dead between
// the grow's end and the next frame) holds two maps: slot -> j (kErMapSlot,
// enc words) and branch -> j of its surviving entry (kErMapBr, wcap words).
#ifndef CTCX_EARLY_RECURSE
#define CTCX_EARLY_RECURSE 1
#endif
constexpr bool kEarlyRecurse = CTCX_EARLY_RECURSE != 0 && kRowPrefetch && kEarlyChunk0;
[[maybe_unused]] constexpr int kErT = 0;
[[maybe_unused]] constexpr int kErNbk = 0, kErNl = 1, kErTot = 2, kErCb = 3, kErCn = 4, kErBpb = 5, kErBpn = 6,
                               kErFlg = 7, kErLab = 8, kErPos = 9, kErPlanes = 10;
[[maybe_unused]] constexpr int kErMapSlot = 0, kErMapBr = 512;   // (word offsets in the offer plane: 3 * 128 + 2 <= 512)
__host__ __device__ constexpr size_t sq_stage_bytes(int wcap, int64_t C) {
  return (kEarlyRecurse && C <= 64) ? 16 + (size_t)kErPlanes * (size_t)wcap * 4 : 0;
}
template <bool SCORED>
__device__ __forceinline__ GQ gq_carve(CTCX_LDS char* p, int slots) {
  GQ q{};
  q.sm = slots - 1;
  if constexpr (SCORED) {
    q.a = (CTCX_LDS u32x4*)p;
    q.p = (CTCX_LDS float*)(p + (size_t)slots * 64 * 16);
    q.h = (CTCX_LDS int*)(p + (size_t)slots * 64 * 20);
  } else {
    q.e = (CTCX_LDS uint32_t*)p;
    q.h = (CTCX_LDS int*)(p + (size_t)slots * 64 * 4);
  }
  return q;
}
// a scored offer's packed word: branch (bits 0-7), branch child + 1 (8-16),
// label (17-31; the scored queue runs for C <= kSqMaxClasses)
constexpr int kSqMaxClasses = 32768;
__device__ __forceinline__ uint32_t sq_pack(int i, int cw, int l) {
  return (uint32_t)i | ((uint32_t)(cw + 1) << 8) | ((uint32_t)l << 17);
}
// ... at small C (labels < 64: bits 17-22) also the chunk lane where the
// offer's branch turn starts, plus one (bits 23-29; 0: in an earlier chunk),
// so wave 0 reads it instead of deriving it from its neighbour's branch
__device__ __forceinline__ uint32_t sq_pack_sl(int i, int cw, int l, int sl) {
  return sq_pack(i, cw, l) | ((uint32_t)(sl + 1) << 23);
}
__device__ __forceinline__ int sq_label_small(uint32_t pk) { return (int)((pk >> 17) & 63u); }
__device__ __forceinline__ int sq_turn_lane(uint32_t pk) { return (int)((pk >> 23) & 127u) - 1; }

// One offer's scored fields, from the frame-start state only (what the
// score table holds): its score (decoder.h:166-171), its branch's total, the
// branch child it re-offers (GetChild finds it; -1: none) and the child's
// label-ending alignment candidate (decoder.h:172-185).  v: a real offer
// (others skip the child walk).
template <typename T>
__device__ __forceinline__ void sq_score(const Ctx<T>& cx, int buf, T norm, bool v, int i, int l, T& s, T& bt,
                                         int& cw, Best<T>& cd) {
  const T NI = ninf<T>();
  const int bl = sel(cx.lab, buf)[i];
  const int bflg = sel(cx.flg, buf)[i];
  bt = sel(cx.ot, buf)[i];
  const T bob = sel(cx.ob, buf)[i];
  const int hd = cx.head[i];
  const T bcb = sel(cx.cb, buf)[i], bcn = sel(cx.cn, buf)[i];
  const T p = cx.row[l] - norm;
  s = p + ((l == bl) ? bob : bt);
  cw = -1;
  for (int k = v ? hd : -1; __ballot(k >= 0);) {
    CTCX_HPC(cx, 27, 1);
    int nk = -1;
    if (k >= 0) {
      const int lk = sel(cx.lab, buf)[k];
      const int sk = cx.sib[k];
      if (lk == l) cw = k;
      else nk = sk;
    }
    k = nk;
  }
  const bool recv_fresh = cw >= 0 ? (sel(cx.ot, buf)[cw] == NI) : true;
  const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
  cd = Best<T>{T(0), kBpNone, false};
  cd.push(((bflg & F_HB) ? bcb : rs_blank) + p, (bflg & F_HB) ? (((uint32_t)i << 1) | 0u) : kBpRestart);
  if (l != bl) cd.push(((bflg & F_HN) ? bcn : NI) + p, (bflg & F_HN) ? (((uint32_t)i << 1) | 1u) : kBpRestart);
}

// Small C (SQ kernels): the offers from (i0, li0) on that can have an effect
// -- a new child scoring above the given bottom, or any re-offer of a branch
// child (it may be evicted by its turn) -- scored and compacted into the
// slot in offer order, up to 64, scanning 64 offers in (branch, label index)
// order per step.  A branch whose turn is closed at that bottom (closed then:
// closed at its turn, as the bottom only rises) ends the frame's grow before
// it (gstop).  Any bottom at or below the true one gives a correct chunk.
template <typename T>
__device__ __forceinline__ void gather_small_scored(const Ctx<T>& cx, int buf, int nb, T norm, T bottom, int& i0,
                                                    int& li0, bool& gstop, CTCX_LDS u32x4* qa, CTCX_LDS float* qp,
                                                    int& cqn, bool one_step) {
  const int lane = threadIdx.x & 63;
  const int Cm1 = cx.C - 1, blank = cx.blank;
  const float rcp = 1.0f / (float)Cm1;
  cqn = 0;
  // each offer's turn-start lane (sq_pack_sl): the chunk position of its
  // branch's first gathered offer, unless the branch began before the span
  // (wave 0 found that turn open in an earlier chunk).  A branch gathered in
  // an earlier scan step of this chunk is the last one gathered there (lbr,
  // its first position lpos): offers come in branch order.
  const int sp_i0 = i0;
  const bool sp_mid = li0 != 0;
  int lbr = -1, lpos = 0;
  while (cqn < 64 && i0 < nb) {
    CTCX_HPC(cx, 31, 1);
    const int x = li0 + lane;
    int q = (int)((float)x * rcp);
    q -= (q * Cm1 > x) ? 1 : 0;
    q += ((q + 1) * Cm1 <= x) ? 1 : 0;
    const int iv = i0 + q;
    const bool v = iv < nb;
    const int i = v ? iv : i0;
    const int li = v ? x - q * Cm1 : 0;
    const int l = li + (li >= blank ? 1 : 0);
    T s, bt;
    int cw;
    Best<T> cd;
    sq_score<T>(cx, buf, norm, v, i, l, s, bt, cw, cd);
    // a turn starting in this step (label index 0) and closed at this bottom
    const uint64_t brkM = __ballot(v && li == 0 && !(bt > bottom));
    const int kb = brkM ? (int)__builtin_ctzll(brkM) : 64;
    const bool want = v && ((s > bottom) || cw >= 0) && lane < kb;
    uint64_t wM = __ballot(want);
    int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(wM >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)wM, 0u));
    const int room = 64 - cqn;
    int adv;   // offers of the step passed over
    if (__builtin_popcountll(wM) > room) {   // the chunk fills: resume after its last offer
      wM = __ballot(want && rank < room);
      adv = 64 - __builtin_clzll(wM);
    } else {
      adv = kb;
      if (kb < 64) gstop = true;
    }
    // branch i's offers begin at step lane b0 (lane - li; 0: in an earlier
    // step), so its first gathered offer follows the wanted lanes below b0
    const int b0 = lane > li ? lane - li : 0;
    const int tl = (i == lbr) ? lpos : cqn + (int)__builtin_popcountll(wM & ((1ull << b0) - 1ull));
    if ((wM >> lane) & 1ull) {
      u32x4 e;
      e.x = __builtin_bit_cast(unsigned, (float)s);
      e.y = __builtin_bit_cast(unsigned, (float)bt);
      e.z = sq_pack_sl(i, cw, l, (sp_mid && i == sp_i0) ? -1 : tl);
      e.w = cd.bp;
      qa[cqn + rank] = e;
      qp[cqn + rank] = (float)cd.p;
    }
    if (wM) {
      const int last = 63 - (int)__builtin_clzll(wM);
      lbr = bcast(i, last);
      lpos = bcast(tl, last);
    }
    cqn += __builtin_popcountll(wM);
    // (i0, li0) += adv offers
    const int xa = li0 + adv;
    int qa2 = (int)((float)xa * rcp);
    qa2 -= (qa2 * Cm1 > xa) ? 1 : 0;
    qa2 += ((qa2 + 1) * Cm1 <= xa) ? 1 : 0;
    i0 += qa2;
    li0 = xa - qa2 * Cm1;
    if (gstop || (one_step && cqn > 0)) break;
  }
}

// CTCX_SPARSE_BRANCH (DESIGN, round 19): pass 1 of the sparse gather below with
// one BRANCH per lane instead of one offer per lane.  The want test
//   (row[l] - norm) + (l == bl ? bob : bt) > bottom
// has one operand that is the same for every branch (row[l] - norm) and three
// that a lane can hold for the whole frame, so a window of 64 branches is
// tested in C - 1 iterations of a few VALU instructions each, with no
// division and no LDS gather, where the offer-per-lane form needs C - 1 scan
// steps for the same 64 * (C - 1) offers.  The result per branch is a mask of
// wanted label indices; popcounts and a prefix over the lanes place each
// lane's wanted offers in the chunk.  The staged words, their order, cqn,
// gstop and the resume point are those of the scan-step form for the same
// (i0, li0, bottom) (tests/test_cpu_branch_gather.py restates both): the
// resume point is that form's, step-granular, computed from the linear offer
// index x = (i - i0) * (C - 1) + li.
#ifndef CTCX_SPARSE_BRANCH
#define CTCX_SPARSE_BRANCH 1
#endif
constexpr bool kSparseBranch = CTCX_SPARSE_BRANCH != 0;
// The frame's branches as the helper holds them, lane b of window w branch
// 64 * w + b (beams <= 128: two windows), from the frame-start arrays.
template <typename T>
struct SqBr {
  T pv;             // lane l < C: row[l] - norm
  T bt[2];          // the branch's total
  T sl[2];          // the score of its own label's offer: (row[bl] - norm) + bob
  int li[2];        // its own label as a label index (-1: none)
  uint64_t cm[2];   // its children's labels, as label indices (wanted whatever the bottom)
};
__device__ __forceinline__ uint64_t lowmask_any(int n) { return n <= 0 ? 0ull : lowmask(n); }
// inclusive prefix sum over the wave's lanes: DPP row shifts inside each row
// of 16, then the row totals by readlane
__device__ __forceinline__ int wave_incl_sum_dpp(int v) {
  v += dpp_i<0x111>(v, 0);   // row_shr:1
  v += dpp_i<0x112>(v, 0);   // row_shr:2
  v += dpp_i<0x114>(v, 0);   // row_shr:4
  v += dpp_i<0x118>(v, 0);   // row_shr:8
  const int r0 = bcast(v, 15), r1 = bcast(v, 31), r2 = bcast(v, 47);
  const int row = (int)(threadIdx.x & 63) >> 4;
  return v + (row == 0 ? 0 : row == 1 ? r0 : row == 2 ? r0 + r1 : r0 + r1 + r2);
}
template <typename T>
__device__ __forceinline__ void sq_br_load(const Ctx<T>& cx, int buf, int nb, T norm, SqBr<T>& S) {
  const int lane = threadIdx.x & 63;
  const int C = cx.C, blank = cx.blank;
  S.pv = cx.row[lane < C ? lane : 0] - norm;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int i = 64 * w + lane;
    const bool v = i < nb;
    const int ii = v ? i : 0;
    const int bl = sel(cx.lab, buf)[ii];
    const T bob = sel(cx.ob, buf)[ii];
    const bool own = bl >= 0 && bl < C && bl != blank;
    S.bt[w] = sel(cx.ot, buf)[ii];
    S.li[w] = own ? bl - (bl > blank ? 1 : 0) : -1;
    S.sl[w] = (cx.row[own ? bl : 0] - norm) + bob;
    uint64_t cm = 0;
    for (int k = v ? cx.head[ii] : -1; __ballot(k >= 0);) {
      CTCX_HPC(cx, 27, 1);
      if (k >= 0) {
        const int lk = sel(cx.lab, buf)[k];
        if (lk >= 0) cm |= 1ull << ((lk - (lk > blank ? 1 : 0)) & 63);
        k = cx.sib[k];
      }
    }
    S.cm[w] = cm;
  }
}
// window w's wanted label indices per branch at this bottom: the same float
// expression per offer as sq_score's (contraction off)
template <typename T>
__device__ __forceinline__ uint64_t sq_br_want(const SqBr<T>& S, int w, int Cm1, int blank, T bottom) {
  const T bt = w ? S.bt[1] : S.bt[0];
  uint32_t lo = 0, hi = 0;
  const int n0 = Cm1 < 32 ? Cm1 : 32;
  for (int li = 0; li < n0; ++li) {
    const T s = bcast(S.pv, li + (li >= blank ? 1 : 0)) + bt;
    lo |= (s > bottom) ? (1u << li) : 0u;
  }
  for (int li = 32; li < Cm1; ++li) {
    const T s = bcast(S.pv, li + (li >= blank ? 1 : 0)) + bt;
    hi |= (s > bottom) ? (1u << (li - 32)) : 0u;
  }
  uint64_t M = ((uint64_t)hi << 32) | lo;
  const int lib = w ? S.li[1] : S.li[0];   // the branch's own label: its label-ending total instead
  if (lib >= 0) {
    const uint64_t b = 1ull << lib;
    M = (M & ~b) | (((w ? S.sl[1] : S.sl[0]) > bottom) ? b : 0ull);
  }
  return M | (w ? S.cm[1] : S.cm[0]);
}
// One window: its wanted masks with the span's start and the first closed turn
// applied (kbr: that branch's lane, 64: none; a turn is closed only if it
// starts inside the scan).
template <typename T>
__device__ __forceinline__ uint64_t sq_br_window(const SqBr<T>& S, int w, int nb, int Cm1, int blank, T bottom, int i0,
                                                  int li0, int& kbr) {
  const int i = 64 * w + (int)(threadIdx.x & 63);
  const bool v = i >= i0 && i < nb;
  uint64_t M = sq_br_want<T>(S, w, Cm1, blank, bottom);
  M = v ? M : 0ull;
  if (i == i0) M &= ~lowmask(li0);
  const uint64_t cM = __ballot(v && !((w ? S.bt[1] : S.bt[0]) > bottom) && (i > i0 || li0 == 0));
  kbr = cM ? (int)__builtin_ctzll(cM) : 64;
  return (int)(threadIdx.x & 63) >= kbr ? 0ull : M;
}
// Pass 1 of gather_small_sparse in that form: stages the chunk's packed words
// at sc[0 .. cqn) and moves (i0, li0) to the resume point.
template <typename T>
__device__ __forceinline__ void gather_small_branch(const Ctx<T>& cx, int buf, int nb, T bottom, int& i0, int& li0,
                                                    bool& gstop, CTCX_LDS uint32_t* sc, int& cqn, const SqBr<T>& S) {
  const int lane = threadIdx.x & 63;
  const int Cm1 = cx.C - 1, blank = cx.blank;
  cqn = 0;
  if (i0 >= nb) return;
  const int xend = (nb - i0) * Cm1;   // offers from branch i0's first to the frame's last
  int xres = 0;                       // the resume point as an offer index from branch i0's first
  for (int w = i0 >> 6;; ++w) {
    CTCX_HPC(cx, 31, 1);
    const int i = 64 * w + lane;
    const int xs = (i - i0) * Cm1;   // the branch's first offer
    int kbr;
    uint64_t R = sq_br_window<T>(S, w, nb, Cm1, blank, bottom, i0, li0, kbr);
    const int cnt = (int)__builtin_popcountll(R);
    const int inc = wave_incl_sum_dpp(cnt);
    const int tot = bcast(inc, 63);
    const int room = 64 - cqn;
    // the lane's wanted offers that fit, lowest label first, at the chunk
    // positions after those of the lanes below
    int pos = cqn + inc - cnt;
    int t = room - (inc - cnt);
    t = t < 0 ? 0 : t > cnt ? cnt : t;
    const uint64_t tM = __ballot(t > 0);
    int lastli = 0;
    while (__ballot(t > 0)) {
      const bool on = t > 0;
      const int li = on ? (int)__builtin_ctzll(R) : 0;
      const int l = li + (li >= blank ? 1 : 0);
      const bool ch = on && (((w ? S.cm[1] : S.cm[0]) >> li) & 1ull);
      int cw = -1;
      if (__ballot(ch)) {   // GetChild: the first child of that label in the sibling list
        for (int k = ch ? cx.head[i] : -1; __ballot(k >= 0);) {
          CTCX_HPC(cx, 27, 1);
          int nk = -1;
          if (k >= 0) {
            const int lk = sel(cx.lab, buf)[k];
            const int sk = cx.sib[k];
            if (lk == l) cw = k;
            else nk = sk;
          }
          k = nk;
        }
      }
      if (on) {
        sc[pos] = sq_pack(i, cw, l);
        R &= R - 1ull;
        lastli = li;
        ++pos;
        --t;
      }
    }
    if (tot >= room) {
      // the chunk fills at offer x64, in the scan step [hi - 64, hi).  A wanted
      // offer left in that step (before a turn closed in it): the step-wise
      // form resumes after x64; none: it passes over the step's rest, up to
      // the closed turn.  The step may run on into the next window.
      const int L = 63 - (int)__builtin_clzll(tM);
      const int x64 = bcast(xs + lastli, L);
      const int hi = li0 + ((x64 - li0) & ~63) + 64;
      bool more = __ballot((R & lowmask_any(hi - xs)) != 0ull) != 0ull;
      int xstop = kbr < 64 ? bcast(xs, kbr) : hi;
      if (!more && kbr == 64 && 64 * (w + 1) < nb && (64 * (w + 1) - i0) * Cm1 < hi) {
        CTCX_HPC(cx, 31, 1);
        int kbr2;
        const uint64_t R2 = sq_br_window<T>(S, w + 1, nb, Cm1, blank, bottom, i0, li0, kbr2);
        const int xs2 = xs + 64 * Cm1;
        more = __ballot((R2 & lowmask_any(hi - xs2)) != 0ull) != 0ull;
        if (kbr2 < 64) xstop = bcast(xs2, kbr2);
      }
      xstop = xstop < hi ? xstop : hi;
      cqn = 64;
      if (more) {
        xres = x64 + 1;
      } else {
        xres = xstop;
        gstop = xstop < hi;
      }
      break;
    }
    cqn += tot;
    if (kbr < 64) {   // a closed turn ends the frame's grow before it
      xres = bcast(xs, kbr);
      gstop = true;
      break;
    }
    if (64 * (w + 1) >= nb) {   // the last step ran past the frame's last offer
      xres = li0 + ((xend - li0 + 63) & ~63);
      break;
    }
  }
  const int qr = xres / Cm1;
  i0 += qr;
  li0 = xres - qr * Cm1;
}

// The same chunk in two passes, for the chunks after the frame's first: those
// are sparse (cfg3, T = 1500: ~6.5 scan steps of 64 offers per chunk of up to
// 64), and gather_small_scored scores every scanned offer in full before it
// knows which are wanted.  Pass 1 (per scan step) reads only what the want
// test needs -- the branch's label, total and blank-ending total, the row
// value and the branch child (sq_score's walk: it runs only where the branch
// has children) -- applies the same brkM / kb / gstop, chunk-fills and resume
// rules, and stages one packed word (sq_pack: branch, child + 1, label) per
// wanted offer in the slot's value plane, as the large-C path stages its
// entries; nothing reads the plane before the chunk is published.  Pass 2
// (once per chunk) scores the staged offers, lane r the r-th, and writes the
// slot: the same entries, fields and order as gather_small_scored gives for
// the same bottom.  The score s is the same expression in both passes.
template <typename T>
__device__ __forceinline__ void gather_small_sparse(const Ctx<T>& cx, int buf, int nb, T norm, T bottom, int& i0,
                                                    int& li0, bool& gstop, CTCX_LDS u32x4* qa, CTCX_LDS float* qp,
                                                    int& cqn, [[maybe_unused]] const SqBr<T>* br = nullptr) {
  const int lane = threadIdx.x & 63;
  const int Cm1 = cx.C - 1, blank = cx.blank;
  const float rcp = 1.0f / (float)Cm1;
  CTCX_LDS uint32_t* sc = (CTCX_LDS uint32_t*)qp;
  cqn = 0;
  const int sp_i0 = i0;
  const bool sp_mid = li0 != 0;
  if constexpr (kSparseBranch) {   // pass 1 with a branch per lane
    gather_small_branch<T>(cx, buf, nb, bottom, i0, li0, gstop, sc, cqn, *br);
  } else
  while (cqn < 64 && i0 < nb) {   // pass 1: filter
    CTCX_HPC(cx, 31, 1);
    const int x = li0 + lane;
    int q = (int)((float)x * rcp);
    q -= (q * Cm1 > x) ? 1 : 0;
    q += ((q + 1) * Cm1 <= x) ? 1 : 0;
    const int iv = i0 + q;
    const bool v = iv < nb;
    const int i = v ? iv : i0;
    const int li = v ? x - q * Cm1 : 0;
    const int l = li + (li >= blank ? 1 : 0);
    const int bl = sel(cx.lab, buf)[i];
    const T bt = sel(cx.ot, buf)[i];
    const T bob = sel(cx.ob, buf)[i];
    const T p = cx.row[l] - norm;
    const T s = p + ((l == bl) ? bob : bt);
    int cw = -1;
    for (int k = v ? cx.head[i] : -1; __ballot(k >= 0);) {
      CTCX_HPC(cx, 27, 1);
      int nk = -1;
      if (k >= 0) {
        const int lk = sel(cx.lab, buf)[k];
        const int sk = cx.sib[k];
        if (lk == l) cw = k;
        else nk = sk;
      }
      k = nk;
    }
    // a turn starting in this step (label index 0) and closed at this bottom
    const uint64_t brkM = __ballot(v && li == 0 && !(bt > bottom));
    const int kb = brkM ? (int)__builtin_ctzll(brkM) : 64;
    const bool want = v && ((s > bottom) || cw >= 0) && lane < kb;
    uint64_t wM = __ballot(want);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(wM >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)wM, 0u));
    const int room = 64 - cqn;
    int adv;   // offers of the step passed over
    if (__builtin_popcountll(wM) > room) {   // the chunk fills: resume after its last offer
      wM = __ballot(want && rank < room);
      adv = 64 - __builtin_clzll(wM);
    } else {
      adv = kb;
      if (kb < 64) gstop = true;
    }
    if ((wM >> lane) & 1ull) sc[cqn + rank] = sq_pack(i, cw, l);
    cqn += __builtin_popcountll(wM);
    // (i0, li0) += adv offers
    const int xa = li0 + adv;
    int qa2 = (int)((float)xa * rcp);
    qa2 -= (qa2 * Cm1 > xa) ? 1 : 0;
    qa2 += ((qa2 + 1) * Cm1 <= xa) ? 1 : 0;
    i0 += qa2;
    li0 = xa - qa2 * Cm1;
    if (gstop) break;
  }
  if (cqn == 0) return;
  // pass 2: score.  The turn-start lane is the chunk position of the branch's
  // first staged offer (the entries are in branch order), unless the branch
  // began before the span.
  wsync<true>();
  const bool v = lane < cqn;
  const uint32_t e = v ? sc[lane] : 0u;
  const uint32_t ep = sc[(v && lane > 0) ? lane - 1 : 0];
  const int i = (int)(e & 255u);
  const int cw = (int)((e >> 8) & 511u) - 1;
  const int l = sq_label_small(e);
  const uint64_t fm = __ballot(v && (lane == 0 || (int)(ep & 255u) != i)) & lowmask(lane + 1);
  const int tl = 63 - (int)__builtin_clzll(fm | 1ull);
  const int bl = sel(cx.lab, buf)[i];
  const int bflg = sel(cx.flg, buf)[i];
  const T bt = sel(cx.ot, buf)[i];
  const T bob = sel(cx.ob, buf)[i];
  const T bcb = sel(cx.cb, buf)[i], bcn = sel(cx.cn, buf)[i];
  const T p = cx.row[l] - norm;
  const T s = p + ((l == bl) ? bob : bt);
  const T NI = ninf<T>();
  const bool recv_fresh = cw >= 0 ? (sel(cx.ot, buf)[cw] == NI) : true;
  const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
  Best<T> cd{T(0), kBpNone, false};
  cd.push(((bflg & F_HB) ? bcb : rs_blank) + p, (bflg & F_HB) ? (((uint32_t)i << 1) | 0u) : kBpRestart);
  if (l != bl) cd.push(((bflg & F_HN) ? bcn : NI) + p, (bflg & F_HN) ? (((uint32_t)i << 1) | 1u) : kBpRestart);
  wsync<true>();   // every lane has read its neighbour's staged word
  if (v) {
    u32x4 ev;
    ev.x = __builtin_bit_cast(unsigned, (float)s);
    ev.y = __builtin_bit_cast(unsigned, (float)bt);
    ev.z = sq_pack_sl(i, cw, l, (sp_mid && i == sp_i0) ? -1 : tl);
    ev.w = cd.bp;
    qa[lane] = ev;
    qp[lane] = (float)cd.p;
  }
}

// The scored gather queue's helper (SQ kernels): as help_gather_chunks, up to
// kSqLead chunks ahead of wave 0, each chunk's offers scored (sq_score).
// small C: one ahead since the branch-per-lane filter (kSparseBranch; round
// 19: with the gather cheap the helper no longer needs the head start, and
// chunks gathered against a fresher bottom carry fewer offers wave 0 then
// rejects: cfg3 106.05 -> 105.39 ms per step, cfg2 39.65 -> 39.32, every
// pair, profiles/r19_ab_lead.txt; with the scan-step filter two ahead won,
// cfg3 decode 124.9 -> 123.4 ms, and a -DCTCX_SPARSE_BRANCH=0 build keeps
// two); large C: one (two costs cfg4 +1.6%, for the same reason)
#ifndef CTCX_SQ_LEAD
#define CTCX_SQ_LEAD (CTCX_SPARSE_BRANCH != 0 ? 1 : 2)
#endif
#ifndef CTCX_SQ_FIRST1
#define CTCX_SQ_FIRST1 1
#endif
constexpr int kSqLead = CTCX_SQ_LEAD;   // (small C; large C gathers one ahead)
constexpr bool kSqFirst1 = CTCX_SQ_FIRST1 != 0;
#ifndef CTCX_SQ_CAP0
#define CTCX_SQ_CAP0 32
#endif
constexpr int kSqCap0 = CTCX_SQ_CAP0;   // large C: offers in the frame's first chunk (cfg4: 16, 32, 64 within 0.2%)
// EARLY (kEarlyChunk0): called beside wave 0's recursion with a bottom of
// -inf.  Chunk 0 is gathered at once; before chunk 1 the helper waits for wave
// 0's starting bottom (kCtlBot no longer the -inf of the row stage: a frame
// that stays exact has finite totals only), or chunk 1 would be gathered
// dense and wave 0 would pay for offers the true bottom rejects.  A frame
// whose recursion gave a non-finite total ends that wait through kCtlDone.
template <typename T, bool BIG, bool EARLY = false>
__device__ __forceinline__ void help_gather_scored(const Ctx<T>& cx, GQ q, int buf, int nb, T norm, T pmax,
                                                   T bottom) {
  const int lane = threadIdx.x & 63;
  CTCX_LDS int* m = cx.misc;
  if (ctl_ld(m, kCtlDead) != 0) return;
  const int blank = cx.blank;
  const int tsn = BIG ? cx.rns : 0;
  const T txo = BIG ? cx.rxout : ninf<T>();
  int i0 = 0, li0 = 0, cbr = -1;
  bool gstop = false;
  [[maybe_unused]] const uint64_t hg0 = CTCX_HTIME();
  [[maybe_unused]] SqBr<T> br;
  for (int c = 0;; ++c) {
    bool done = false;
    uint64_t tw = 0;
    // (kSparseBranch: the frame's branches into registers ahead of the first
    // sparse chunk, beside the wait for wave 0's starting bottom)
    if constexpr (!BIG && kSparseBranch)
      if (c == (kSqFirst1 ? 1 : 0)) sq_br_load<T>(cx, buf, nb, norm, br);
    [[maybe_unused]] const uint64_t hw0 = CTCX_HTIME();
    for (int spin = 0;; ++spin) {   // the grow still running, and wave 0 at most kSqLead chunks behind
      if (ctl_ld(m, kCtlDone) != 0) { done = true; break; }
      if (wait_expired(spin, tw)) {
        __hip_atomic_store(&m[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        done = true;
        break;
      }
      if (c < ctl_ld(m, kCtlCons) + (BIG ? 1 : kSqLead)) {
        if constexpr (EARLY) {
          if (c == 0 || ctl_ld(m, kCtlBot) != (int)0xff800000u) break;
        } else {
          break;
        }
      }
      __builtin_amdgcn_s_sleep(CTCX_SLEEP);
    }
    CTCX_HPC(cx, 26, CTCX_HTIME() - hw0);
    if (done) break;
    // wave 0's bottom after its last chunk (it only rises)
    const T pb = (T)__builtin_bit_cast(float, (unsigned)ctl_ld(m, kCtlBot));
    bottom = pb > bottom ? pb : bottom;
#ifdef CTCX_SQ_NOFILTER   // (diagnostics: every offer gathered, no closed turn found here)
    bottom = ninf<T>();
#endif
    // (diagnostics, small C: the frame's first chunk in three spans -- to the
    // control words read, the scan step, the publish: counters 16..18, which
    // the scored kernels leave free)
    [[maybe_unused]] const uint64_t hs1 = CTCX_HTIME();
    const int slot = c & q.sm;
    const int s_i0 = i0, s_l0 = li0;
    int cqn = 0;
    CTCX_LDS u32x4* qa = q.a + slot * 64;
    CTCX_LDS float* qp = q.p + slot * 64;
#if defined(CTCX_PHASE_LATE) && defined(CTCX_PHASES)   // (this chunk's scan steps or window passes: counter 31 before and after)
    const bool hlate = cx.prof && threadIdx.x == 64;
    const uint64_t hst0 = hlate ? __hip_atomic_load(cx.prof + 31, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
#endif
    if constexpr (BIG) {
      // the compacted (branch, label index) entries go to the slot's value
      // array first; each lane then scores its entry and overwrites its own
      // value word
      CTCX_LDS uint32_t* sc = (CTCX_LDS uint32_t*)qp;
      // (the frame's first chunk capped at kSqCap0 offers, so wave 0 starts sooner)
      gather_chunk<T>(cx, buf, nb, norm, pmax, bottom, tsn, txo, i0, li0, cbr, gstop, sc, cqn, PhaseCtr{nullptr},
                      c == 0 ? kSqCap0 : 64);
      wsync<true>();
      const bool v = lane < cqn;
      const uint32_t e = sc[v ? lane : 0];
      const int i = v ? (int)(e >> 16) : 0;
      const int li = v ? (int)(e & 0xFFFFu) : 0;
      const int l = li + (li >= blank ? 1 : 0);
      T s, bt;
      int cw;
      Best<T> cd;
      sq_score<T>(cx, buf, norm, v, i, l, s, bt, cw, cd);
      wsync<true>();
      if (v) {
        u32x4 ev;
        ev.x = __builtin_bit_cast(unsigned, (float)s);
        ev.y = __builtin_bit_cast(unsigned, (float)bt);
        ev.z = sq_pack(i, cw, l);
        ev.w = cd.bp;
        qa[lane] = ev;
        qp[lane] = (float)cd.p;
      }
    } else {
      // the frame's first chunk: the first scan step's offers only, so wave 0
      // starts after one step instead of a full chunk (the helper gathers the
      // next chunk meanwhile).  Its offers are dense and wave 0 waits for it:
      // scored as it is scanned.  The later chunks are sparse: filtered, then
      // scored (gather_small_sparse).
      if (kSqFirst1 && c == 0) gather_small_scored<T>(cx, buf, nb, norm, bottom, i0, li0, gstop, qa, qp, cqn, true);
      else if constexpr (kSparseBranch) gather_small_sparse<T>(cx, buf, nb, norm, bottom, i0, li0, gstop, qa, qp, cqn, &br);
      else gather_small_sparse<T>(cx, buf, nb, norm, bottom, i0, li0, gstop, qa, qp, cqn);
    }
    [[maybe_unused]] const uint64_t hs2 = CTCX_HTIME();
    if (lane == 0) {
      q.h[slot * 4 + 0] = cqn;
      q.h[slot * 4 + 1] = s_i0;
      q.h[slot * 4 + 2] = s_l0;
      q.h[slot * 4 + 3] = gstop ? 1 : 0;
    }
    __hip_atomic_store(&m[kCtlReady], c + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (c == 0) CTCX_HPC(cx, 25, CTCX_HTIME() - hg0);
    if (!BIG && c == 0) {
      CTCX_HPC(cx, 16, hs1 - hg0);
      CTCX_HPC(cx, 17, hs2 - hs1);
      CTCX_HPC(cx, 18, CTCX_HTIME() - hs2);
    }
    CTCX_HPC(cx, 30, 1);
#if defined(CTCX_PHASE_LATE) && defined(CTCX_PHASES)
    if (hlate)
      CTCX_HPC_(cx, kPhLateSteps + (c < 15 ? c : 15),
                __hip_atomic_load(cx.prof + 31, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - hst0);
#endif
    if (cqn == 0 || gstop) break;   // the last chunk of the frame
  }
  CTCX_HPC(cx, 24, CTCX_HTIME() - hg0);
  if (BIG && cbr >= 0) cq_children(cx, buf, nb, cbr, -1);   // the child bitmap starts the next frame clear
}

// Extract by rank, beside wave 0's sort_heap (SQ kernels, beams <= 128).
// sort_heap over a valid heap yields the totals in descending order; only the
// order WITHIN a group of equal totals depends on the heap's shape.  So if
// positions 0..p-1 hold entries whose totals are all distinct (p = the
// smallest rank of any tied entry, rank = the number of larger totals), each
// of them lands at its rank whatever the pops do, and wave 0 need only pop
// positions W-1 down to p.  Wave 0 copies the final heap (totals to
// cx.newpos, slots to cx.alias: neither is read between the grow and the
// commit) and raises kCtlExt before kCtlDone; the helper ranks the copy,
// writes sorted[r] for every r < p, then publishes p in kCtlStop.  Wave 0
// never waits for it: it reads kCtlStop between extract segments and stops at
// p once it sees one (round 3 placed by rank on wave 0: the rank pass cost
// ~5k cycles per frame, about what it saved).  A position both write holds the
// same slot either way.
#ifndef CTCX_EXT_RANK
#define CTCX_EXT_RANK 1
#endif
#ifndef CTCX_EXT_SLEEP
#define CTCX_EXT_SLEEP 1
#endif
constexpr bool kExtRank = CTCX_EXT_RANK != 0;
constexpr int kCtlStop = 3, kCtlExt = 7;   // (misc words; both reset per frame)
constexpr int kExtMinW = 16;               // beams below this pop too few positions to gain
template <typename T>
__device__ __forceinline__ void help_rank_extract(const Ctx<T>& cx, int tbuf = 0) {
  const int lane = threadIdx.x & 63;
  CTCX_LDS int* m = cx.misc;
  if (ctl_ld(m, kCtlDead) != 0) return;
  uint64_t tw = 0;
  for (int spin = 0;; ++spin) {   // wave 0's grow over (its copy, if any, is then in place)
    if (ctl_ld(m, kCtlDone) != 0) break;
    if (wait_expired(spin, tw)) {
      __hip_atomic_store(&m[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
    __builtin_amdgcn_s_sleep(CTCX_EXT_SLEEP);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (ctl_ld(m, kCtlExt) != 1) return;   // 1: wave 0 pops from the heap and reads the ranks' stop
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef CTCX_PHASE_EXTT
  const uint32_t hx0 = (uint32_t)__builtin_amdgcn_s_memtime();
  CTCX_HPC_(cx, 24, hx0 - (uint32_t)m[14]);   // (kCtlDone seen, after wave 0's extract start)
#endif
  const int W = cx.W;
  const CTCX_LDS float* xv = (const CTCX_LDS float*)cx.newpos;
  const bool in0 = lane < W, in1 = lane + 64 < W;
  const float v0 = in0 ? xv[lane] : 0.0f, v1 = in1 ? xv[lane + 64] : 0.0f;
  int g0 = 0, e0 = 0, g1 = 0, e1 = 0;
  const int W4 = (W + 3) >> 2;   // (wave 0 pads the copy to a multiple of 4 with NaN: never > or ==)
  int p = W;
  for (int j = 0; j < W4; ++j) {
    const u32x4 xq = ((const CTCX_LDS u32x4*)xv)[j];   // one address: a broadcast
    const float x[4] = {__uint_as_float(xq.x), __uint_as_float(xq.y), __uint_as_float(xq.z), __uint_as_float(xq.w)};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      g0 += x[u] > v0;
      e0 += x[u] == v0;
      g1 += x[u] > v1;
      e1 += x[u] == v1;
    }
  }
  if (__ballot((in0 && v0 != v0) || (in1 && v1 != v1))) return;   // (no order to rank by)
  if (in0 && e0 > 1) p = g0 < p ? g0 : p;
  if (in1 && e1 > 1) p = g1 < p ? g1 : p;
  p = uni(wave_min(p));
#ifdef CTCX_PHASE_BIRTH   // (diagnostics: ties in a frame whose previous frame ended without one)
  if ((cx).prof && threadIdx.x == 64) {
    const int pp = (int)cx.prof[29];   // the previous frame's p (state, not a sum; 0 at the first frame)
    if (pp == W) {
      CTCX_HPC_(cx, 30, 1);
      CTCX_HPC_(cx, 31, p < W ? 1 : 0);
    }
    CTCX_HPC_(cx, 28, p == W ? 1 : 0);
    cx.prof[29] = (uint64_t)p;
  }
#endif
#ifdef CTCX_PHASE_EXTP   // (diagnostics: the stop the helper found, 16-bit frame counts per range)
  CTCX_HPC(cx, 27, 1ull << (16 * (p <= 2 ? 0 : p < 64 ? 1 : p < 96 ? 2 : 3)));
#endif
#ifdef CTCX_PHASE_TIES   // (diagnostics: what the first two entries tied at rank p are)
  if (p < W) {
    const uint64_t t0m = __ballot(in0 && e0 > 1 && g0 == p), t1m = __ballot(in1 && e1 > 1 && g1 == p);
    const int fa = t0m ? (int)__builtin_ctzll(t0m) : 64 + (int)__builtin_ctzll(t1m);
    const uint64_t r0 = fa < 64 ? (t0m & (t0m - 1)) : 0ull, r1 = fa < 64 ? t1m : (t1m & (t1m - 1));
    const int fb = r0 ? (int)__builtin_ctzll(r0) : 64 + (int)__builtin_ctzll(r1);
    const int sa = cx.alias[fa], sb = cx.alias[fb];
    const uint32_t ka = cx.ekind[sa], kb = cx.ekind[sb];
    const int l = cx.elab[sa];
    if ((ka & 1u) && (kb & 1u) && l == cx.elab[sb]) {   // two new children, one label: their parents
      const int pa = (int)(ka >> 1), pb = (int)(kb >> 1);
      const int la = sel(cx.lab, tbuf)[pa], lb = sel(cx.lab, tbuf)[pb];
      const int qa = sel(cx.par, tbuf)[pa], qb = sel(cx.par, tbuf)[pb];
      CTCX_HPC_(cx, 25, 1);
      CTCX_HPC_(cx, 29, (l == la) + (l == lb));
      CTCX_HPC_(cx, 30, (qa == pb || qb == pa) ? 1 : 0);
      CTCX_HPC_(cx, 27, qa == qb ? 1 : 0);
      CTCX_HPC_(cx, 26, la == lb ? 1 : 0);
      CTCX_HPC_(cx, 24, sel(cx.ot, tbuf)[pa] == sel(cx.ot, tbuf)[pb] ? 1 : 0);
      CTCX_HPC_(cx, 31, (sel(cx.ob, tbuf)[pa] == sel(cx.ot, tbuf)[pb] || sel(cx.ob, tbuf)[pb] == sel(cx.ot, tbuf)[pa]) ? 1 : 0);
    }
  }
#endif
  if (p <= 2) return;   // wave 0 pops every position anyway
  if (in0 && g0 < p) cx.sorted[g0] = cx.alias[lane];
  if (in1 && g1 < p) cx.sorted[g1] = cx.alias[lane + 64];
  __hip_atomic_store(&m[kCtlStop], p, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef CTCX_PHASE_EXTT   // (diagnostics: cycles from wave 0's extract start to this publish)
  CTCX_HPC_(cx, 25, (uint32_t)__builtin_amdgcn_s_memtime() - (uint32_t)m[14]);
  CTCX_HPC_(cx, 26, 1);
  CTCX_HPC_(cx, 27, (uint32_t)__builtin_amdgcn_s_memtime() - hx0);
#endif
}

template <typename T>
__device__ __forceinline__ void help_gather_chunks(const Ctx<T>& cx, GQ q, int buf, int nb, T norm, T pmax, T bottom,
                                                   int lead) {
  const int lane = threadIdx.x & 63;
  CTCX_LDS int* m = cx.misc;
  if (ctl_ld(m, kCtlDead) != 0) return;
  const int tsn = cx.rns;
  const T txo = cx.rxout;
  int i0 = 0, li0 = 0, cbr = -1;
  bool gstop = false;
  for (int c = 0;; ++c) {
    bool done = false;
    uint64_t tw = 0;
    for (int spin = 0;; ++spin) {   // the grow still running, and a free slot
      if (ctl_ld(m, kCtlDone) != 0) { done = true; break; }
      if (wait_expired(spin, tw)) {
        __hip_atomic_store(&m[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        done = true;
        break;
      }
      if (c < ctl_ld(m, kCtlCons) + lead) break;
      __builtin_amdgcn_s_sleep(CTCX_SLEEP);
    }
    if (done) break;
    // wave 0's bottom after its last chunk (it only rises)
    const T pb = (T)__builtin_bit_cast(float, (unsigned)ctl_ld(m, kCtlBot));
    bottom = pb > bottom ? pb : bottom;
    const int slot = c & q.sm;
    const int s_i0 = i0, s_l0 = li0;
    int cqn = 0;
    gather_chunk<T>(cx, buf, nb, norm, pmax, bottom, tsn, txo, i0, li0, cbr, gstop, q.e + slot * 64, cqn, PhaseCtr{nullptr});
    if (lane == 0) {
      q.h[slot * 4 + 0] = cqn;
      q.h[slot * 4 + 1] = s_i0;
      q.h[slot * 4 + 2] = s_l0;
      q.h[slot * 4 + 3] = gstop ? 1 : 0;
    }
    __hip_atomic_store(&m[kCtlReady], c + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cqn == 0 || gstop) break;   // the last chunk of the frame
  }
  if (cbr >= 0) cq_children(cx, buf, nb, cbr, -1);   // the child bitmap starts the next frame clear
}

// kEarlyChunk0: wave 0's roll and recursion over every branch of a full beam
// (beams <= 128: branches lane and lane + 64), with no workgroup barrier.
template <typename T, class SC>
__device__ __forceinline__ void recurse_wave0(const Ctx<T>& cx, int buf, int nb, T norm) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < nb; i += 64) {
    cx.et[i] = sel(cx.ot, buf)[i]; cx.eb[i] = sel(cx.ob, buf)[i]; cx.el[i] = sel(cx.ol, buf)[i];
    cx.eflg[i] = 0;
    cx.bst[i] = 0;
    cx.bloom[i] = 0;
  }
  for (int i = lane; i < nb; i += 64) recurse_branch<T, SC>(cx, buf, i, i, norm, false);
  wsync<true>();   // (one wave: its LDS operations execute in order)
}

// kEarlyRecurse: the next frame's recursion in slot space, on the helper,
// while wave 0 extracts (DESIGN, round 17).  Called after help_rank_extract
// and after the row prefetch, in a frame whose final heap wave 0 published
// (kCtlExt == 1: xv[j], alias[j] for j < W): row (frame t + 1's, in the second
// row buffer) and norm are the helper's own prefetch.  For entry j at slot
// e = alias[j] it computes what the roll and recurse_branch(i, i, norm, false)
// compute next frame for i = the position the commit gives j, from what the
// commit will put there:
//   own words            et/eb/el/ecb/ecn/eflg/elab[e]      (put_branch)
//   flags, parent entry  as parent_of forms them, by slot: a new child's parent
//     is its source branch, a survivor's the branch par[buf][src], both present
//     iff that branch's entry is in the final beam (mb: branch -> j); a
//     survivor whose parent had left the beam finds it among the final beam's
//     new children by prefix hash (the commit's re-entered parent)
//   the parent's words   its entry's, eb/et/ecb/ecn/eflg/elab[alias[pj]]
// Same expressions in the same order as recurse_branch; back-pointers are
// staged as (j << 1) | kind and translated to positions by the commit.
// Reads only what stays as it is from the grow's end to the commit; writes
// the staging planes and the two maps in the gather queue's offer plane.
template <typename T, int WC>
__device__ __forceinline__ void help_early_recurse(const Ctx<T>& cx, int buf, const CTCX_LDS T* row, T norm,
                                                  CTCX_LDS int* sp, CTCX_LDS int* maps) {
  const int lane = threadIdx.x & 63;
  const int W = cx.W;
  const T NI = ninf<T>();
  CTCX_LDS int* const ms = maps + kErMapSlot;
  CTCX_LDS int* const mb = maps + kErMapBr;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // (the heap's copy, after kCtlExt)
  // the maps, and each new child's prefix hash (in registers: the re-entered
  // parent lookup compares across lanes)
  mb[lane] = -1;
  if (lane + 64 < WC) mb[lane + 64] = -1;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  int es[2], srcs[2];
  bool isn[2];
  uint64_t ca[2], cb2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    const bool in = j < W;
    const int e = in ? cx.alias[j] : 0;
    const uint32_t kd = cx.ekind[e];
    const int src = (int)(kd >> 1);
    es[h] = e;
    srcs[h] = src;
    isn[h] = in && (kd & 1u);
    ca[h] = sel(cx.ha, buf)[src];
    cb2[h] = sel(cx.hb, buf)[src];
    if (in) {
      ms[e] = j;
      if (!(kd & 1u)) mb[src] = j;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
  // parent entry (pj: its j, -1: none) and next-frame flags, as parent_of
  int pjs[2], fls[2];
  uint64_t pa[2] = {0, 0}, pb[2] = {0, 0};
  bool need[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    const bool in = j < W;
    const int e = es[h], src = srcs[h];
    const int pf = sel(cx.flg, buf)[src];
    const int pp = sel(cx.par, buf)[src];
    int pj, fl;
    need[h] = false;
    if (isn[h]) {
      pj = mb[src];
      fl = (pf & F_ROOT) ? F_PROOT : 0;
    } else {
      pj = pp >= 0 ? mb[pp] : -1;
      fl = pf & (F_ROOT | F_PROOT);
      need[h] = in && pp < 0 && !(pf & F_ROOT);
      if (need[h]) hmix_inv(ca[h], cb2[h], cx.elab[e], pa[h], pb[h]);
    }
    pjs[h] = pj;
    fls[h] = fl | (cx.eflg[e] & (F_HB | F_HN));
  }
  // a new child's own hash (a survivor's stays its branch's)
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (isn[h]) hmix(ca[h], cb2[h], cx.elab[es[h]], ca[h], cb2[h]);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint64_t m = __ballot(need[h]);
    while (m) {   // (uniform: one re-entered-parent lookup per round)
      const int l = (int)__builtin_ctzll(m);
      m &= m - 1;
      const uint64_t qa = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pa[h] >> 32), l) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pa[h], l);
      const uint64_t qb = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pb[h] >> 32), l) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pb[h], l);
      const uint64_t h0 = __ballot(isn[0] && ca[0] == qa && cb2[0] == qb);
      const uint64_t h1 = __ballot(isn[1] && ca[1] == qa && cb2[1] == qb);
      const int found = h0 ? (int)__builtin_ctzll(h0) : h1 ? 64 + (int)__builtin_ctzll(h1) : -1;
      if (lane == l) pjs[h] = found;
    }
  }
  // the recursion (recurse_branch's expressions after the roll, sources by slot)
  const T xb = row[cx.blank];
  const T pbk = xb - norm;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    if (j >= W) continue;
    const int e = h ? es[1] : es[0];
    const int f = h ? fls[1] : fls[0];
    const int pj = h ? pjs[1] : pjs[0];
    const int L = cx.elab[e];
    const bool isroot = (f & F_ROOT) != 0;
    const T o_t = cx.et[e];
    const bool fresh = (o_t == NI);
    const T rs_blank = (isroot || ((f & F_PROOT) && fresh)) ? T(0) : NI;
    const T ocb = cx.ecb[e], ocn = cx.ecn[e];
    T nl = cx.el[e];
    Best<T> bn{T(0), kBpNone, false}, bb{T(0), kBpNone, false};
    auto cand = [&](int sf, T scb, T scn, int sj, int kind, T p, T restart, Best<T>& best) {
      const bool has = (sf & (kind == 0 ? F_HB : F_HN)) != 0;
      const T base = has ? (kind == 0 ? scb : scn) : restart;
      best.push(base + p, has ? (((uint32_t)sj << 1) | (uint32_t)kind) : kBpRestart);
    };
    if (!isroot) {
      const T xl = row[L];
      const T p = xl - norm;
      if (pj >= 0) {
        const int pe = cx.alias[pj];
        const int pfl = cx.eflg[pe];
        const T pcb = cx.ecb[pe], pcn = cx.ecn[pe];
        const bool same = (L == cx.elab[pe]);
        const T prev = same ? cx.eb[pe] : cx.et[pe];
        nl = lse(nl, prev, cx.etab) + xl - norm;
        cand(pfl, pcb, pcn, pj, 0, p, rs_blank, bn);
        if (!same) cand(pfl, pcb, pcn, pj, 1, p, NI, bn);
        cand(f, ocb, ocn, j, 1, p, NI, bn);
      } else {
        nl += xl - norm;
        cand(f, ocb, ocn, j, 1, p, NI, bn);
      }
    }
    const T nbk = o_t + xb - norm;
    cand(f, ocb, ocn, j, 0, pbk, rs_blank, bb);
    cand(f, ocb, ocn, j, 1, pbk, NI, bb);
    const T tot = lse(nbk, nl, cx.etab);
    sp[kErNbk * WC + j] = (int)__float_as_uint(nbk);
    sp[kErNl * WC + j] = (int)__float_as_uint(nl);
    sp[kErTot * WC + j] = (int)__float_as_uint(tot);
    sp[kErCb * WC + j] = (int)__float_as_uint(bb.p);
    sp[kErCn * WC + j] = (int)__float_as_uint(bn.p);
    sp[kErBpb * WC + j] = (int)bb.bp;
    sp[kErBpn * WC + j] = (int)bn.bp;
    sp[kErFlg * WC + j] = (bb.ok ? F_HB : 0) | (bn.ok ? F_HN : 0);
    sp[kErLab * WC + j] = L;
  }
}

// CTCX_REG_SORT: Extract()'s std::sort (a beam no push changed this frame, or
// one that is not full yet) over two wave registers instead of lane 0's
// literal replay over LDS -- ctcx_regsort.h, in the one-node float LDS-tier
// kernels.  0: lit_sort as before.
#ifndef CTCX_REG_SORT
#define CTCX_REG_SORT 1
#endif
#if CTCX_REG_SORT && !defined(CTCX_GSTATE)
// ctcx_regsort.h's lane array over VGPRs: position p is lane p & 63 of
// r[p >> 6]; every index and every value that crosses lanes is wave-uniform
struct WaveLanes {
  int r0, r1, aux;
  CTCX_LDS int* out;   // the result, by position
  __device__ __forceinline__ unsigned get(int p) const {
    return (unsigned)(p < 64 ? bcast(r0, p) : bcast(r1, p - 64));
  }
  __device__ __forceinline__ void set(int p, unsigned v) {
    if (p < 64) r0 = writelane(r0, (int)v, p);
    else r1 = writelane(r1, (int)v, p - 64);
  }
  __device__ __forceinline__ uint64_t below(int reg, unsigned x) const {
    return __ballot((unsigned)(reg ? r1 : r0) < x);
  }
  __device__ __forceinline__ uint64_t above(int reg, unsigned x) const {
    return __ballot((unsigned)(reg ? r1 : r0) > x);
  }
  // The stable placement (ctcx_regsort.h): position p's element goes to its
  // key plus the number of equal keys below p.  x = key << 8 | p; for a lower
  // position q with the same key, x_q - (key << 8) = q < p, and for any other
  // key the difference is negative (wraps) or at least 256.
  __device__ __forceinline__ void finish(int n) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned key0 = (unsigned)r0 >> 16, key1 = (unsigned)r1 >> 16;
    const unsigned b0 = key0 << 8, b1 = key1 << 8;
    const int x0 = (int)(b0 | lane), x1 = (int)(b1 | (lane + 64));
    unsigned c0 = 0, c1 = 0;
    // (eight lanes a round; a position at or past n holds 0xFFFFFFFF, whose
    // x never comes out below 256 more than a member's base)
    const int n0 = n < 64 ? (n + 7) & ~7 : 64, n1 = (n + 7) & ~7;
    for (int q = 0; q < n0; q += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned xq = (unsigned)bcast(x0, q + u);
        c0 += xq - b0 < lane ? 1u : 0u;
        c1 += xq - b1 < lane + 64 ? 1u : 0u;
      }
    }
    for (int q = 64; q < n1; q += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) c1 += (unsigned)bcast(x1, q + u - 64) - b1 < lane + 64 ? 1u : 0u;
    }
    const unsigned d0 = key0 + c0, d1 = key1 + c1;   // (< n for keys that are ranks: checked all the same)
    if (lane < (unsigned)n && d0 < (unsigned)n) out[d0] = r0 & 0xFFFF;
    if (lane + 64 < (unsigned)n && d1 < (unsigned)n) out[d1] = r1 & 0xFFFF;
  }
  __device__ __forceinline__ unsigned aux_get(int i) const { return (unsigned)bcast(aux, i); }
  __device__ __forceinline__ void aux_set(int i, unsigned v) { aux = writelane(aux, (int)v, i); }
};

// std::sort of he[1..n]'s slots by their current totals into sorted[0..n), in
// registers; false (nothing stored): a NaN total or the sort's depth limit --
// the caller runs lit_sort.  Wave 0, all lanes; 1 <= n <= 128.
template <typename T>
__device__ __forceinline__ bool reg_sort_extract(const Ctx<T>& cx, const CTCX_LDS HE<T>* he, int n) {
  static_assert(sizeof(T) == 4, "float totals");
  const int lane = threadIdx.x & 63;
  const bool in0 = lane < n, in1 = lane + 64 < n;
  const int s0 = in0 ? he[lane + 1].s : 0, s1 = in1 ? he[lane + 65].s : 0;
  // (the comparator's operand: the slot's current total; past n: NaN, which
  // no comparison below counts)
  const T t0 = in0 ? cx.et[s0] : __builtin_nanf(""), t1 = in1 ? cx.et[s1] : __builtin_nanf("");
  if (__ballot((in0 && t0 != t0) || (in1 && t1 != t1))) return false;
  // key: the number of elements with a strictly greater total (eight lanes a
  // round: the rounds past n read NaN)
  int k0 = 0, k1 = 0;
  const int n0 = n < 64 ? (n + 7) & ~7 : 64, n1 = (n + 7) & ~7;
  for (int j = 0; j < n0; j += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const T tj = bcast(t0, j + u);
      k0 += tj > t0 ? 1 : 0;
      k1 += tj > t1 ? 1 : 0;
    }
  }
  for (int j = 64; j < n1; j += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const T tj = bcast(t1, j + u - 64);
      k0 += tj > t0 ? 1 : 0;
      k1 += tj > t1 ? 1 : 0;
    }
  }
  WaveLanes l;
  l.r0 = in0 ? (k0 << 16 | s0) : -1;
  l.r1 = in1 ? (k1 << 16 | s1) : -1;
  l.aux = 0;
  l.out = cx.sorted;
  return rs_sort(l, n);
}
#endif

#ifdef CTCX_SQ_CHECK
__shared__ int g_sq_dbg[8];   // (diagnostics: the first scored-field mismatch)
#endif
template <typename T, int RN, bool BIG, class SC, bool HW, bool SQ>
__device__ __forceinline__ int exact_step(Ctx<T>& cx, int buf, int nb, T norm, bool last, int P, int* n_out,
                          int* n_leaves, PhaseCtr pc, Tab tb, GQ gq, bool er_hit = false) {
  // SQ: the scored gather queue (two-wave kernels, beams <= 128, any C): with
  // the beam full, every chunk of the grow comes from the helper scored
  static_assert(!SQ || (HW && (RN == 1 || (RN == 2 && BIG))), "SQ kernels");
  uint64_t ts0 = pc ? __builtin_amdgcn_s_memtime() : 0;
  // HW: both waves run up to the recursion, then wave 1 becomes the helper;
  // wave 0 (threadIdx.x == lane) runs the rest
  const int lane = threadIdx.x & 63;
  constexpr int NT = HW ? 128 : 64;
  const int tid = threadIdx.x;
  const T NI = ninf<T>();
  const int W = cx.W;
  const int C = cx.C;
  const int blank = cx.blank;
  CTCX_LDS HE<T>* he = cx.he;

  bool bad = !(norm > NI && norm < pinf<T>());
  T xmax = NI;
  // large C: the row's maximum, its NaN / +inf test and the per 64-label block
  // maxima (bounds for window skipping in the grow loop below, in LDS after
  // the row) come from the pre-pass (ctcx_row_prep, loaded with the row)
  [[maybe_unused]] CTCX_LDS T* bmax = row_bmax(cx);
  if constexpr (BIG) {   // BIG <=> C > 64
    bad |= cx.rbad != 0;
    xmax = cx.rxmax;
  } else {
    for (int j = lane; j < C; j += 64) {
      const T xv = cx.row[j];
      bad |= (xv != xv) || (xv == pinf<T>());
      xmax = xv > xmax ? xv : xmax;
    }
    xmax = wave_max(xmax);
  }
  if (__ballot(bad)) return 1;
  // max_l (x_l - norm): float rounding is monotone, so pmax + base bounds
  // every offer's score p + base computed the reference's way
  const T pmax = xmax - norm;

  // The frame's first chunk beside the recursion (kEarlyChunk0; small-C scored
  // float kernels, beam full: where the helper gathers at all).  Chunk 0 reads
  // only the frame-start arrays, the row and norm, and the recursion writes
  // only the e* arrays, so the helper starts its gather here, from a bottom of
  // -inf, while wave 0 rolls and recurses every branch itself (lanes over i and
  // i + 64: recurse_branch(i), not literal, reads the frame-start arrays, the
  // row and entry i's own words, which the same lane has just rolled).
  // Workgroup barriers executed inside exact_step, per path (nb is uniform
  // over the workgroup, and the row test above is decided alike by both
  // waves; a mismatch between the waves would be a hang):
  //                                  wave 0   wave 1
  //   bad row (return 1 above)         0        0
  //   early path (nb >= W)             0        0     <- neither runs the two below
  //   ... its recursion in place       0        0     (kEarlyRecurse, er_hit: wave 0 skips
  //                                                    recurse_wave0, which has no barrier)
  //   every other path                 2        2
  // kEarlyRecurse adds no barrier and no wait anywhere: the helper stages
  // between its ranks and the barrier that follows exact_step in the frame
  // loop, the commit places between two of its own barriers, and both read
  // their go-ahead (erw[kErT], er_place, er_hit) as workgroup-uniform values
  // written before a barrier both waves have passed.
  // A non-finite total on the early path: wave 0 returns 1 alone; the helper,
  // already in its loop, leaves through the kCtlDone the kernel stores next.
  constexpr bool kEc0 = kEarlyChunk0 && HW && SQ && !BIG && RN == 1 && sizeof(T) == 4 && !SC::kStateful;
  bool early = false;
  if constexpr (kEc0) early = nb >= W;
  if (kEc0 && early) {
    if constexpr (kEc0) {
      if (helper_wave()) {
        help_gather_scored<T, BIG, true>(cx, gq, buf, nb, norm, pmax, NI);
        if constexpr (kExtRank) {
          [[maybe_unused]] const uint64_t hr0 = CTCX_HTIME();
          help_rank_extract<T>(cx, buf);
          CTCX_HPC(cx, 28, CTCX_HTIME() - hr0);
        }
        return 0;   // the kernel takes wave 0's result
      }
      // (kEarlyRecurse, er_hit: the last commit put this frame's recursion in
      // place, from the helper's staging; uniform over the workgroup)
      if (!(kEarlyRecurse && er_hit)) recurse_wave0<T, SC>(cx, buf, nb, norm);
    }
  } else {
    // roll (decoder.h:87-92) + recursion (decoder.h:95-143), threads over branches
    for (int i = tid; i < nb; i += NT) {
      cx.et[i] = sel(cx.ot, buf)[i]; cx.eb[i] = sel(cx.ob, buf)[i]; cx.el[i] = sel(cx.ol, buf)[i];
      cx.eflg[i] = 0;
      cx.bst[i] = 0;
      cx.bloom[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < nb; i += NT) recurse_branch<T, SC>(cx, buf, i, i, norm, false);
    __syncthreads();
  }
  bool nonfinite = false;
  T lmin = pinf<T>();   // (the smallest leaf: the bottom of a full beam)
  for (int i = lane; i < nb; i += 64) {   // (HW: each wave tests every branch, so both decide alike)
    const T v = cx.et[i];
    nonfinite |= !(v > NI && v < pinf<T>());
    lmin = v < lmin ? v : lmin;
    if (!HW || tid < 64) he_st(he, i + 1, HE<T>{v, i});     // leaves_.push(b) in branch order
  }
  if (__ballot(nonfinite)) return 1;
  if constexpr (HW) {
    if (helper_wave()) {
      if constexpr (SQ) {
        // (kEc0: a full beam took the early path above, so this call is never
        // reached there.  Compiling it out was measured: the kernel is 2 KB
        // shorter and cfg3 1.5% slower, 116.1 against 114.4 ms per step --
        // placement; profiles/r16_ab_prefetch_cfg3.txt.  It stays.)
        if (nb >= W) help_gather_scored<T, BIG>(cx, gq, buf, nb, norm, pmax, wave_min(lmin));
        if constexpr (RN == 1 && kExtRank && !BIG) {
          [[maybe_unused]] const uint64_t hr0 = CTCX_HTIME();
          help_rank_extract<T>(cx, buf);
          CTCX_HPC(cx, 28, CTCX_HTIME() - hr0);
        }
      } else if constexpr (BIG) {
        // how far ahead of wave 0 the helper gathers (at most kQSlots chunks):
        // a chunk gathered early carries offers a later bottom rejects, and at
        // beams of <= 128 wave 0 runs those chunks faster than the helper
        // gathers, so one ahead is best there (cfg4 179.3 -> 165.2 ms per
        // launch, same box); beams of 129..256 gain from the full lead (cfg5:
        // 1434 ms at 4 ahead, 1437 at 2, 1454 at 1)
        if (nb >= W) help_gather_chunks<T>(cx, gq, buf, nb, norm, pmax, wave_min(lmin), RN == 1 ? 1 : kQSlots);
      } else {
        help_score_chunks<T>(cx, tb, buf, nb, norm);
      }
      return 0;   // the kernel takes wave 0's result
    }
  } else {
    __syncthreads();
  }

  uint64_t ts1 = pc ? __builtin_amdgcn_s_memtime() : 0;
  if (pc) pc[1] += ts1 - ts0;
  int n = nb;                     // elements_.size()
  // Child slots come from a bump allocator; a new child reuses the slot of the
  // child entry it evicts.  A bump happens for an append before the beam is
  // full (<= W - nb) or when the evicted entry is a branch's (a branch is
  // evicted at most twice: it re-enters only through its one (parent, label)
  // offer), so slots stay below W + 2 nb <= 3W < enc.
  int nextfree = nb;
  int st = kTopUnordered;
  bool full = (n >= W);
  HE<T> front;                    // elements_[0] once BOTTOM_KNOWN / HEAP (uniform, in VGPRs)
  front.v = NI;
  front.s = 0;
  if (full) {                     // branch 0's is_candidate() peeks
    front = wave_first_min_to_front(he, n);
    st = kTopBottomKnown;
    // (kEarlyChunk0: the helper, gathering since before the recursion, waits
    // for this starting bottom before its second chunk)
    if constexpr (kEc0)
      if (early)
        __hip_atomic_store(&cx.misc[kCtlBot], (int)__builtin_bit_cast(unsigned, (float)front.v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  T bottom = full ? front.v : NI;

  // grow (decoder.h:146-209): offers in (branch order, label order), 64 per
  // chunk.  Within a chunk the entry writes, the resets of evicted branch
  // entries and the S_EVICT / S_DEACT flags are kept in registers (myslot, the
  // record list evr/nev) and flushed by all lanes at the chunk's end: nothing
  // reads them before then, and an event then costs no divergent stores.
  // Branch turns (decoder.h:151-159): once the beam is full, branch b is
  // skipped iff b.old.total <= bottom at the moment its turn starts; branches
  // come in descending total and bottom only rises, so the first skipped
  // branch ends the grow.  A chunk can hold the starts of several branches:
  // each lane carries the bottom at its branch's start (bat); a skipped turn
  // can only show through a re-offer (a skipped branch's new children score
  // <= its total <= bottom), so only re-offers consult it, and the turn that
  // continues into the next chunk is checked at the chunk's end.
  // Skipping (ours, exact): with the beam full, an offer whose child is new and
  // whose score is <= bottom is rejected without effect, and an offer whose
  // child is an active branch is skipped by the reference too; only a re-offer
  // of an evicted branch-child has an effect (deactivation).  bloom flags the
  // labels that may be such re-offers, so the rest of a branch with
  // pmax + ot <= bottom and no flagged label, or a chunk without any score >
  // bottom or flagged lane, is skipped whole (what matters at large C).
  const int Cm1 = C - 1;
  const float rcp = 1.0f / (float)Cm1;
  const int q128 = 128 / Cm1, r128 = 128 - q128 * Cm1;   // a window's 128 offers in (branch, label index)
  int i0 = 0, li0 = 0;   // the chunk's first offer: branch i0, label index li0
  bool stop = false;
  // large C (compacted chunks): the gathered offers, the span's first offer,
  // a closed turn found by the gather, the branch whose children the bitmap holds
  int cqn = 0, cq_i0 = 0, cq_l0 = 0, cbr = -1;
  bool gstop = false;
  bool dz = false;           // a branch was deactivated this frame (HW window loop: bst then read)
  int gqc = 0;               // HW, large C: chunks taken from the gather queue
  uint32_t gqe = 0, gqp = 0; // ... this chunk's entry of the lane and of the lane before
  u32x4 gqa{};               // SQ: this lane's scored offer
  float gqv = 0.0f;          // ... its candidate value
  // |S|, the row's top set, and the largest value outside S (pre-pass; for
  // double rows |S| = 0 and the S path below is never taken)
  const int tsn = BIG ? cx.rns : 0;
  const T txo = BIG ? cx.rxout : NI;
  // The scored queue at small C (float, base scorer): once the beam is a heap
  // (the chunk that fills it goes by the generic path below), the rest of the
  // frame's grow is scored chunks only, and they run as one loop of their own,
  // as the windows do: the heap's geometry and addresses are set up once per
  // frame, the front and the bump pointer stay in registers from chunk to
  // chunk, and a chunk is its hand-over read, the unpack (the turn-start lane
  // comes packed: sq_pack_sl), the events and the flush, with none of the
  // generic chunk path's state around them.  Same decisions, pushes, slots,
  // records and published bottoms as that path, chunk for chunk; the bounded
  // wait, a dead helper and the re-offers of branch children are its code.
  constexpr bool kSqHeapM = SQ && HW && !BIG && RN == 1 && sizeof(T) == 4;
  constexpr bool kSqLoop = kSqHeapM && !SC::kStateful;
  while (i0 < nb && !stop) {
    if constexpr (kSqLoop) {
      if (full && st == kTopHeap && W >= 2) {
        const auto geo = mask_geo<RN>(cx.hdum);
        const unsigned heb = (unsigned)(uintptr_t)he;   // LDS byte address of he[0]
        const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
        const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(cx.hdum + lane);
        T fv = front.v;
        int fs = front.s;
        int nfree = nextfree;
        while (!stop) {
          // the next chunk of the helper's queue: the published count first,
          // the slot's words in the same batch
          const int slot = gqc & gq.sm;
          int h0 = 0, h3 = 0;
          auto read_slot = [&]() {
            h0 = gq.h[slot * 4 + 0]; h3 = gq.h[slot * 4 + 3];
            gqa = gq.a[slot * 64 + lane];
            gqv = gq.p[slot * 64 + lane];
          };
          {
            int rdy = __hip_atomic_load(&cx.misc[kCtlReady], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __asm__ volatile("" ::: "memory");
            read_slot();
            __asm__ volatile("" ::"v"(h0), "v"(h3), "v"(gqa), "v"(gqv));
            if (__builtin_expect(uni(rdy) <= gqc && !cx.tabdead, 0)) {
              // the helper is behind: the bounded wait of the generic path (a
              // wait that runs out, or a helper that gave up, ends the grow)
              uint64_t tw = 0;
              const uint64_t tq0 = pc ? __builtin_amdgcn_s_memtime() : 0;
              int spins = 0;
              for (int spin = 0;; ++spin) {
                spins = spin + 1;
                __builtin_amdgcn_s_sleep(CTCX_SLEEP);
                if (ctl_ld(cx.misc, kCtlReady) > gqc) break;
                if (ctl_ld(cx.misc, kCtlDead) != 0 || wait_expired(spin, tw)) {   // never in a correct run
                  cx.tabdead = 1;
                  __hip_atomic_store(&cx.misc[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                  break;
                }
              }
              __asm__ volatile("" ::: "memory");
              read_slot();
              if (pc) {
                (void)uni((int)h0);
                pc[19] += __builtin_amdgcn_s_memtime() - tq0;
                pc[20] += spins;
#ifdef CTCX_PHASE_LATE   // (how late the chunk was: from this ask to wave 0 seeing it published)
                pc[kPhLateWait + (gqc < 15 ? gqc : 15)] += __builtin_amdgcn_s_memtime() - tq0;
                pc[kPhLateCnt + (gqc < 15 ? gqc : 15)] += 1;
#endif
              }
            }
#ifdef CTCX_PHASE_LATE
            if (pc) pc[kPhLateAsk + (gqc < 15 ? gqc : 15)] += 1;
#endif
          }
          __asm__ volatile("" ::: "memory");
          ++gqc;
          __hip_atomic_store(&cx.misc[kCtlCons], gqc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          cqn = cx.tabdead ? 0 : uni(h0);
          gstop = uni(h3) != 0;
          if (cqn == 0) {
            if (gstop) stop = true;
            break;
          }
          const uint64_t tc0 = pc ? __builtin_amdgcn_s_memtime() : 0;
          const bool valid = lane < cqn;
          const uint32_t ax = gqa.x, ay = gqa.y, az = gqa.z, aw = gqa.w;   // (scalar copies: see the generic path)
          const uint32_t pk = valid ? az : 0u;
          const int i = (int)(pk & 255u);
          const int c = (int)((pk >> 8) & 511u) - 1;
          const int l = sq_label_small(pk);
          const int sl = sq_turn_lane(pk);
          const T s = (T)__builtin_bit_cast(float, ax);
          const T bt = (T)__builtin_bit_cast(float, ay);
          const bool isbc = c >= 0;
          const uint64_t isbm = __ballot(isbc);
          // what events change: the branch deactivated (read only after a
          // deactivation this frame), the branch child evicted
          bool live = valid;
          if (dz) live = live && !(cx.bst[i] & S_DEACT);
          bool cev = false;
          if (isbm) cev = isbc && (cx.bst[isbc ? c : i] & S_EVICT);
          T bat = sl > 0 ? fv : NI;
          const uint64_t startsM = __ballot(valid && sl == lane && lane != 0);   // branch turns starting mid-chunk
          if (pc) pc[10] += __builtin_amdgcn_s_memtime() - tc0;
          if (!__ballot(live && ((s > fv) | (isbc && cev)))) {
            if (startsM & ~__ballot(bt > fv)) break;   // no event here: every start sees this bottom
            if (gstop) break;
            continue;
          }
          const uint64_t tc1 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (pc) { pc[8] += tc1 - tc0; pc[11] += 1; }
          int myslot = -1;   // slot of this lane's accepted offer (-1: none, or evicted again)
          int evr = 0;       // record nv-th: evicted branch slot, or kDeactRec | rejected branch
          int nv = 0;
          uint64_t done = 0;
          const uint64_t liveM = __ballot(live);
          uint64_t NC = liveM & ~isbm, LB = liveM & isbm, RB = LB & __ballot(cev);
          for (;;) {
            int k;
            fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv);
            int nev_asm = 0;
            const uint64_t ta = pc ? __builtin_amdgcn_s_memtime() : 0;
            const int est = heap_events_f32(s, c, sl, geo.anc, geo.req, aj, al, ar, dum, myslot, evr, bat, NC, RB, done,
                                            LB, fv, fs, nfree, nv, uni(nb), k, nev_asm);
            if (pc) { pc[13] += __builtin_amdgcn_s_memtime() - ta; pc[6] += uni(nev_asm); pc[12] += 1; }
            if (est == 0) break;
            k = uni(k);
            // lane k re-offers a branch child: was k's turn skipped?
            const uint64_t gtM = __ballot(s > fv);
            const uint64_t m = ((gtM & NC) | RB) & ~done;   // its lowest lane is k
            if ((__ballot(!(bt > bat)) >> k) & 1ull) {
              const uint64_t keepM = lowmask(bcast(sl, k));   // that branch and every later one
              NC &= keepM; LB &= keepM; RB &= keepM;
              stop = true;
              continue;
            }
            done = m ^ (m - 1ull);
            const int kc = bcast(c, k);
            if (!((gtM >> k) & 1ull)) {
              // re-offered evicted branch rejected -> deactivated (decoder.h:200-205)
              evr = writelane(evr, kc | kDeactRec, nv);
              dz = true;
              nv += 1;
              const uint64_t dm = ~__ballot(i == kc);
              NC &= dm; LB &= dm; RB &= dm;
              continue;
            }
            // accepted: the branch's entry keeps its slot
            if (fs < nb) {
              evr = writelane(evr, fs, nv);
              nv += 1;
              RB |= LB & __ballot(c == fs);
            }
            const T k_s = bcast(s, k);
            myslot = (myslot == fs) ? -1 : myslot;
            myslot = __builtin_amdgcn_inverse_ballot_w64(1ull << k) ? kc : myslot;
            MPairs<T, RN> pp;
            mpairs<T, RN>(he, geo, pp);
            T c0;
            int s0;
            bool keep;
            mpush<T, RN>(he, geo, k_s, kc, pp, c0, s0, keep);
            fv = keep ? k_s : c0;
            fs = keep ? kc : s0;
            bat = (sl > k) ? fv : bat;
          }
          // the turn continuing into the next chunk: skipped -> so is every later one
          if ((__ballot(valid && !(bt > bat)) >> (cqn - 1)) & 1ull) stop = true;
          if (gstop) stop = true;
          // flush: resets and flags first, then the surviving accepted entries
          const uint64_t q5 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (lane < nv) {
            const int rs = evr & ~kDeactRec;
            if (evr & kDeactRec) {
              __hip_atomic_fetch_or(&cx.bst[rs], S_DEACT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
              cx.et[rs] = NI; cx.eb[rs] = NI; cx.el[rs] = NI; cx.eflg[rs] = 0;
              __hip_atomic_fetch_or(&cx.bst[rs], S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          if (myslot >= 0) {
            cx.et[myslot] = s; cx.eb[myslot] = NI; cx.el[myslot] = s;
            cx.ecn[myslot] = (T)gqv; cx.ebpn[myslot] = aw;
            cx.eflg[myslot] = F_HN;
            cx.ekind[myslot] = isbc ? ((uint32_t)c << 1) : (((uint32_t)i << 1) | 1u);
            cx.elab[myslot] = l;
            if (isbc) __hip_atomic_fetch_and(&cx.bst[c], ~S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          // the helper gathers the next chunks against this bottom
          __hip_atomic_store(&cx.misc[kCtlBot], (int)__builtin_bit_cast(unsigned, (float)fv), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
          if (pc) pc[15] += __builtin_amdgcn_s_memtime() - q5;
          if (pc) pc[9] += __builtin_amdgcn_s_memtime() - tc1;
        }
        front.v = fv;
        front.s = fs;
        bottom = fv;
        nextfree = nfree;
        break;
      }
    }
    if constexpr (RN == 1 && !BIG && sizeof(T) == 4 && !SC::kStateful && !SQ) {
      if (st == kTopHeap && W >= 2) {
        // the windows run as one loop of their own (each window ends with the
        // grow's state in registers; the generic chunk path's loop-carried
        // state stays out of it): from here on the frame's grow is windows only
#define CTCX_WIN_HALF(H, O)                                                                                       \
          for (;;) {                                                                                                \
            int k, cnt = 0;                                                                                         \
            fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv);                                           \
            const uint64_t ta = pc ? __builtin_amdgcn_s_memtime() : 0;                                              \
            const int est = heap_events2_f32<H == 0>(sw[H], cw[H], slw[H] - 64 * H, cw[O], slw[O] - 64 * H,      \
                                                     geo.anc, geo.req, aj,                                         \
                                                     al, ar, dum, mys[H], mys[O], evr, batw[H], batw[O], NCw[H],   \
                                                     RBw[H], RBw[O], donew[H], LBw[H], LBw[O], fv, fs, nfree, nv,  \
                                                     uni(nb), 64 * H, k, cnt);                                     \
            if (pc) { pc[13] += __builtin_amdgcn_s_memtime() - ta; pc[6] += uni(cnt); pc[12] += 1; }             \
            if (est == 0) break;                                                                                    \
            k = uni(k);                                                                                             \
            const uint64_t gtM = __ballot(sw[H] > fv);                                                             \
            const uint64_t m = ((gtM & NCw[H]) | RBw[H]) & ~donew[H];                                              \
            if ((__ballot(!(bt[H] > batw[H])) >> k) & 1ull) {                                                      \
              const int ksl = bcast(slw[H], k);                                                                     \
              const uint64_t km0 = lowmask(ksl), km1 = ksl > 64 ? lowmask(ksl - 64) : 0ull;                        \
              NCw[0] &= km0; LBw[0] &= km0; RBw[0] &= km0;                                                          \
              NCw[1] &= km1; LBw[1] &= km1; RBw[1] &= km1;                                                          \
              stop = true;                                                                                          \
              continue;                                                                                             \
            }                                                                                                       \
            donew[H] = m ^ (m - 1ull);                                                                              \
            const int kc = bcast(cw[H], k);                                                                         \
            if (!((gtM >> k) & 1ull)) {                                                                             \
              evr = writelane(evr, kc | kDeactRec, nv);                                                             \
              dz = true;                                                             \
              nv += 1;                                                                                              \
              const uint64_t dm0 = ~__ballot(wi[0] == kc), dm1 = ~__ballot(wi[1] == kc);                            \
              NCw[0] &= dm0; LBw[0] &= dm0; RBw[0] &= dm0;                                                          \
              NCw[1] &= dm1; LBw[1] &= dm1; RBw[1] &= dm1;                                                          \
              continue;                                                                                             \
            }                                                                                                       \
            if (fs < nb) {                                                                                          \
              evr = writelane(evr, fs, nv);                                                                         \
              nv += 1;                                                                                              \
              RBw[0] |= LBw[0] & __ballot(cw[0] == fs);                                                             \
              RBw[1] |= LBw[1] & __ballot(cw[1] == fs);                                                             \
            }                                                                                                       \
            const T k_s = bcast(sw[H], k);                                                                          \
            mys[0] = (mys[0] == fs) ? -1 : mys[0];                                                                  \
            mys[1] = (mys[1] == fs) ? -1 : mys[1];                                                                  \
            mys[H] = __builtin_amdgcn_inverse_ballot_w64(1ull << k) ? kc : mys[H];                                 \
            HE<T> pL, pR;                                                                                           \
            pairs_m(he, geo, pL, pR);                                                                               \
            T c0;                                                                                                   \
            int s0;                                                                                                 \
            bool keep;                                                                                              \
            push_m<T>(he, geo, k_s, kc, pL, pR, c0, s0, keep);                                                      \
            fv = keep ? k_s : c0;                                                                                   \
            fs = keep ? kc : s0;                                                                                    \
            const int kp = k + 64 * H;                                                                              \
            batw[0] = (slw[0] > kp) ? fv : batw[0];                                                                 \
            batw[1] = (slw[1] > kp) ? fv : batw[1];                                                                 \
          }
        if constexpr (HW) {
        const int nch = (nb * Cm1 + 63) >> 6;   // the frame's chunks
        int ch = (i0 * Cm1 + li0) >> 6;
        // the chunks before this one went by the generic path: their slots are free
        __hip_atomic_store(&cx.misc[kCtlCons], ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        // the helper gave up in an earlier frame: no table slot is used again
        // (inside the loop tabdead only turns on in the wait below, which
        // then ends the grow)
        if (cx.tabdead) stop = true;
        if (!stop) do {
          const uint64_t tc0 = pc ? __builtin_amdgcn_s_memtime() : 0;
          const bool turnw = (li0 == 0);
          const int c = ch;   // the window's first chunk (the generic chunks before it were 64 offers each)
          ch += 2;
          i0 += q128;   // 128 offers on: (i0, li0) + (q128, r128), one carry
          li0 += r128;
          if (li0 >= Cm1) { li0 -= Cm1; ++i0; }
          // the window's two chunks from the score table: the published
          // count is read first, so the slot reads issued after it see every
          // chunk it covers (one wave's LDS operations execute in order)
          const int need = c + 2 < nch ? c + 2 : nch;
          u32x4 ta[2];
          float tpv[2];
          const uint64_t tq0 = pc ? __builtin_amdgcn_s_memtime() : 0;
          int spins = 0;
          const int s0 = (c % kTabSlots) * 64 + lane, s1 = ((c + 1) % kTabSlots) * 64 + lane;
          {
            // one batch of reads, no loop around it (a loop would make the
            // compiler wait out every read's predecessor: write-after-write on
            // the same registers across the back edge)
            int rdy = __hip_atomic_load(&cx.misc[kCtlReady], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __asm__ volatile("" ::: "memory");
            ta[0] = tb.a[s0];
            tpv[0] = tb.p[s0];
            ta[1] = tb.a[s1];
            tpv[1] = tb.p[s1];
            // the slot reads complete with the count (one round trip): otherwise
            // the compiler sinks them below the test, or hoists the count's
            // readfirstlane above them -- a second round trip either way
            __asm__ volatile("" ::"v"(ta[0]), "v"(ta[1]), "v"(tpv[0]), "v"(tpv[1]));
            if (__builtin_expect(uni(rdy) < need, 0)) {
              // wave 1 is behind (rare): wait for the count, then read again.
              // A wait that runs out of time, or a helper that gave up, ends
              // this frame's grow here and every later frame's at its first
              // window: the table's slots are never used then (the host
              // decodes the call again with the one-wave kernel, or fails it)
              uint64_t tw = 0;
              for (int spin = 0;; ++spin) {
                spins = spin + 1;
                __builtin_amdgcn_s_sleep(CTCX_SLEEP);
                if (ctl_ld(cx.misc, kCtlReady) >= need) break;
                if (ctl_ld(cx.misc, kCtlDead) != 0 || wait_expired(spin, tw)) {   // never in a correct run
                  cx.tabdead = 1;
                  __hip_atomic_store(&cx.misc[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                  break;
                }
              }
              if (cx.tabdead) {
                stop = true;
                break;
              }
              __asm__ volatile("" ::: "memory");
              ta[0] = tb.a[s0];
              tpv[0] = tb.p[s0];
              ta[1] = tb.a[s1];
              tpv[1] = tb.p[s1];
            }
          }
          __asm__ volatile("" ::: "memory");
          __hip_atomic_store(&cx.misc[kCtlCons], c + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (pc) {   // diagnostics: the table wait (its s_sleep rounds)
            (void)uni((int)ta[1].x);
            pc[19] += __builtin_amdgcn_s_memtime() - tq0;
            pc[20] += spins;
          }
          // per-lane fields, then every per-lane predicate as a wave mask (SGPRs)
          int wi[2], wl[2], slw[2], cw[2];
          T sw[2], bt[2], batw[2];
          Best<T> cdw[2];
          uint64_t wvM[2], stM[2], bcM[2], wantM[2];
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned x = (h == 0 || c + 1 < nch) ? (unsigned)ta[h].z : 0u;
            const unsigned a0 = ta[h].x, a1 = ta[h].y, a3 = ta[h].w;
            wi[h] = (int)(x & 127u);
            wl[h] = (int)((x >> 7) & 63u);
            const int wli = (int)((x >> 13) & 63u);
            cw[h] = (int)((x >> 19) & 255u) - 1;
            sw[h] = __builtin_bit_cast(float, a0);
            bt[h] = __builtin_bit_cast(float, a1);
            cdw[h] = Best<T>{(T)tpv[h], a3, true};
            slw[h] = lane + 64 * h - wli;   // window position where the lane's branch turn starts
            batw[h] = slw[h] > 0 ? bottom : NI;
            wvM[h] = __ballot((x >> 27) & 1u);
            bcM[h] = __ballot((x >> 19) & 255u);   // the offer re-offers a branch child
            stM[h] = wvM[h] & __ballot(wli == 0) & (h == 0 ? ~1ull : ~0ull);
          }
          if (turnw && !(bcast(bt[0], 0) > bottom)) break;   // branch i0's turn: skipped, and all later
          // what events change: the offer's branch deactivated (read only after a
          // deactivation this frame), its branch child evicted (read only when
          // the window re-offers a branch child: a few windows per frame)
          uint64_t dM[2] = {0ull, 0ull}, eM[2] = {0ull, 0ull};
          if (dz) {
  #pragma unroll
            for (int h = 0; h < 2; ++h) dM[h] = __ballot(cx.bst[wi[h]] & S_DEACT);
          }
          if (bcM[0] | bcM[1]) {
  #pragma unroll
            for (int h = 0; h < 2; ++h) eM[h] = bcM[h] & __ballot(cx.bst[cw[h] >= 0 ? cw[h] : wi[h]] & S_EVICT);
          }
          uint64_t NCw[2], LBw[2], RBw[2], donew[2] = {0ull, 0ull};
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint64_t liveM = wvM[h] & ~dM[h];
            NCw[h] = liveM & ~bcM[h];
            LBw[h] = liveM & bcM[h];
            RBw[h] = LBw[h] & eM[h];
            wantM[h] = (NCw[h] & __ballot(sw[h] > bottom)) | RBw[h];
          }
          if (pc) pc[10] += __builtin_amdgcn_s_memtime() - tc0;
          if (!(wantM[0] | wantM[1])) {
            if ((stM[0] & ~__ballot(bt[0] > bottom)) | (stM[1] & ~__ballot(bt[1] > bottom))) break;
            continue;
          }
          const uint64_t tc1 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (pc) { pc[8] += tc1 - tc0; pc[11] += 1; }
          int mys[2] = {-1, -1};
          int evr = 0, nv = 0;
          T fv = front.v;
          int fs = front.s;
          int nfree = nextfree;
          const HeapM geo = heap_m(cx.hdum);
          const unsigned heb = (unsigned)(uintptr_t)he;
          const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
          const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(cx.hdum + lane);
          // the events of half H (other half O); rare ones (re-offered branch
          // children) are decided here, as in the chunk loop below
          CTCX_WIN_HALF(0, 1)
          donew[0] = ~0ull;   // the first half's offers are all behind
          CTCX_WIN_HALF(1, 0)
          front.v = fv;
          front.s = fs;
          bottom = fv;
          nextfree = nfree;
          // the turn continuing into the next window: skipped -> so is every later one
          if (((wvM[1] & ~__ballot(bt[1] > batw[1])) >> 63) & 1ull) stop = true;
          const uint64_t q5 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (lane < nv) {
            const int rs = evr & ~kDeactRec;
            if (evr & kDeactRec) {
              __hip_atomic_fetch_or(&cx.bst[rs], S_DEACT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
              cx.et[rs] = NI; cx.eb[rs] = NI; cx.el[rs] = NI; cx.eflg[rs] = 0;
              __hip_atomic_fetch_or(&cx.bst[rs], S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              // (no bloom: the window path reads the events' effects from bst)
            }
          }
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ms = mys[h];
            if (ms >= 0) {
              const bool isbc = cw[h] >= 0;
              cx.et[ms] = sw[h]; cx.eb[ms] = NI; cx.el[ms] = sw[h];
              cx.ecn[ms] = cdw[h].p; cx.ebpn[ms] = cdw[h].bp;
              cx.eflg[ms] = F_HN;
              cx.ekind[ms] = isbc ? ((uint32_t)cw[h] << 1) : (((uint32_t)wi[h] << 1) | 1u);
              cx.elab[ms] = wl[h];
              if (isbc) __hip_atomic_fetch_and(&cx.bst[cw[h]], ~S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          if (pc) pc[15] += __builtin_amdgcn_s_memtime() - q5;
          if (pc) pc[9] += __builtin_amdgcn_s_memtime() - tc1;
        } while (i0 < nb && !stop);
        } else {
        do {
          // ---- HEAP_SORTED, C <= 64, float: 128-offer windows (two halves of
          // 64 lanes).  The same offer semantics as the 64-offer chunk below,
          // with window positions 0..127 in place of lanes: one batch of reads,
          // one skip test, one child walk and one flush per window, and the
          // events of the first half, then the second, in one register state.
          const uint64_t tc0 = pc ? __builtin_amdgcn_s_memtime() : 0;
          const bool turnw = (li0 == 0);
          int wi[2], wli[2], wl[2];
          bool wv[2];
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int x = li0 + lane + 64 * h;
            int q = (int)((float)x * rcp);
            q -= (q * Cm1 > x) ? 1 : 0;
            q += ((q + 1) * Cm1 <= x) ? 1 : 0;
            const int iv = i0 + q;
            wv[h] = iv < nb;
            wi[h] = wv[h] ? iv : i0;
            wli[h] = wv[h] ? x - q * Cm1 : 0;
            wl[h] = wli[h] + (wli[h] >= blank ? 1 : 0);
          }
          i0 += q128;   // 128 offers on: (i0, li0) + (q128, r128), one carry
          li0 += r128;
          if (li0 >= Cm1) { li0 -= Cm1; ++i0; }
          int bl[2], bflg[2], bsti[2], hd[2];
          T bt[2], bob[2], bcb[2], bcn[2], xl[2];
          uint64_t blm[2];
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ii = wi[h];
            bl[h] = sel(cx.lab, buf)[ii];
            bflg[h] = sel(cx.flg, buf)[ii];
            bt[h] = sel(cx.ot, buf)[ii];
            bob[h] = sel(cx.ob, buf)[ii];
            bsti[h] = cx.bst[ii];
            blm[h] = cx.bloom[ii];
            hd[h] = cx.head[ii];
            bcb[h] = sel(cx.cb, buf)[ii];
            bcn[h] = sel(cx.cn, buf)[ii];
            xl[h] = cx.row[wl[h]];
          }
          if (turnw && !(bcast(bt[0], 0) > bottom)) break;   // branch i0's turn: skipped, and all later
          bool wlive[2];
          T sw[2], pw[2], batw[2];
          int slw[2];
          uint64_t stM[2], wantM[2];
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            wlive[h] = wv[h] && !(bsti[h] & S_DEACT);
            pw[h] = xl[h] - norm;
            sw[h] = pw[h] + ((wl[h] == bl[h]) ? bob[h] : bt[h]);
            slw[h] = lane + 64 * h - wli[h];   // window position where the lane's branch turn starts
            batw[h] = slw[h] > 0 ? bottom : NI;
            stM[h] = __ballot(wv[h] && wli[h] == 0 && lane + 64 * h != 0);
            wantM[h] = __ballot(wlive[h] && ((sw[h] > bottom) | (((blm[h] >> (wl[h] & 63)) & 1ull) != 0)));
          }
          if (pc) pc[10] += __builtin_amdgcn_s_memtime() - tc0;
          if (!(wantM[0] | wantM[1])) {
            if ((stM[0] & ~__ballot(bt[0] > bottom)) | (stM[1] & ~__ballot(bt[1] > bottom))) break;
            continue;
          }
          int cw[2] = {-1, -1};
          {
            const uint64_t tw0 = pc ? __builtin_amdgcn_s_memtime() : 0;
            int k0 = wlive[0] ? hd[0] : -1, k1 = wlive[1] ? hd[1] : -1;
            while (__ballot(k0 >= 0 || k1 >= 0)) {
              if (pc) pc[17] += 1;
              int n0 = -1, n1 = -1;
              if (k0 >= 0) {
                const int lk = sel(cx.lab, buf)[k0];
                const int sk = cx.sib[k0];
                if (lk == wl[0]) cw[0] = k0;
                else n0 = sk;
              }
              if (k1 >= 0) {
                const int lk = sel(cx.lab, buf)[k1];
                const int sk = cx.sib[k1];
                if (lk == wl[1]) cw[1] = k1;
                else n1 = sk;
              }
              k0 = n0;
              k1 = n1;
            }
            if (pc) pc[18] += __builtin_amdgcn_s_memtime() - tw0;
          }
          Best<T> cdw[2];
          uint64_t NCw[2], LBw[2], RBw[2], donew[2] = {0ull, 0ull};
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool isbc = cw[h] >= 0;
            bool cev = false, recv_fresh = true;
            if (isbc) {   // the offer's child is a branch (few lanes, most windows none): its state
              cev = (cx.bst[cw[h]] & S_EVICT) != 0;
              recv_fresh = sel(cx.ot, buf)[cw[h]] == NI;
            }
            const T rs_blank = ((bflg[h] & F_ROOT) && recv_fresh) ? T(0) : NI;
            cdw[h] = Best<T>{T(0), kBpNone, false};
            cdw[h].push(((bflg[h] & F_HB) ? bcb[h] : rs_blank) + pw[h],
                        (bflg[h] & F_HB) ? (((uint32_t)wi[h] << 1) | 0u) : kBpRestart);
            if (wl[h] != bl[h])
              cdw[h].push(((bflg[h] & F_HN) ? bcn[h] : NI) + pw[h],
                          (bflg[h] & F_HN) ? (((uint32_t)wi[h] << 1) | 1u) : kBpRestart);
            const uint64_t liveM = __ballot(wlive[h]), isbm = __ballot(isbc);
            NCw[h] = liveM & ~isbm;
            LBw[h] = liveM & isbm;
            RBw[h] = LBw[h] & __ballot(cev);
          }
          const uint64_t tc1 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (pc) { pc[8] += tc1 - tc0; pc[11] += 1; }
          int mys[2] = {-1, -1};
          int evr = 0, nv = 0;
          T fv = front.v;
          int fs = front.s;
          int nfree = nextfree;
          const HeapM geo = heap_m(cx.hdum);
          const unsigned heb = (unsigned)(uintptr_t)he;
          const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
          const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(cx.hdum + lane);
          // the events of half H (other half O); rare ones (re-offered branch
          // children) are decided here, as in the chunk loop below
          CTCX_WIN_HALF(0, 1)
          donew[0] = ~0ull;   // the first half's offers are all behind
          CTCX_WIN_HALF(1, 0)
          front.v = fv;
          front.s = fs;
          bottom = fv;
          nextfree = nfree;
          // the turn continuing into the next window: skipped -> so is every later one
          if ((__ballot(wv[1] && !(bt[1] > batw[1])) >> 63) & 1ull) stop = true;
          const uint64_t q5 = pc ? __builtin_amdgcn_s_memtime() : 0;
          if (lane < nv) {
            const int rs = evr & ~kDeactRec;
            if (evr & kDeactRec) {
              __hip_atomic_fetch_or(&cx.bst[rs], S_DEACT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
              cx.et[rs] = NI; cx.eb[rs] = NI; cx.el[rs] = NI; cx.eflg[rs] = 0;
              __hip_atomic_fetch_or(&cx.bst[rs], S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              const int par = sel(cx.par, buf)[rs];
              if (par >= 0)
                __hip_atomic_fetch_or(&cx.bloom[par], 1ull << (sel(cx.lab, buf)[rs] & 63), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
  #pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ms = mys[h];
            if (ms >= 0) {
              const bool isbc = cw[h] >= 0;
              cx.et[ms] = sw[h]; cx.eb[ms] = NI; cx.el[ms] = sw[h];
              cx.ecn[ms] = cdw[h].p; cx.ebpn[ms] = cdw[h].bp;
              cx.eflg[ms] = F_HN;
              cx.ekind[ms] = isbc ? ((uint32_t)cw[h] << 1) : (((uint32_t)wi[h] << 1) | 1u);
              cx.elab[ms] = wl[h];
              if (isbc) __hip_atomic_fetch_and(&cx.bst[cw[h]], ~S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
          if (pc) pc[15] += __builtin_amdgcn_s_memtime() - q5;
          if (pc) pc[9] += __builtin_amdgcn_s_memtime() - tc1;
        } while (i0 < nb && !stop);
        }
#undef CTCX_WIN_HALF
        break;
      }
    }
    // large C, the beam full: a compacted chunk.  The offers of the span from
    // (i0, li0) on that can have an effect are gathered, in offer order, into
    // cx.cq (up to 64): a new child whose score can beat the current bottom
    // ((x_l - norm) + ot > bottom bounds the score; bottom only rises, so an
    // offer failing it now fails at its turn too) and every re-offer of a branch
    // child (evicted now, or by an event of this chunk before it).  The rest of
    // the span is rejected by the reference without effect.  Branch turns are
    // checked here at the current bottom (closed now: closed at its turn, the
    // grow ends after this chunk) and again in the chunk at the bottom its turn
    // sees (sl, bat below).
    if ((BIG || SQ) && full) {
      if constexpr (HW) {
        // the next chunk of wave 1's gather queue (the published count is read
        // first, so the reads issued after it see the chunk)
        const int slot = gqc & gq.sm;
        int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
        auto read_slot = [&]() {
          h0 = gq.h[slot * 4 + 0]; h1 = gq.h[slot * 4 + 1]; h2 = gq.h[slot * 4 + 2]; h3 = gq.h[slot * 4 + 3];
          if constexpr (SQ) {
            gqa = gq.a[slot * 64 + lane];
            gqv = gq.p[slot * 64 + lane];
            if constexpr (BIG) gqp = gq.a[slot * 64 + (lane > 0 ? lane - 1 : 0)].z;   // (small C: sq_pack_sl)
          } else {
            gqe = gq.e[slot * 64 + lane];
            gqp = gq.e[slot * 64 + (lane > 0 ? lane - 1 : 0)];
          }
        };
        {
          // one batch of reads, no loop around it (see the score-table read)
          int rdy = __hip_atomic_load(&cx.misc[kCtlReady], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __asm__ volatile("" ::: "memory");
          read_slot();
          if constexpr (SQ)
            __asm__ volatile("" ::"v"(h0), "v"(h1), "v"(h2), "v"(h3), "v"(gqa), "v"(gqv), "v"(gqp));   // one round trip
          else
            __asm__ volatile("" ::"v"(h0), "v"(h1), "v"(h2), "v"(h3), "v"(gqe), "v"(gqp));
          if (__builtin_expect(uni(rdy) <= gqc && !cx.tabdead, 0)) {
            // wave 1 is behind: wait for the count, then read again (a wait that
            // runs out of time, or a helper that gave up, takes cqn = 0 below:
            // the grow of this frame and of every later one ends, no queue
            // slot is used)
            uint64_t tw = 0;
            const uint64_t tq0 = pc ? __builtin_amdgcn_s_memtime() : 0;
            int spins = 0;
            for (int spin = 0;; ++spin) {
              spins = spin + 1;
              __builtin_amdgcn_s_sleep(CTCX_SLEEP);
              if (ctl_ld(cx.misc, kCtlReady) > gqc) break;
              if (ctl_ld(cx.misc, kCtlDead) != 0 || wait_expired(spin, tw)) {   // never in a correct run
                cx.tabdead = 1;
                __hip_atomic_store(&cx.misc[kCtlDead], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
              }
            }
            __asm__ volatile("" ::: "memory");
            read_slot();
            if (pc) {   // diagnostics: the queue wait (its s_sleep rounds); gqc 0: the frame's first chunk
              (void)uni((int)h0);
              pc[19] += __builtin_amdgcn_s_memtime() - tq0;
              pc[20] += spins;
              if (gqc == 0) pc[14] += __builtin_amdgcn_s_memtime() - tq0;
            }
          }
        }
        __asm__ volatile("" ::: "memory");
        ++gqc;
        __hip_atomic_store(&cx.misc[kCtlCons], gqc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        cqn = cx.tabdead ? 0 : uni(h0);
        cq_i0 = uni(h1);
        cq_l0 = uni(h2);
        gstop = uni(h3) != 0;
      } else {
        cq_i0 = i0;
        cq_l0 = li0;
        gather_chunk<T>(cx, buf, nb, norm, pmax, bottom, tsn, txo, i0, li0, cbr, gstop, row_cq(cx), cqn, pc);
      }
      if (cqn == 0) {
        if (gstop) stop = true;
        break;
      }
    }
    // small C: the turn check of a branch starting at this chunk's lane 0 uses
    // that lane's total from the chunk's read batch below (a branch spans few
    // chunks, and the chunk test below suffices for the rest)
    const bool turn0 = !BIG && !SQ && full && li0 == 0;
    const uint64_t tc0 = pc ? __builtin_amdgcn_s_memtime() : 0;
    // the chunk's lanes: offer (branch i, label l), valid / live, score s, the
    // branch total bt, the branch child c it re-offers (-1: none) and whether
    // that child has been evicted (cev), the child's label-ending candidate cd
    bool valid, live, isbc, cev;
    int i, l, c;
    int sl;   // the lane where this lane's branch turn starts in the chunk (see bat below)
    T s, bt;
    T cst = T(0);   // the child's scorer state (ExpandState, decoder.h:171)
    Best<T> cd{T(0), kBpNone, false};
    if (SQ && full) {
      // a scored chunk (help_gather_scored): lane j < cqn holds the j-th
      // gathered offer ready to push; what events change is read here: the
      // branch deactivated (only after a deactivation this frame), the branch
      // child evicted (only when a lane re-offers one)
      valid = lane < cqn;
      // (the words go through scalar copies: clang's __builtin_bit_cast of an
      // ext_vector element lvalue reads element 0 whatever the element -- the
      // cause of round 4's failed scored queue, where every field read the
      // score)
      const uint32_t ax = gqa.x, ay = gqa.y, az = gqa.z, aw = gqa.w;
      const uint32_t pk = valid ? az : 0u;   // (lanes past cqn: branch 0, no child)
      i = (int)(pk & 255u);
      c = (int)((pk >> 8) & 511u) - 1;
      s = (T)__builtin_bit_cast(float, ax);
      bt = (T)__builtin_bit_cast(float, ay);
      cd = Best<T>{(T)gqv, aw, true};
      if constexpr (BIG) {
        l = (int)(pk >> 17);
        const int ip = lane > 0 ? (int)(gqp & 255u) : -1;
        const uint64_t fm = __ballot(valid && i != ip) & lowmask(lane + 1);
        sl = (i > cq_i0 || cq_l0 == 0) ? 63 - __builtin_clzll(fm) : -1;
      } else {   // small C: the helper packed the turn-start lane (sq_pack_sl)
        l = sq_label_small(pk);
        sl = sq_turn_lane(pk);
      }
#ifdef CTCX_SQ_CHECK   // (diagnostics: wave 0 recomputes every scored field; mismatches counted in misc[15])
      {
        T s2, bt2;
        int c2;
        Best<T> cd2;
        sq_score<T>(cx, buf, norm, valid, i, l, s2, bt2, c2, cd2);
        const int fmask = (__builtin_bit_cast(unsigned, (float)s2) != __builtin_bit_cast(unsigned, (float)s) ? 1 : 0) |
                          (__builtin_bit_cast(unsigned, (float)bt2) != __builtin_bit_cast(unsigned, (float)bt) ? 2 : 0) |
                          (c2 != c ? 4 : 0) |
                          (__builtin_bit_cast(unsigned, (float)cd2.p) != __builtin_bit_cast(unsigned, (float)cd.p) ? 8 : 0) |
                          (cd2.bp != cd.bp ? 16 : 0);
        const bool bad = valid && fmask != 0;
        const uint64_t badM = __ballot(bad);
        if (badM) {
          const int kf = (int)__builtin_ctzll(badM);
          if (lane == kf) {
            if (__hip_atomic_fetch_add(&cx.misc[15], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) {
              // the first mismatch: fields, (lane, chunk, cqn, i, l), the two scores
              g_sq_dbg[0] = fmask | ((c + 1) << 8) | ((c2 + 1) << 16);
              g_sq_dbg[1] = lane | (gqc << 8) | (cqn << 16);
              g_sq_dbg[2] = i | (l << 16);
              // the branch totals: the slot's (read with the chunk), wave 0's, and the slot's read again now
              g_sq_dbg[3] = (int)__builtin_bit_cast(unsigned, (float)bt);
              g_sq_dbg[4] = (int)__builtin_bit_cast(unsigned, (float)bt2);
              g_sq_dbg[6] = (int)gq.a[((gqc - 1) & gq.sm) * 64 + lane].y;
              g_sq_dbg[7] = (int)__builtin_bit_cast(unsigned, (float)sel(cx.ot, buf ^ 1)[i]);
              g_sq_dbg[5] = (c & 0xffff) | (c2 << 16);
            }
          }
          __hip_atomic_fetch_add(&cx.misc[15], __builtin_popcountll(badM) - 1, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        s = s2; bt = bt2; c = c2; cd = cd2;
      }
#endif
      isbc = c >= 0;
      live = valid;
      if (dz) live = live && !(cx.bst[i] & S_DEACT);
      cev = false;
      if (__ballot(isbc)) cev = isbc && (cx.bst[isbc ? c : i] & S_EVICT);
    } else {
      int li;
      if (BIG && full) {
        // the compacted chunk: lane j < cqn holds the j-th gathered offer; a
        // branch turn starts at the first lane of its branch unless the branch
        // began before the span
        valid = lane < cqn;
        uint32_t e, ep;
        if constexpr (HW) {
          e = valid ? gqe : (uint32_t)__builtin_amdgcn_readfirstlane(gqe);   // (read with the slot's header)
          ep = gqp;
        } else {
          CTCX_LDS uint32_t* cq = row_cq(cx);
          e = cq[valid ? lane : 0];
          ep = cq[lane > 0 ? lane - 1 : 0];
        }
        i = (int)(e >> 16);
        li = (int)(e & 0xFFFFu);
        const int ip = lane > 0 ? (int)(ep >> 16) : -1;
        const uint64_t fm = __ballot(valid && i != ip) & lowmask(lane + 1);
        sl = (i > cq_i0 || cq_l0 == 0) ? 63 - __builtin_clzll(fm) : -1;
      } else {
        // lane -> (branch, label index): x / Cm1 for x < 64 + Cm1, by float reciprocal
        const int x = li0 + lane;
        int q = (int)((float)x * rcp);
        q -= (q * Cm1 > x) ? 1 : 0;
        q += ((q + 1) * Cm1 <= x) ? 1 : 0;
        const int iv = i0 + q;
        valid = iv < nb;
        i = valid ? iv : i0;
        li = valid ? x - q * Cm1 : 0;
        for (li0 += 64; li0 >= Cm1; li0 -= Cm1) ++i0;
        sl = lane - li;
      }
      l = li + (li >= blank ? 1 : 0);
      // one batch of LDS reads, every lane (i is a valid branch, l a valid
      // label), so the chunk waits on LDS once before its skip test
      const int bl = sel(cx.lab, buf)[i];
      const int bflg = sel(cx.flg, buf)[i];
      bt = sel(cx.ot, buf)[i];
      const T bob = sel(cx.ob, buf)[i];
      const int bsti = cx.bst[i];
      const uint64_t blm = cx.bloom[i];
      const int hd = cx.head[i];
      const T bcb = sel(cx.cb, buf)[i], bcn = sel(cx.cn, buf)[i];
      const T xl = cx.row[l];
      if (turn0 && !(bcast(bt, 0) > bottom)) break;   // branch i0's turn: skipped, and all later
      live = valid && !(bsti & S_DEACT);
      const T p = xl - norm;
      T base = (l == bl) ? bob : bt;
      if constexpr (SC::kStateful) {
        cst = SC::expand(cx, sel(cx.est, buf)[i], bl, l);
        base = SC::score(cst, base);
      }
      s = p + base;
      // the skip test below with the evicted-children bloom in place of the
      // children (found after it)
      if (full && !__ballot(live && ((s > bottom) | (((blm >> (l & 63)) & 1ull) != 0)))) {
        if (__ballot(valid && sl == lane && lane != 0) & ~__ballot(bt > bottom)) break;   // no event here: every start sees this bottom
        if (gstop) break;
        continue;
      }
      // the branch child this offer re-offers, if any (GetChild finds it): walk
      // branch i's children, each step one read pair (label, next sibling)
      c = -1;
      for (int k = live ? hd : -1; __ballot(k >= 0);) {
        int nk = -1;
        if (k >= 0) {
          const int lk = sel(cx.lab, buf)[k];
          const int sk = cx.sib[k];
          if (lk == l) c = k;
          else nk = sk;
        }
        k = nk;
      }
      isbc = c >= 0;
      const int cc = isbc ? c : i;
      cev = isbc && (cx.bst[cc] & S_EVICT);
      // label-ending candidate for the child (decoder.h:172-185), from branch i's
      // candidates read in the batch above
      const bool recv_fresh = isbc ? (sel(cx.ot, buf)[cc] == NI) : true;
      const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
      cd.push(((bflg & F_HB) ? bcb : rs_blank) + p, (bflg & F_HB) ? (((uint32_t)i << 1) | 0u) : kBpRestart);
      if (l != bl) cd.push(((bflg & F_HN) ? bcn : NI) + p, (bflg & F_HN) ? (((uint32_t)i << 1) | 1u) : kBpRestart);
    }
    // sl: the lane where this lane's branch turn starts in the chunk (< 0: in
    // an earlier chunk, found open there), and the bottom at that moment (bat:
    // refreshed after every event for turns that start later in the chunk)
    T bat = sl > 0 ? bottom : NI;
    const uint64_t startsM = __ballot(valid && sl == lane && lane != 0);   // branch turns starting mid-chunk
    if (pc) pc[10] += __builtin_amdgcn_s_memtime() - tc0;
    if (SQ && full && !__ballot(live && ((s > bottom) | (isbc && cev)))) {
      if (startsM & ~__ballot(bt > bottom)) break;   // no event here: every start sees this bottom
      if (gstop) break;
      continue;
    }
    const uint64_t isbm = __ballot(isbc);

    uint64_t tc1 = pc ? __builtin_amdgcn_s_memtime() : 0;
    if (pc) { pc[8] += tc1 - tc0; pc[11] += 1; }
    int myslot = -1;   // slot of this lane's accepted offer (-1: none, or evicted again)
    int evr = 0;       // record nev-th: evicted branch slot, or kDeactRec | rejected branch
    int nev = 0;
    uint64_t done = 0;
    while (true) {
      if ((RN == 1 || RN == 2) && st == kTopHeap && W >= 2) {
        // HEAP_SORTED, beams up to 128 (the mask form of the loop below, same
        // decisions): new-child lanes wanting in (NC: live, not a branch) are
        // accepted while they beat the front, re-offers of evicted branch
        // children (RB) are decided one by one.  The next push's child pairs
        // are loaded right after the previous push's stores, so their latency
        // overlaps the selection.
        // NC: live lanes offering a new child; LB: live lanes re-offering a
        // branch child; RB: those of LB whose branch has been evicted (wanted
        // whatever their score).  HEAP_SORTED is the last TopN state of the
        // frame, so live / cev are not needed after this loop.
        const uint64_t liveM = __ballot(live);
        uint64_t NC = liveM & ~isbm, LB = liveM & isbm, RB = LB & __ballot(cev);
        const auto geo = mask_geo<RN>(cx.hdum);
        T fv = front.v;
        int fs = front.s;
        int nfree = nextfree;
        int nv = uni(nev);
        if constexpr (sizeof(T) == 4 && (RN == 1 || RN == 2)) {
          // float: the hand-scheduled loop; re-offers of branch children come
          // back here one at a time
          const unsigned heb = (unsigned)(uintptr_t)he;   // LDS byte address of he[0]
          const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
          const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(cx.hdum + lane);
          for (;;) {
            int k;
            fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv);
            int nev_asm = 0;
            const uint64_t ta = pc ? __builtin_amdgcn_s_memtime() : 0;
            int est;
            if constexpr (RN == 1) {
              est = heap_events_f32(s, c, sl, geo.anc, geo.req, aj, al, ar, dum, myslot, evr, bat, NC, RB, done, LB,
                                    fv, fs, nfree, nv, uni(nb), k, nev_asm);
            } else {
              est = heap_events_m2_f32(s, c, sl, geo.g.anc, geo.g.req, (unsigned)geo.anc1, (unsigned)(geo.anc1 >> 32),
                                       (unsigned)geo.req1, (unsigned)(geo.req1 >> 32), aj, al, ar, aj + 512u,
                                       al + 1024u, ar + 1024u, dum, myslot, evr, bat, NC, RB, done, LB, fv, fs,
                                       nfree, nv, nb, k, nev_asm);
            }
            if (pc) { pc[13] += __builtin_amdgcn_s_memtime() - ta; pc[6] += uni(nev_asm); pc[12] += 1; }
            if (est == 0) break;
            k = uni(k);
            // lane k re-offers a branch child.  Only a re-offer can make a closed
            // turn visible (a closed branch's new children score <= its total <=
            // bottom): was k's turn skipped?
            const uint64_t gtM = __ballot(s > fv);
            const uint64_t m = ((gtM & NC) | RB) & ~done;   // its lowest lane is k
            if ((__ballot(!(bt > bat)) >> k) & 1ull) {
              const uint64_t keepM = lowmask(bcast(sl, k));   // that branch and every later one
              NC &= keepM; LB &= keepM; RB &= keepM;
              stop = true;
              continue;
            }
            done = m ^ (m - 1ull);
            const int kc = bcast(c, k);
            if (!((gtM >> k) & 1ull)) {
              // re-offered evicted branch rejected -> deactivated (decoder.h:200-205)
              evr = writelane(evr, kc | kDeactRec, nv);                                                             \
              dz = true;
              nv += 1;
              const uint64_t dm = ~__ballot(i == kc);
              NC &= dm; LB &= dm; RB &= dm;
              continue;
            }
            // accepted: the branch's entry keeps its slot
            if (fs < nb) {
              evr = writelane(evr, fs, nv);
              nv += 1;
              RB |= LB & __ballot(c == fs);
            }
            const T k_s = bcast(s, k);
            myslot = (myslot == fs) ? -1 : myslot;
            myslot = __builtin_amdgcn_inverse_ballot_w64(1ull << k) ? kc : myslot;
            MPairs<T, RN> pp;
            mpairs<T, RN>(he, geo, pp);
            T c0;
            int s0;
            bool keep;
            mpush<T, RN>(he, geo, k_s, kc, pp, c0, s0, keep);
            fv = keep ? k_s : c0;
            fs = keep ? kc : s0;
            bat = (sl > k) ? fv : bat;
          }
        } else {
          for (;;) {
            // the push's child pairs first: they depend only on the previous
            // push's stores, and their latency overlaps the selection below
            MPairs<T, RN> pp;
            mpairs<T, RN>(he, geo, pp);
            const uint64_t gtM = __ballot(s > fv);
            const uint64_t m = ((gtM & NC) | RB) & ~done;
            if (m == 0) break;
            const int k = (int)__builtin_ctzll(m);
            int slot;
            if (__builtin_expect((LB >> k) & 1ull, 0)) {
              // a re-offered branch child.  Only a re-offer can make a closed turn
              // visible (a closed branch's new children score <= its total <=
              // bottom): was k's turn skipped?
              if ((__ballot(!(bt > bat)) >> k) & 1ull) {
                const uint64_t keepM = lowmask(bcast(sl, k));   // that branch and every later one
                NC &= keepM; LB &= keepM; RB &= keepM;
                stop = true;
                continue;
              }
              done = m ^ (m - 1ull);
              slot = bcast(c, k);
              if (!((gtM >> k) & 1ull)) {
                // re-offered evicted branch rejected -> deactivated (decoder.h:200-205)
                evr = writelane(evr, slot | kDeactRec, nv);
                dz = true;
                nv += 1;
                const uint64_t dm = ~__ballot(i == slot);
                NC &= dm; LB &= dm; RB &= dm;
                continue;
              }
              // accepted: the branch's entry keeps its slot
              if (fs < nb) {
                evr = writelane(evr, fs, nv);
                nv += 1;
                RB |= LB & __ballot(c == fs);
              }
            } else {
              // a new child: it takes the evicted front's slot, or a fresh one when
              // the front is a branch's entry (which is reset and flagged instead)
              done = m ^ (m - 1ull);   // lanes <= k
              slot = fs;
              if (fs < nb) {
                slot = nfree;
                nfree += 1;
                evr = writelane(evr, fs, nv);
                nv += 1;
                RB |= LB & __ballot(c == fs);
              }
            }
            slot = uni(slot);
            const T k_s = bcast(s, k);
            myslot = (myslot == fs) ? -1 : myslot;
            myslot = __builtin_amdgcn_inverse_ballot_w64(1ull << k) ? slot : myslot;
            T c0;
            int s0;
            bool keep;
            mpush<T, RN>(he, geo, k_s, slot, pp, c0, s0, keep);   // push = pop_heap(W + 1)
            fv = uni(keep ? k_s : c0);
            fs = uni(keep ? slot : s0);
            bat = (sl > k) ? fv : bat;
          }
        }
        nev = nv;
        front.v = fv;
        front.s = fs;
        bottom = fv;
        nextfree = nfree;
        break;
      }
      if (st == kTopHeap) {
        // HEAP_SORTED (the beam is full): every wanted new child is accepted
        // and replaces the front; a re-offered evicted branch is accepted iff
        // it beats the bottom.  Per-lane flags are kept as wave masks so one
        // compare per event feeds both decisions.
        uint64_t liveM = __ballot(live), cevM = __ballot(cev);
        const HeapGeo<RN> geo = heap_geo<RN>(W, cx.hdum);
        // the front and the bump pointer as (uniform) VGPR values: nothing on
        // the event chain below leaves the vector unit except the event pick
        T fv = front.v;
        int fs = front.s;
        int nfree = nextfree;
        for (;;) {
          HeapPairs<T, RN> hp;
          heap_pairs<T, RN>(he, geo, hp);   // issued first: overlaps the event selection
#ifdef CTCX_FASTLOOP_PROF
          const uint64_t q0 = __builtin_amdgcn_s_memtime();
#endif
          const uint64_t gtM = __ballot(s > fv);
          const uint64_t m = liveM & ((isbm & cevM) | (~isbm & gtM)) & ~done;
          if (m == 0) break;
          const int k = (int)__builtin_ctzll(m);
          const bool kbc = (isbm >> k) & 1ull;
          if (__builtin_expect(kbc, 0)) {
            // only a re-offer can make a closed turn visible (a closed branch's new
            // children score <= its total <= bottom): was k's turn skipped?
            const uint64_t closedM = __ballot(!(bt > bat));
            if ((closedM >> k) & 1ull) {
              const int k_sl = bcast(sl, k);
              liveM &= (1ull << k_sl) - 1ull;   // that branch and every later one
              stop = true;
              continue;
            }
            if (!((gtM >> k) & 1ull)) {
              done = m ^ (m - 1ull);
              const int k_c = bcast(c, k);
              // re-offered evicted branch rejected -> deactivated (decoder.h:200-205)
              evr = (lane == nev) ? (k_c | kDeactRec) : evr;
              dz = true;
              nev += 1;
              liveM &= ~__ballot(i == k_c);
              continue;
            }
          }
          done = m ^ (m - 1ull);   // lanes <= k (k is m's lowest set bit; done's lanes are below it)
          const T k_s = bcast(s, k);
#ifdef CTCX_FASTLOOP_PROF
          const uint64_t q1 = __builtin_amdgcn_s_memtime();
#endif
          // the evicted front: a branch's entry is reset and flagged (the slot
          // stays the branch's); a new child's slot is reused
          const bool evb = fs < nb;
          const int slot = kbc ? bcast(c, k) : (evb ? nfree : fs);
          nfree += (!kbc && evb) ? 1 : 0;
          myslot = (myslot == fs) ? -1 : myslot;
          evr = (evb && lane == nev) ? fs : evr;
          nev += evb ? 1 : 0;
          myslot = (lane == k) ? slot : myslot;
          cevM |= isbm & __ballot(evb && c == fs);
#ifdef CTCX_FASTLOOP_PROF
          const uint64_t q2 = __builtin_amdgcn_s_memtime();
#endif
          wave_push_heap_v<T, RN>(he, geo, k_s, slot, hp, fv, fs);   // push = pop_heap(W + 1)
          bat = (sl > k) ? fv : bat;
#ifdef CTCX_FASTLOOP_PROF
          const uint64_t q3 = __builtin_amdgcn_s_memtime();
          if (pc) { pc[10] += q1 - q0; pc[12] += q2 - q1; pc[13] += q3 - q2; }
#endif
#ifdef CTCX_PHASES
          if (pc) pc[6] += 1;
#endif
        }
        front.v = uni(fv);
        front.s = uni(fs);
        bottom = front.v;
        nextfree = uni(nfree);
        live = (liveM >> lane) & 1ull;
        cev = (cevM >> lane) & 1ull;
        break;
      }
      const bool want = live && (isbc ? cev : (s > (full ? bottom : NI)));
      const bool acc = !isbc || (s > NI && (!full || s > bottom));
      const uint64_t m = __ballot(want) & ~done;
      if (m == 0) break;
      const int k = __ffsll((unsigned long long)m) - 1;
      if (full && ((isbm >> k) & 1ull) && ((__ballot(!(bt > bat)) >> k) & 1ull)) {
        live = live && lane < bcast(sl, k);   // k's turn was skipped, and every later one
        stop = true;
        continue;
      }
      done = (k == 63) ? ~0ull : ((2ull << k) - 1ull);
      const bool k_isbc = (isbm >> k) & 1ull;
      const bool accept = (__ballot(acc) >> k) & 1ull;
      const int k_c = bcast(c, k);
      if (accept) {
        const T k_s = bcast(s, k);
        // the evicted bottom is the front (decoder.h:192-198)
        const int fsl = front.s;
        const bool evb = full && fsl < nb;   // a branch's entry: reset, flagged
        const bool evc = full && fsl >= nb;  // a new child's entry: its slot is reused
        const int slot = k_isbc ? k_c : (evc ? fsl : nextfree);
        nextfree += (!k_isbc && !evc) ? 1 : 0;
        myslot = (full && myslot == fsl) ? -1 : myslot;
        evr = (evb && lane == nev) ? fsl : evr;
        nev += evb ? 1 : 0;
        myslot = (lane == k) ? slot : myslot;
        cev = cev || (evb && isbc && c == fsl);
        HE<T> nv;
        nv.v = k_s;
        nv.s = slot;
        {
          // UNORDERED (not full) appends; BOTTOM_KNOWN only ever sees a push right
          // after its front was evicted (-inf), so the swap check never fires
          if (full && lane == 0) he[1].v = NI;
          if (lane == 0) he_st(he, n + 1, nv);
          ++n;
          if (n == W + 1) {
#ifdef CTCX_FASTLOOP_PROF
            const uint64_t q4 = __builtin_amdgcn_s_memtime();
#endif
            if constexpr (kSqHeapM) {   // the mask form (its sentinels past the W + 1 elements first)
              heap_sentinels(he, W + 1, 128);
              wave_make_heap_m<T, true>(he, heap_m(cx.hdum), W + 1);   // (the front was set to -inf above)
            } else {
              wave_make_heap(he, W + 1);
            }
            const HE<T> r0 = he_ld(he, 1);
            front = wave_adjust_heap<T, RN>(he, heap_geo<RN>(W, cx.hdum), nv, W);   // pop_heap(W + 1)
            if (lane == 0) he_st(he, W + 1, r0);
            if ((RN == 1 || RN == 2) && W >= 2) heap_sentinels(he, W, RN == 2 ? 256 : 128);   // the mask-form sift's geometry
            st = kTopHeap;
#ifdef CTCX_FASTLOOP_PROF
            if (pc) pc[23] += __builtin_amdgcn_s_memtime() - q4;   // (make_heap: 14 is the first-chunk wait)
#endif
          } else if (n == W) {
            return 2;   // filled mid-frame: the lazy peek is replayed literally
          }
        }
        if (full) {
          bottom = front.v;
          bat = (sl > k) ? bottom : bat;
        }
      } else {
        // re-offered evicted branch rejected -> deactivated (decoder.h:200-205)
        evr = (lane == nev) ? (k_c | kDeactRec) : evr;
              dz = true;
        nev += 1;
        live = live && (i != k_c);
      }
    }
    // the turn continuing into the next chunk: skipped -> so is every later one
    if (full && (__ballot(valid && !(bt > bat)) >> (((BIG || SQ) && full) ? cqn - 1 : 63)) & 1ull) stop = true;
    if (gstop) stop = true;
    // flush: resets and flags first, then the surviving accepted entries
    const uint64_t q5 = pc ? __builtin_amdgcn_s_memtime() : 0;
    if (lane < nev) {
      const int rs = evr & ~kDeactRec;
      if (evr & kDeactRec) {
        __hip_atomic_fetch_or(&cx.bst[rs], S_DEACT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        cx.et[rs] = NI; cx.eb[rs] = NI; cx.el[rs] = NI; cx.eflg[rs] = 0;
        __hip_atomic_fetch_or(&cx.bst[rs], S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!(SQ && full)) {   // (scored chunks know their branch children: no bloom)
          const int par = sel(cx.par, buf)[rs];
          if (par >= 0)
            __hip_atomic_fetch_or(&cx.bloom[par], 1ull << (sel(cx.lab, buf)[rs] & 63), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    if (myslot >= 0) {
      cx.et[myslot] = s; cx.eb[myslot] = NI; cx.el[myslot] = s;
      cx.ecn[myslot] = cd.p; cx.ebpn[myslot] = cd.bp;
      cx.eflg[myslot] = F_HN;
      cx.ekind[myslot] = isbc ? ((uint32_t)c << 1) : (((uint32_t)i << 1) | 1u);
      cx.elab[myslot] = l;
      if constexpr (SC::kStateful) cx.eest[myslot] = cst;
      if (isbc) __hip_atomic_fetch_and(&cx.bst[c], ~S_EVICT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if constexpr (HW && (BIG || SQ))   // the helper gathers the next chunks against this bottom
      if (full)
        __hip_atomic_store(&cx.misc[kCtlBot], (int)__builtin_bit_cast(unsigned, (float)bottom), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    if (pc) pc[15] += __builtin_amdgcn_s_memtime() - q5;
    if (pc) pc[9] += __builtin_amdgcn_s_memtime() - tc1;
  }

  // the extract's rank placement on the helper (help_rank_extract): the final
  // heap's copy, then kCtlExt, both ahead of kCtlDone
  constexpr bool kExt = HW && SQ && RN == 1 && kExtRank && !BIG;
  const bool ext_rank = kExt && st == kTopHeap && W >= kExtMinW;
  if constexpr (kExt) {
    if (ext_rank) {
      CTCX_LDS float* xv = (CTCX_LDS float*)cx.newpos;
      const int W4 = (W + 3) & ~3;
#pragma unroll
      for (int k0 = 0; k0 < 128; k0 += 64) {
        const int k = k0 + lane;
        if (k < W) {
          xv[k] = (float)he[k + 1].v;
          cx.alias[k] = he[k + 1].s;
        } else if (k < W4) {
          xv[k] = __builtin_nanf("");
        }
      }
      // release (LDS only: no wait on the record stores): the copy before kCtlExt
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) __hip_atomic_store(&cx.misc[kCtlExt], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  // kEarlyRecurse: a full beam whose grow accepted no push never makes the
  // heap (st stays kTopBottomKnown: the W leaves in branch order, the smallest
  // in front), so the helper has nothing to rank -- but it can still recurse
  // the next frame from them.  The same copy, under kCtlExt 3: not ranked
  // (help_rank_extract returns on any value but 1), staged from.
  if constexpr (kExt && kEarlyRecurse && kEc0) {
    if (!ext_rank && st == kTopBottomKnown && full && n == W && W >= kExtMinW) {
      CTCX_LDS float* xv = (CTCX_LDS float*)cx.newpos;
#pragma unroll
      for (int k0 = 0; k0 < 128; k0 += 64) {
        const int k = k0 + lane;
        if (k < W) {
          xv[k] = (float)he[k + 1].v;
          cx.alias[k] = he[k + 1].s;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) __hip_atomic_store(&cx.misc[kCtlExt], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  // the grow is over: the helper stops scoring.  Released (LDS only): the
  // helper's acquire after it reads kCtlDone then sees kCtlExt and the copy
  if constexpr (HW) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __hip_atomic_store(&cx.misc[kCtlDone], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (BIG && cbr >= 0) cq_children(cx, buf, nb, cbr, -1);
  uint64_t ts2 = pc ? __builtin_amdgcn_s_memtime() : 0;
  if (pc) pc[2] += ts2 - ts1;
  const int size = n < W ? n : W;
  *n_leaves = size;
  // TopPaths (decoder.h:245-252) reads the unsorted layout: lane 0, literal
  if (last) {
    if (lane == 0) {
      for (int q = 0; q < size; ++q) cx.heap[q] = he[q + 1].s;
      SlotGreater<T> gt{cx.et};
      const int lim = P < W ? P : W;
      LitTop tp{cx.tops, 0, lim, kTopUnordered};
      for (int q = 0; q < size; ++q) lit_top_push(tp, cx.heap[q], gt);
      lit_top_extract(tp, gt);
    }
    wsync<HW>();
  }
  // Extract() of the next frame (decoder.h:84): sort_heap, or std::sort
  int nout;
  if (RN == 1 && st == kTopHeap && W >= 2) {
    // sort_heap in mask form (beams up to 128).  pop_heap(len) parks the old
    // front at position len - 1, which no later sift reads: the slot goes
    // straight into a register lane (position p: lane p of srt[p >> 6])
    // instead of back to LDS.
    const HeapM geo = heap_m(cx.hdum);
    int fs = front.s;
    int srt0 = 0, srt1 = 0;
    int stop = 2;   // positions below it: placed by rank (help_rank_extract)
#ifdef CTCX_PHASE_EXTP
    int ext_pops = 0;
#endif
    if constexpr (sizeof(T) == 4) {
      const unsigned heb = (unsigned)(uintptr_t)he;
      const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
      const unsigned dum = heb + 8u * (unsigned)(cx.hdum + lane);
      fs = uni(fs);
      // positions 127..64 into srt1, 63..2 into srt0, in four segments; with
      // the helper ranking (ext_rank), kCtlStop is read between them and the
      // pops end at the first position it has not placed
#ifdef CTCX_PHASE_EXTT
      if (lane == 0) cx.misc[14] = (int)(uint32_t)__builtin_amdgcn_s_memtime();
#endif
      const int cur = W;   // the first position to pop, plus one (a copy: with W read inside seg part 11's code moves)
      auto seg = [&](int top, int lo, int base, int& srt) {
        const int hi = cur < top ? cur : top;
        const int l = lo > stop ? lo : stop;
#ifdef CTCX_PHASE_EXTT
        const uint64_t sx0 = __builtin_amdgcn_s_memtime();
#endif
        if (hi > l) extract_fwd_f32(heb, uni(hi), uni(l), base, geo.anc, geo.req, aj, al, dum, srt, fs);
#ifdef CTCX_PHASE_EXTT
        if (pc && hi > l) { pc[23] += __builtin_amdgcn_s_memtime() - sx0; pc[17] += 1; pc[18] += hi - l; }
#endif
#ifdef CTCX_PHASE_EXTP
        if (hi > l) ext_pops += hi - l;
#endif
      };
      auto poll = [&]() {
        if (ext_rank) {   // acquire: the helper's sorted[] writes before its release of kCtlStop
          const int p = uni(__hip_atomic_load(&cx.misc[kCtlStop], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
          stop = p > stop ? p : stop;
        }
      };
      // (polls every 16 or 8 pops measured slower: cfg3 +0.4% / +1.2%,
      // profiles/r6i_ab_ext_seg.txt -- the helper's stop rarely lands early)
      seg(128, 96, 64, srt1);
      poll();
      seg(96, 64, 64, srt1);
      poll();
      seg(64, 32, 0, srt0);
      poll();
      seg(32, 2, 0, srt0);
    } else {
      for (int len = W; len > 2; --len) {
        const HE<T> v = he_ld(he, len);   // e[len-1] (uniform address)
        if (lane == 0) he_st(he, len, HE<T>{pinf<T>(), -1});   // vacated: a sentinel for the sift over len - 1
        HE<T> pL, pR;
        pairs_m(he, geo, pL, pR);
        const int pos = len - 1;
        if (pos >= 64) srt1 = writelane(srt1, fs, pos - 64);
        else srt0 = writelane(srt0, fs, pos);
        T c0;
        int s0;
        bool keep;
        push_m<T>(he, geo, v.v, v.s, pL, pR, c0, s0, keep);
        fs = keep ? uni(v.s) : s0;
      }
    }
#ifdef CTCX_PHASE_EXTP   // (diagnostics: the stop wave 0 used, and the frames it came from the helper)
    if (pc) { pc[16] += stop; pc[17] += stop > 2 ? 1 : 0; pc[18] += ext_pops; }
#endif
    // pop_heap(2): the front goes to position 1, e[1] becomes the root
    if (stop <= 2) {
      srt0 = writelane(srt0, fs, 1);
      srt0 = writelane(srt0, uni(he_ld(he, 2).s), 0);
    }
    nout = W;
    // (positions below a stop the helper published: the helper's)
    const int from = stop > 2 ? stop : 0;
    if (lane < nout && lane >= from) cx.sorted[lane] = srt0;
    if (lane + 64 < nout && lane + 64 >= from) cx.sorted[lane + 64] = srt1;
  } else if (RN == 2 && st == kTopHeap) {
    // sort_heap in the two-node mask form (beams 129..256), positions into
    // register lanes as above (position p: lane p & 63 of srt[p >> 6])
    const auto geo = mask_geo<RN>(cx.hdum);
    int fs = uni(front.s);
    int srt0 = 0, srt1 = 0, srt2 = 0, srt3 = 0;
    if constexpr (sizeof(T) == 4 && RN == 2) {
      const unsigned heb = (unsigned)(uintptr_t)he;
      const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
      const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(cx.hdum + lane);
      const unsigned an1l = (unsigned)geo.anc1, an1h = (unsigned)(geo.anc1 >> 32);
      const unsigned rq1l = (unsigned)geo.req1, rq1h = (unsigned)(geo.req1 >> 32);
      // positions 255..192 into srt3, 191..128 into srt2 (two-group sift),
      // then 127..64 into srt1 and 63..2 into srt0 (one-group sift)
      extract_m2_f32(heb, uni(W), 192, 192, geo.g.anc, geo.g.req, an1l, an1h, rq1l, rq1h, aj, al, ar, aj + 512u,
                     al + 1024u, ar + 1024u, dum, srt3, fs);
      extract_m2_f32(heb, uni(W < 192 ? W : 192), 128, 128, geo.g.anc, geo.g.req, an1l, an1h, rq1l, rq1h, aj, al,
                     ar, aj + 512u, al + 1024u, ar + 1024u, dum, srt2, fs);
      extract_f32(heb, uni(W < 128 ? W : 128), 64, 64, geo.g.anc, geo.g.req, aj, al, ar, dum, srt1, fs);
      extract_f32(heb, uni(W < 64 ? W : 64), 2, 0, geo.g.anc, geo.g.req, aj, al, ar, dum, srt0, fs);
    } else
    for (int len = W; len > 2; --len) {
      const HE<T> v = he_ld(he, len);   // e[len-1] (uniform address)
      if (lane == 0) he_st(he, len, HE<T>{pinf<T>(), -1});   // vacated: a sentinel for the sift over len - 1
      MPairs<T, RN> pp;
      mpairs<T, RN>(he, geo, pp);
      const int pos = len - 1;
      if (pos >= 192) srt3 = writelane(srt3, fs, pos - 192);
      else if (pos >= 128) srt2 = writelane(srt2, fs, pos - 128);
      else if (pos >= 64) srt1 = writelane(srt1, fs, pos - 64);
      else srt0 = writelane(srt0, fs, pos);
      T c0;
      int s0;
      bool keep;
      mpush<T, RN>(he, geo, v.v, v.s, pp, c0, s0, keep);
      fs = keep ? uni(v.s) : s0;
    }
    srt0 = writelane(srt0, fs, 1);
    srt0 = writelane(srt0, uni(he_ld(he, 2).s), 0);
    nout = W;
    if (lane < nout) cx.sorted[lane] = srt0;
    if (lane + 64 < nout) cx.sorted[lane + 64] = srt1;
    if (lane + 128 < nout) cx.sorted[lane + 128] = srt2;
    if (lane + 192 < nout) cx.sorted[lane + 192] = srt3;
  } else if (st == kTopHeap) {
    // pop_heap(len): e[len-1] <- e[0], then sift the old e[len-1] from the root
    T fv = front.v;
    int fs = front.s;
    for (int len = W; len > 1; --len) {
      const HeapGeo<RN> geo = heap_geo<RN>(len - 1, cx.hdum);
      const HE<T> v = he_ld(he, len);   // e[len-1], read before the old front lands there
      HeapPairs<T, RN> hp;
      heap_pairs<T, RN>(he, geo, hp);
      const T ofv = fv;
      const int ofs = fs;
      wave_push_heap_v<T, RN>(he, geo, v.v, v.s, hp, fv, fs);
      if (lane == 0) he_st(he, len, HE<T>{ofv, ofs});
    }
    nout = W;
    for (int k = lane; k < nout; k += 64) cx.sorted[k] = he[k + 1].s;
  } else {
    nout = n;
#ifdef CTCX_PHASES   // (the std::sort frames and their cycles: the upper halves of counters 7 and 11)
    const uint64_t tq0 = pc ? __builtin_amdgcn_s_memtime() : 0;
#endif
    bool placed = false;
#if CTCX_REG_SORT && !defined(CTCX_GSTATE)
    // in registers (all lanes store, as the sort_heap branch does); he is
    // untouched, so a frame it gives up on is sorted the literal way below.
    // Small C only: at large C nearly every frame accepts a push, so the
    // branch is rare there, and with it compiled in cfg4 measured 0.7% slower
    // (placement; profiles/r18_ab_reg_sort.txt).
    if constexpr (RN == 1 && sizeof(T) == 4 && !BIG) {
      if (n >= 1 && n <= 128) placed = reg_sort_extract<T>(cx, he, n);
    }
#endif
    if (!placed && lane == 0) {
      for (int q = 0; q < n; ++q) cx.sorted[q] = he[q + 1].s;
      lit_sort(cx.sorted, n, SlotGreater<T>{cx.et});
    }
#ifdef CTCX_PHASES
    if (pc) {
      pc[11] += (__builtin_amdgcn_s_memtime() - tq0) << 32;
      pc[7] += 1ull << 32;
    }
#endif
  }
  wsync<HW>();
  if (last && lane == 0) {
    // TopPaths slots -> sorted positions
    for (int q = 0; q < nout; ++q) cx.freel[cx.sorted[q]] = q;
    const int lim = (P < size) ? P : size;
    for (int q = 0; q < lim; ++q) cx.tops[q] = cx.freel[cx.tops[q]];
  }
  wsync<HW>();
  if (pc) pc[3] += __builtin_amdgcn_s_memtime() - ts2;
  *n_out = nout;
  return 0;
}

// ---------------------------------------------------------------------------
// LITERAL path for one frame, executed by lane 0 (decoder.h:69-210 verbatim in
// semantics, including TopN layout).  Returns the number of surviving entries
// (sorted slots in cx.sorted); for the last frame also fills cx.tops[0..P)
// with the TopPaths selection as positions.
//
// Duplicate entries.  With -inf totals the reference can push one BeamEntry
// twice: every branch is pushed after its recursion (decoder.h:142), and a
// branch whose new total is -inf is not Active, so its parent's grow loop
// re-creates it and pushes it again (decoder.h:168, 189-199).  Extract() then
// hands the entry out twice and the next Step visits it twice:
//   * the second roll copies the already reset new_cands into old_cands, so a
//     duplicated entry starts the frame without alignment candidates
//     (decoder.h:87-92);
//   * the second recursion accumulates into the newp.label the first one wrote
//     and keeps the first one's candidates (decoder.h:102-139);
//   * its grow loop runs twice over the same children (GetChild is the same
//     node), and deactivating or evicting the node affects every occurrence.
// Positions holding the same entry are linked by cx.alias (the first
// occurrence, which owns the entry slot); dup_in says this frame has any, and
// *dup_out that the next one does.
#ifdef CTCX_GSTATE
template <typename T, class SC, bool WAVE = true>
__host__ __device__ __attribute__((noinline)) int literal_step(Ctx<T> cx, int buf, int nb, T norm, bool last, int P,
                                                               bool dup_in, int* dup_out, int* n_leaves) {
  const T NI = ninf<T>();
  const int W = cx.W, C = cx.C, blank = cx.blank;
  // WAVE (the global-state tier): the whole wave enters; lane 0 alone runs
  // the replay and owns every state write, the other lanes only help scan a
  // branch's offers (below).  Otherwise one lane runs it all.
#ifdef __HIP_DEVICE_COMPILE__
  const bool me = !WAVE || (threadIdx.x & 63) == 0;
#else
  const bool me = true;
#endif
  int nfree = 0;
  SlotGreater<T> gt{cx.et};
  LitTop h{cx.heap, 0, W, kTopUnordered};
  if (me) {
    // roll (decoder.h:87-92)
    for (int i = 0; i < nb; ++i) {
      const int a = dup_in ? cx.alias[i] : i;
      if (a == i) {
        cx.et[i] = sel(cx.ot, buf)[i]; cx.eb[i] = sel(cx.ob, buf)[i]; cx.el[i] = sel(cx.ol, buf)[i];
        cx.eflg[i] = 0;
        cx.bst[i] = 0;
      } else {   // a second roll of the entry: old_cands = (reset) new_cands
        sel(cx.flg, buf)[i] &= ~(F_HB | F_HN);
        sel(cx.flg, buf)[a] &= ~(F_HB | F_HN);
      }
    }
    for (int s = cx.enc - 1; s >= nb; --s) {
      cx.freel[nfree++] = s;
      if (dup_in) cx.ekind[s] = 0xFFFFFFFFu;   // no stale match in the child lookup below
    }
    for (int i = 0; i < nb; ++i) {
      const int a = dup_in ? cx.alias[i] : i;
      recurse_branch<T, SC>(cx, buf, i, a, norm, true);
      lit_top_push(h, a, gt);
    }
  }
  // WAVE: lane 0's heap facts for the scan -- full, and the bottom's value
  // once the heap has been peeked since its last change (botk)
  [[maybe_unused]] auto heap_facts = [&](int& full, int& botk, T& botv) {
    full = (me && h.size() == W) ? 1 : 0;
    botk = (me && full && h.state != kTopUnordered) ? 1 : 0;
    botv = botk ? cx.et[h.e[0]] : NI;
    if constexpr (WAVE) {
#ifdef __HIP_DEVICE_COMPILE__
      full = __builtin_amdgcn_readfirstlane(full);
      botk = __builtin_amdgcn_readfirstlane(botk);
      botv = bcast(botv, 0);
#endif
    }
  };

  for (int i = 0; i < nb; ++i) {
    int go = 0;
    if (me) {
      const T bt = sel(cx.ot, buf)[i];
      go = (bt > NI && (h.size() < W || bt > cx.et[lit_top_peek_bottom(h, gt)])) ? 1 : 0;
    }
#ifdef __HIP_DEVICE_COMPILE__
    if constexpr (WAVE) go = __builtin_amdgcn_readfirstlane(go);
#endif
    if (!go) continue;
    const int a = dup_in ? cx.alias[i] : i;
    const int bl = sel(cx.lab, buf)[i];
    const int bflg = sel(cx.flg, buf)[i];
    // One offer (decoder.h:160-208), lane 0.
    auto offer = [&](int l) {
      int c = -1;
      for (int k = cx.head[a]; k >= 0; k = cx.sib[k])
        if (sel(cx.lab, buf)[k] == l) { c = k; break; }
      if (c < 0 && dup_in) {
        // GetChild of an entry visited twice: the child an earlier visit created
        // this frame is the same node (Active: skipped; otherwise re-created)
        bool act = false;
        for (int s = nb; s < cx.enc; ++s)
          if (cx.ekind[s] == (((uint32_t)a << 1) | 1u) && cx.elab[s] == l && cx.et[s] != NI) { act = true; break; }
        if (act) return;
      }
      int slot;
      const bool fresh_slot = (c < 0);
      if (!fresh_slot) {
        slot = c;
        if (cx.et[c] != NI) return;            // c.Active()
      } else {
        slot = cx.freel[nfree - 1];
        cx.eflg[slot] = 0;
      }
      const T xl = cx.row[l];
      const T p = xl - norm;
      cx.eb[slot] = NI;
      T prev = (l == bl) ? sel(cx.ob, buf)[i] : sel(cx.ot, buf)[i];
      if constexpr (SC::kStateful) {
        const T cst = SC::expand(cx, sel(cx.est, buf)[i], bl, l);   // ExpandState (decoder.h:171)
        cx.eest[slot] = cst;
        prev = SC::score(cst, prev);
      }
      cx.el[slot] = xl - norm + prev;
      const bool recv_fresh = fresh_slot ? true : (sel(cx.ot, buf)[c] == NI);
      const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
      Best<T> cd{cx.ecn[slot], cx.ebpn[slot], (cx.eflg[slot] & F_HN) != 0};
      cand_from(cx, buf, i, 0, p, rs_blank, cd);
      if (l != bl) cand_from(cx, buf, i, 1, p, NI, cd);
      cx.ecn[slot] = cd.p; cx.ebpn[slot] = cd.bp;
      cx.eflg[slot] |= F_HN;
      cx.et[slot] = cx.el[slot];
      cx.ekind[slot] = fresh_slot ? (((uint32_t)a << 1) | 1u) : ((uint32_t)c << 1);
      cx.elab[slot] = l;
      const T ct = cx.et[slot];
      if (ct > NI && (h.size() < W || ct > cx.et[lit_top_peek_bottom(h, gt)])) {
        if (fresh_slot) nfree--;
        if (h.size() == W) {
          const int bot = lit_top_peek_bottom(h, gt);
          cx.et[bot] = NI; cx.eb[bot] = NI; cx.el[bot] = NI;
          cx.eflg[bot] = 0;
          if (bot >= nb) cx.freel[nfree++] = bot;
        }
        lit_top_push(h, slot, gt);
      } else {
        // deactivate the child (decoder.h:200-205); a branch child's oldp and
        // old_cands are its frame-start arrays, at every position holding it
        cx.et[slot] = NI; cx.eb[slot] = NI; cx.el[slot] = NI;
        cx.eflg[slot] = 0;
        if (!fresh_slot) {
          for (int j = c; j < nb; ++j) {
            if (j != c && !(dup_in && cx.alias[j] == c)) continue;
            sel(cx.ot, buf)[j] = NI; sel(cx.ob, buf)[j] = NI; sel(cx.ol, buf)[j] = NI;
            sel(cx.flg, buf)[j] &= ~(F_HB | F_HN);
            if (!dup_in) break;
          }
        }
      }
    };
    if constexpr (!WAVE) {
      for (int l = 0; l < C; ++l)
        if (l != blank) offer(l);
    } else {
#ifdef __HIP_DEVICE_COMPILE__
      // With the beam full, an offer whose child is new and scores <= bottom is
      // rejected without effect (the reference creates the node and deactivates
      // it; nothing reads it again).  So the wave scores 64 labels at a time
      // and lane 0 replays only the offers that can matter: a label of one of
      // the branch's children (up to 4 kept; more: no scan), or a new child
      // scoring above the bottom -- any score above -inf while the bottom is
      // not known, since the reference's peek happens at that offer (lane 0
      // does it there).  The bottom only rises, so the scan's bottom, from
      // before the offers it lets through, passes a superset.
      const int lane = threadIdx.x & 63;
      int ch0 = -1, ch1 = -1, ch2 = -1, ch3 = -1;
      bool scan = !dup_in;
      if (scan) {
        int nch = 0;
        for (int k = cx.head[a]; k >= 0; k = cx.sib[k]) {
          const int lk = sel(cx.lab, buf)[k];
          if (nch == 0) ch0 = lk;
          else if (nch == 1) ch1 = lk;
          else if (nch == 2) ch2 = lk;
          else if (nch == 3) ch3 = lk;
          else { scan = false; break; }
          ++nch;
        }
      }
      const T b_ot = sel(cx.ot, buf)[i], b_ob = sel(cx.ob, buf)[i];
      int full, botk;
      T botv;
      heap_facts(full, botk, botv);
      for (int l = 0; l < C;) {
        if (scan && full) {
          uint64_t want = 0ull;
          for (; l < C; l += 64) {
            const int lq = l + lane;
            bool w = false;
            if (lq < C && lq != blank) {
              if (lq == ch0 || lq == ch1 || lq == ch2 || lq == ch3) {
                w = true;
              } else {
                T prev = (lq == bl) ? b_ob : b_ot;
                if constexpr (SC::kStateful) prev = SC::score(SC::expand(cx, sel(cx.est, buf)[i], bl, lq), prev);
                const T ct = cx.row[lq] - norm + prev;
                w = ct > NI && (!botk || ct > botv);
              }
            }
            want = __ballot(w);
            if (want) break;
          }
          if (l >= C) break;
          l += __builtin_ctzll(want);
        } else if (l == blank) {
          ++l;
          continue;
        }
        if (me) offer(l);
        ++l;
        heap_facts(full, botk, botv);
      }
#endif
    }
  }
  if (!me) return 0;   // (WAVE: lane 0's count is the result)
  *n_leaves = h.size();
  if (last) {
    const int lim = P < W ? P : W;
    LitTop tp{cx.tops, 0, lim, kTopUnordered};
    for (int q = 0; q < h.size(); ++q) lit_top_push(tp, h.e[q], gt);
    lit_top_extract(tp, gt);
  }
  const int n = lit_top_extract(h, gt);
  // slot -> first sorted position (freel reused as the map; -1 = not a leaf);
  // the next frame's aliases
  for (int s = 0; s < cx.enc; ++s) cx.freel[s] = -1;
  int dup = 0;
  for (int k = 0; k < n; ++k) {
    const int s = cx.heap[k];
    if (cx.freel[s] < 0) cx.freel[s] = k;
    else dup = 1;
    cx.sorted[k] = s;
    cx.alias[k] = cx.freel[s];
  }
  *dup_out = dup;
  if (last) {
    const int lim = (P < *n_leaves) ? P : *n_leaves;
    for (int q = 0; q < lim; ++q) cx.tops[q] = cx.freel[cx.tops[q]];
  }
  return n;
}

#else
// (the LDS tier's copy: one lane, every offer; it replays only the rare
// frames, and its decode kernels' register allocation was tuned beside it)
template <typename T, class SC>
__host__ __device__ __attribute__((noinline)) int literal_step(Ctx<T> cx, int buf, int nb, T norm, bool last, int P,
                                                               bool dup_in, int* dup_out, int* n_leaves) {
  const T NI = ninf<T>();
  const int W = cx.W, C = cx.C, blank = cx.blank;
  // roll (decoder.h:87-92)
  for (int i = 0; i < nb; ++i) {
    const int a = dup_in ? cx.alias[i] : i;
    if (a == i) {
      cx.et[i] = sel(cx.ot, buf)[i]; cx.eb[i] = sel(cx.ob, buf)[i]; cx.el[i] = sel(cx.ol, buf)[i];
      cx.eflg[i] = 0;
      cx.bst[i] = 0;
    } else {   // a second roll of the entry: old_cands = (reset) new_cands
      sel(cx.flg, buf)[i] &= ~(F_HB | F_HN);
      sel(cx.flg, buf)[a] &= ~(F_HB | F_HN);
    }
  }
  int nfree = 0;
  for (int s = cx.enc - 1; s >= nb; --s) {
    cx.freel[nfree++] = s;
    if (dup_in) cx.ekind[s] = 0xFFFFFFFFu;   // no stale match in the child lookup below
  }
  SlotGreater<T> gt{cx.et};
  LitTop h{cx.heap, 0, W, kTopUnordered};

  for (int i = 0; i < nb; ++i) {
    const int a = dup_in ? cx.alias[i] : i;
    recurse_branch<T, SC>(cx, buf, i, a, norm, true);
    lit_top_push(h, a, gt);
  }

  for (int i = 0; i < nb; ++i) {
    {
      const T bt = sel(cx.ot, buf)[i];
      if (!(bt > NI && (h.size() < W || bt > cx.et[lit_top_peek_bottom(h, gt)]))) continue;
    }
    const int a = dup_in ? cx.alias[i] : i;
    const int bl = sel(cx.lab, buf)[i];
    const int bflg = sel(cx.flg, buf)[i];
    for (int l = 0; l < C; ++l) {
      if (l == blank) continue;
      int c = -1;
      for (int k = cx.head[a]; k >= 0; k = cx.sib[k])
        if (sel(cx.lab, buf)[k] == l) { c = k; break; }
      if (c < 0 && dup_in) {
        // GetChild of an entry visited twice: the child an earlier visit created
        // this frame is the same node (Active: skipped; otherwise re-created)
        bool act = false;
        for (int s = nb; s < cx.enc; ++s)
          if (cx.ekind[s] == (((uint32_t)a << 1) | 1u) && cx.elab[s] == l && cx.et[s] != NI) { act = true; break; }
        if (act) continue;
      }
      int slot;
      const bool fresh_slot = (c < 0);
      if (!fresh_slot) {
        slot = c;
        if (cx.et[c] != NI) continue;            // c.Active()
      } else {
        slot = cx.freel[nfree - 1];
        cx.eflg[slot] = 0;
      }
      const T xl = cx.row[l];
      const T p = xl - norm;
      cx.eb[slot] = NI;
      T prev = (l == bl) ? sel(cx.ob, buf)[i] : sel(cx.ot, buf)[i];
      if constexpr (SC::kStateful) {
        const T cst = SC::expand(cx, sel(cx.est, buf)[i], bl, l);   // ExpandState (decoder.h:171)
        cx.eest[slot] = cst;
        prev = SC::score(cst, prev);
      }
      cx.el[slot] = xl - norm + prev;
      const bool recv_fresh = fresh_slot ? true : (sel(cx.ot, buf)[c] == NI);
      const T rs_blank = ((bflg & F_ROOT) && recv_fresh) ? T(0) : NI;
      Best<T> cd{cx.ecn[slot], cx.ebpn[slot], (cx.eflg[slot] & F_HN) != 0};
      cand_from(cx, buf, i, 0, p, rs_blank, cd);
      if (l != bl) cand_from(cx, buf, i, 1, p, NI, cd);
      cx.ecn[slot] = cd.p; cx.ebpn[slot] = cd.bp;
      cx.eflg[slot] |= F_HN;
      cx.et[slot] = cx.el[slot];
      cx.ekind[slot] = fresh_slot ? (((uint32_t)a << 1) | 1u) : ((uint32_t)c << 1);
      cx.elab[slot] = l;
      const T ct = cx.et[slot];
      if (ct > NI && (h.size() < W || ct > cx.et[lit_top_peek_bottom(h, gt)])) {
        if (fresh_slot) nfree--;
        if (h.size() == W) {
          const int bot = lit_top_peek_bottom(h, gt);
          cx.et[bot] = NI; cx.eb[bot] = NI; cx.el[bot] = NI;
          cx.eflg[bot] = 0;
          if (bot >= nb) cx.freel[nfree++] = bot;
        }
        lit_top_push(h, slot, gt);
      } else {
        // deactivate the child (decoder.h:200-205); a branch child's oldp and
        // old_cands are its frame-start arrays, at every position holding it
        cx.et[slot] = NI; cx.eb[slot] = NI; cx.el[slot] = NI;
        cx.eflg[slot] = 0;
        if (!fresh_slot) {
          for (int j = c; j < nb; ++j) {
            if (j != c && !(dup_in && cx.alias[j] == c)) continue;
            sel(cx.ot, buf)[j] = NI; sel(cx.ob, buf)[j] = NI; sel(cx.ol, buf)[j] = NI;
            sel(cx.flg, buf)[j] &= ~(F_HB | F_HN);
            if (!dup_in) break;
          }
        }
      }
    }
  }

  *n_leaves = h.size();
  if (last) {
    const int lim = P < W ? P : W;
    LitTop tp{cx.tops, 0, lim, kTopUnordered};
    for (int q = 0; q < h.size(); ++q) lit_top_push(tp, h.e[q], gt);
    lit_top_extract(tp, gt);
  }
  const int n = lit_top_extract(h, gt);
  // slot -> first sorted position (freel reused as the map; -1 = not a leaf);
  // the next frame's aliases
  for (int s = 0; s < cx.enc; ++s) cx.freel[s] = -1;
  int dup = 0;
  for (int k = 0; k < n; ++k) {
    const int s = cx.heap[k];
    if (cx.freel[s] < 0) cx.freel[s] = k;
    else dup = 1;
    cx.sorted[k] = s;
    cx.alias[k] = cx.freel[s];
  }
  *dup_out = dup;
  if (last) {
    const int lim = (P < *n_leaves) ? P : *n_leaves;
    for (int q = 0; q < lim; ++q) cx.tops[q] = cx.freel[cx.tops[q]];
  }
  return n;
}

#endif

// ---------------------------------------------------------------------------
// Record ring (LDS tier).  The traceback reads back only the P final paths'
// record chains (ctcx_traceback), and the chains of a frame's beams merge a
// few frames back: the beams share prefixes (the link) and alignment
// candidates (the two back-pointers).  Writing all W records of every frame
// (T·W·8 B per item, 393 MB per cfg3 launch) spends HBM writes on records
// nothing reads.  So the commit writes a frame's records into an LDS ring of
// R frames instead, and every R/2 frames ring_flush marks the records
// reachable from the current beam back through the ring (frame by frame: a
// reachable record's link and back-pointers mark their targets one frame
// down) and appends the reachable records of the oldest R/2 frames to the
// item's record stream in HBM, compacted, their pointers renumbered to the
// targets' compacted positions (frame u's records start at foff[u]).  A
// record unreachable now stays unreachable: every later beam descends from a
// current one.  After the last frame the walk starts from the TopPaths
// positions alone, and their compacted positions are what top_pos reports.
// record operations by format (the 8-byte Rec, the two-wave kernel's Rec32)
template <class RT> struct RecOps;
template <> struct RecOps<Rec> {
  __device__ static uint32_t link(Rec r) { return rec_link(r); }
  __device__ static int label(Rec r) { return rec_label(r); }
  __device__ static uint32_t bpb(Rec r) { return rec_bp_blank(r); }
  __device__ static uint32_t bpn(Rec r) { return rec_bp_nblank(r); }
  __device__ static Rec pack(uint32_t l, int lab, uint32_t b, uint32_t n) { return rec_pack(l, lab, b, n); }
};
template <> struct RecOps<Rec32> {
  __device__ static uint32_t link(Rec32 r) { return r & 255u; }
  __device__ static int label(Rec32 r) { return (int)((r >> 8) & 63u); }
  __device__ static uint32_t bpb(Rec32 r) { return rec32_unbp9((r >> 14) & 511u); }
  __device__ static uint32_t bpn(Rec32 r) { return rec32_unbp9(r >> 23); }
  __device__ static Rec32 pack(uint32_t l, int lab, uint32_t b, uint32_t n) { return rec32_pack(l, lab, b, n); }
};

template <class RT = Rec>
struct Ring {
  CTCX_LDS RT* rec;         // [R][W]: frame u in row u & (R - 1)
  CTCX_LDS int* rn;         // [R]: entries of each ring frame
  CTCX_LDS int16_t* tbl;    // [2][W]: compacted positions, by frame parity
  CTCX_LDS int16_t* sv;     // [2][W]: the newest written frame's, by flush parity
  CTCX_LDS int* st;         // [2][W]: reachability stamps, by frame parity
  int R, W;
};

template <class RT = Rec>
__device__ __forceinline__ Ring<RT> ring_carve(CTCX_LDS char* p, int R, int W) {
  auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  Ring<RT> g;
  g.R = R;
  g.W = W;
  g.rec = (CTCX_LDS RT*)p; p += a16((size_t)R * W * sizeof(RT));
  g.rn = (CTCX_LDS int*)p; p += a16(4 * (size_t)R);
  g.tbl = (CTCX_LDS int16_t*)p; p += a16(4 * (size_t)W);
  g.sv = (CTCX_LDS int16_t*)p; p += a16(4 * (size_t)W);
  g.st = (CTCX_LDS int*)p;
  return g;
}

// Reachable positions (a[j]: position lane + 64 j) -> compacted positions
// (rk[j]), in position order; returns how many there are.
template <int KM>
__device__ __forceinline__ int ring_rank(const bool (&a)[KM], int (&rk)[KM]) {
  int base = 0;
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    const uint64_t m = __ballot(a[j]);
    rk[j] = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    base += __builtin_popcountll(m);
  }
  return base;
}

// Marks from frame t_new (every entry, or the tops positions) down to u_lo,
// the oldest frame in the ring, and writes frames u_hi .. u_lo (reachable
// records, compacted) to the stream at out + cursor on.  fp: this flush's
// number (the previous flush left frame u_lo - 1's compacted positions in
// sv[(fp - 1) & 1]; this one leaves frame u_hi's in sv[fp & 1]).  Lane L
// holds positions L + 64 j (j < KM, KM * 64 >= W): their reachability, compacted
// positions and records stay in registers; a frame's reachable records stamp
// their targets one frame down (a value unique to this flush and step, so the
// stamps need no clearing), and the compacted positions go to LDS for the
// renumbering gathers.  ONE: a single wave runs it (the two-wave kernel's
// helper), so its barriers are wave-local.
template <int KM, class RT = Rec, bool ONE = false>
__device__ void ring_flush(const Ring<RT>& g, RT* out, int32_t* foff, int t_new, int u_lo, int u_hi,
                           const CTCX_LDS int* tops, int ntops, int fp, int& cursor) {
  using RO = RecOps<RT>;
  const int lane = threadIdx.x & 63, M = g.R - 1, W = g.W;
  const int sbase = fp * 4096;   // stamps of this flush: sbase + (t_new - frame) + 1; R <= 256
  bool al[KM];
  int rk[KM];
  {
    const int n = g.rn[t_new & M];
    if (tops != nullptr) {
      for (int q = lane; q < ntops; q += 64) g.st[(t_new & 1) * W + tops[q]] = sbase;
      wsync<ONE>();
    }
#pragma unroll
    for (int j = 0; j < KM; ++j) {
      const int k = lane + 64 * j;
      al[j] = k < n && (tops == nullptr || g.st[(t_new & 1) * W + k] == sbase);
    }
  }
  int cnt = ring_rank<KM>(al, rk);
  for (int u = t_new; u >= u_lo; --u) {
    const CTCX_LDS RT* ru = g.rec + (size_t)(u & M) * W;
    RT r[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) r[j] = al[j] ? ru[lane + 64 * j] : (RT)0;
    bool al1[KM];
    int rk1[KM], cnt1 = 0;
    if (u > u_lo) {
      // frame u - 1: the targets of frame u's reachable records
      CTCX_LDS int* s1 = g.st + ((u - 1) & 1) * W;
      const int sv1 = sbase + (t_new - u) + 1;
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        if (al[j]) {
          const uint32_t qb = RO::bpb(r[j]), qn = RO::bpn(r[j]);
          s1[RO::link(r[j]) >> 1] = sv1;
          if (qb < kBpRestart) s1[qb >> 1] = sv1;
          if (qn < kBpRestart) s1[qn >> 1] = sv1;
        }
      }
      wsync<ONE>();
      const int n1 = g.rn[(u - 1) & M];
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        const int k = lane + 64 * j;
        al1[j] = k < n1 && s1[k] == sv1;
      }
      cnt1 = ring_rank<KM>(al1, rk1);
      if (u <= u_hi) {
        CTCX_LDS int16_t* t1 = g.tbl + ((u - 1) & 1) * W;
#pragma unroll
        for (int j = 0; j < KM; ++j)
          if (al1[j]) t1[lane + 64 * j] = (int16_t)rk1[j];
        wsync<ONE>();
      }
    }
    if (u <= u_hi) {
      if (u == u_hi) {
#pragma unroll
        for (int j = 0; j < KM; ++j)
          if (al[j]) g.sv[(fp & 1) * W + lane + 64 * j] = (int16_t)rk[j];
      }
      // the targets' compacted positions: frame u - 1 in the ring, or written
      // by the previous flush; frame 0's targets are the root (left as they are)
      const CTCX_LDS int16_t* tp = u > u_lo ? g.tbl + ((u - 1) & 1) * W : g.sv + ((fp - 1) & 1) * W;
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        if (al[j]) {
          uint32_t lk = RO::link(r[j]), qb = RO::bpb(r[j]), qn = RO::bpn(r[j]);
          if (u > 0) {
            lk = ((uint32_t)tp[lk >> 1] << 1) | (lk & 1u);
            if (qb < kBpRestart) qb = ((uint32_t)tp[qb >> 1] << 1) | (qb & 1u);
            if (qn < kBpRestart) qn = ((uint32_t)tp[qn >> 1] << 1) | (qn & 1u);
          }
          out[cursor + rk[j]] = RO::pack(lk, RO::label(r[j]), qb, qn);
        }
      }
      if (lane == 0) foff[u] = cursor;
      cursor += cnt;
    }
#pragma unroll
    for (int j = 0; j < KM; ++j) { al[j] = al1[j]; rk[j] = rk1[j]; }
    cnt = cnt1;
  }
  wsync<ONE>();
}

// HW: two waves per item (wave 1 the helper, see help_score_chunks); every
// loop over positions below then runs over NT = 128 threads, and one-thread
// work is thread 0's (wave 0, the decoding wave).
template <typename T, int RN, int WC, bool BIG, class SC, bool HW, bool SQ = false>
__global__ __launch_bounds__(HW ? 128 : 64) void ctcx_beam_decode(DecodeParams<T> prm) {
  static_assert(!HW || (sizeof(T) == 4 && !SC::kStateful && (BIG ? WC > 0 : (RN == 1 && WC == 128))), "HW kernels");
  static_assert(!SQ || (HW && (RN == 1 ? WC == 128 : (RN == 2 && WC == 256 && BIG))), "SQ kernels");
  constexpr int NT = HW ? 128 : 64;
  Ctx<T> cx;
#ifdef CTCX_GSTATE
  // global-state tier: the item's state in global memory (gstate_bytes), the
  // row read in place from the inputs
  carve(cx, prm.gstate + (int64_t)blockIdx.x * prm.gstate_stride, prm.W, prm.W, 1, SC::kStateful, false);
  cx.C = (int)prm.C;
#else
  extern __shared__ __attribute__((aligned(16))) char lds[];
  carve(cx, (CTCX_LDS char*)lds, WC > 0 ? WC : prm.W, prm.W, (int)prm.C, SC::kStateful, BIG);   // BIG == decode_inplace(C)
#endif
  cx.blank = prm.blank;
  cx.sctab = prm.scorer_tab;
  cx.tabdead = 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t b = blockIdx.x;
#ifdef CTCX_PRIO
  if constexpr (HW) {   // the decoding wave first
    if (__builtin_amdgcn_readfirstlane(tid) < 64) __builtin_amdgcn_s_setprio(3);   // (a scalar branch)
  }
#endif
  const int W = prm.W;
  const int C = (int)prm.C;
  const int64_t B = prm.B;
  const int sl = prm.seq_len[b] > 0 ? prm.seq_len[b] : 0;
  CTCX_LDS int* const misc = cx.misc;
  // the record ring (host: ring_frames) after the decode layout; R = 0 writes
  // every record to rec[b][t][k]
  // HW kernels: 4-byte records, the score table after the decode layout,
  // then the ring, whose flushes the helper wave runs
  const int R = prm.ring;
  using RT = typename std::conditional<HW && !BIG, Rec32, Rec>::type;
  Ring<RT> rg{};
  [[maybe_unused]] Tab tb{};
  [[maybe_unused]] GQ gq{};
  // kRowPrefetch (small-C scored kernels): the row buffer the frame does not
  // use, and the words that say which frame's row and normaliser it holds
#ifndef CTCX_GSTATE
  constexpr bool kPf = kRowPrefetch && HW && SQ && !BIG && RN == 1 && sizeof(T) == 4 && !SC::kStateful;
#else
  constexpr bool kPf = false;
#endif
  [[maybe_unused]] CTCX_LDS T* row2 = nullptr;
  [[maybe_unused]] CTCX_LDS int* pfw = nullptr;
  // kEarlyRecurse (the same kernels): the staging area of the helper's recursion
  constexpr bool kEr = kEarlyRecurse && kPf;
  [[maybe_unused]] CTCX_LDS int* erw = nullptr;
#ifndef CTCX_GSTATE
  {
    size_t off = (decode_lds_bytes(WC > 0 ? WC : W, C, (int)sizeof(T), SC::kStateful) + 15) & ~(size_t)15;
    if constexpr (HW && !BIG && !SQ) {
      tb = tab_carve((CTCX_LDS char*)lds + off);
      off += tab_lds_bytes();
    }
    if constexpr (HW && (BIG || SQ)) {
      constexpr int kSlots = SQ ? sq_slots(WC) : kQSlots;
      gq = gq_carve<SQ>((CTCX_LDS char*)lds + off, kSlots);
      off += gq_lds_bytes(SQ, kSlots);
      if constexpr (kPf) {   // the second row buffer and its words (sq_rowpf_bytes)
        row2 = (CTCX_LDS T*)((CTCX_LDS char*)lds + off);
        pfw = (CTCX_LDS int*)((CTCX_LDS char*)lds + off + sq_rowpf_bytes(C) - 16);
        off += sq_rowpf_bytes(C);
      }
      if constexpr (kEr) {   // the staged recursion (sq_stage_bytes): four words, then the planes
        static_assert(WC == 128 && sq_slots(WC) * 64 * 4 >= kErMapBr + WC && kErMapBr >= 3 * WC + 2, "the maps' room");
        erw = (CTCX_LDS int*)((CTCX_LDS char*)lds + off);
        off += sq_stage_bytes(WC, C);
      }
    }
    if (R > 0) rg = ring_carve<RT>((CTCX_LDS char*)lds + off, R, W);
  }
#endif
  if (R > 0)
    for (int k = lane; k < 2 * W; k += 64) rg.st[k] = -1;   // no stamp yet
  RT* const rstream = (RT*)prm.rec + b * prm.Tmax * W;   // item b's record stream (ring)
  int pf_t = -1, pf_lo = 0, pf_hi = 0, pf_fp = 0;      // HW: a ring flush pending for the helper
  int32_t* const foff = prm.foff ? prm.foff + b * prm.Tmax : nullptr;
  int flushed = 0, nflush = 0, nrec = 0;   // first frame not yet in HBM, flushes, ring stream cursor
  int64_t nrec_all = 0;                    // records written without the ring (T * W can pass 2^31)

#ifdef CTCX_STREAM
  // A stream's push: sl frames of item b's chunk, on top of the hin.frames the
  // item has behind it.  Its state at a frame boundary is the whole LDS
  // allocation (the global-state build: the carve, which already lives in the
  // stream's HBM buffer) and the scalars of the header.
  const char* const st_in = prm.st.in + b * prm.st.stride;
  char* const st_out = prm.st.out + b * prm.st.stride;
  const CtcxStreamHdr hin = *(const CtcxStreamHdr*)st_in;
  const int t0g = uni(hin.frames);  // the item's global index of the chunk's first frame
  const bool resume = t0g > 0;      // (uniform)
  const size_t st_hdr = ctcx_stream_hdr_bytes(prm.P);
  if (resume && sl == 0) {
    // no frame for this item: state and header pass through to the out
    // buffer, and the item reports the hypotheses it had
    const size_t n16 = (st_hdr + (size_t)prm.st.image_bytes + 15) >> 4;   // (stride is a multiple of 256)
    for (size_t q = tid; q < n16; q += NT) ((u32x4*)st_out)[q] = ((const u32x4*)st_in)[q];
    const int32_t* hp = (const int32_t*)(st_in + sizeof(CtcxStreamHdr));
    const int64_t* hl = (const int64_t*)(hp + 2 * prm.P);
    for (int q = tid; q < prm.P; q += NT) {
      prm.top_pos[b * prm.P + q] = hp[q];
      prm.top_kind[b * prm.P + q] = hp[prm.P + q];
      prm.log_prob[b * prm.P + q] = *(const T*)(hl + q);
    }
    if (tid == 0) {
      ItemOut io;
      io.n_leaves = hin.n_leaves; io.literal_steps = hin.literal_steps; io.dup_frames = hin.dup_frames;
      io.why_nonfinite = hin.why_nonfinite; io.why_fill = hin.why_fill; io.pad = kEr ? (hin.pad[0] << 1) : 0;
      io.records = hin.records;
      prm.item[b] = io;
    }
    return;
  }
#ifndef CTCX_GSTATE
  if (resume) {   // the image into LDS: 16-byte loads over all threads, then the words the layout's sizes leave over
    const char* img = st_in + st_hdr;
    const size_t nby = (size_t)prm.st.image_bytes, n16 = nby >> 4;
    for (size_t q = tid; q < n16; q += NT) ((CTCX_LDS u32x4*)lds)[q] = ((const u32x4*)img)[q];
    for (size_t q = (n16 << 2) + tid; q < (nby >> 2); q += NT) ((CTCX_LDS uint32_t*)lds)[q] = ((const uint32_t*)img)[q];
    __syncthreads();
  }
#endif
#endif
  // Reset(): root with newp.total = newp.blank = 0 (decoder.h:213-227)
  int buf = 0;
  if (tid < 32) cx.etab[tid] = gm::exp2f_tab(tid);
  if (tid == 0) {
    // (tests: kTestHelperDead starts the helper out as if its first wait had
    // run out of time, so the failure path runs without a hang)
    cx.misc[kCtlDead] = (HW && (prm.test_flags & kTestHelperDead)) ? 1 : 0;
    cx.misc[15] = 0;
    if constexpr (kPf) pfw[kPfRowT] = -1;   // no row held: a prefetch never crosses a launch (a stream's push)
    if constexpr (kEr) erw[kErT] = -1;      // ... nor does a staged recursion
#ifdef CTCX_STREAM
  }
  // (the per-launch words above are set after the load; the rest of Reset()
  // is for an item without frames behind it)
  if (!resume) {
  if (tid == 0) {
#endif
    cx.lab[0][0] = -1; cx.par[0][0] = -1; cx.flg[0][0] = F_ROOT;
    cx.ot[0][0] = T(0); cx.ob[0][0] = T(0); cx.ol[0][0] = ninf<T>();
    cx.cb[0][0] = T(0); cx.cn[0][0] = T(0);
    cx.ha[0][0] = kRootHa; cx.hb[0][0] = kRootHb;
    cx.head[0] = -1;
    cx.alias[0] = 0;
    if constexpr (SC::kStateful) cx.est[0][0] = T(0);   // InitializeState (decoder.h:226)
  }
  if constexpr (BIG) {   // the child bitmap and window summary start (and stay, between branches) clear
    const int nw = (C - 1 + 63) / 64;
    CTCX_LDS uint64_t* z = row_cbm(cx);
    for (int k = lane; k < nw + (nw + 63) / 64; k += 64) z[k] = 0ull;
  }
#ifdef CTCX_STREAM
  }   // !resume
#endif
  int nb = 1;
  int literal_steps = 0;
  int why_nf = 0, why_fill = 0, dup_frames = 0;
  bool dup = false;   // this frame's beam holds an entry twice (literal frames only)
  int n_leaves = 1;
  // kEarlyRecurse: this frame's recursion is in place already (the last commit
  // moved the helper's staged words there), and the item's count of such frames
  [[maybe_unused]] bool er_hit = false;
  [[maybe_unused]] int early_rec = 0;
#ifdef CTCX_STREAM
  // (the header's reserved word, 0 in every image, goes from push to push as
  // the flag it once was: the stream builds' code stays what it was)
  bool reserved0 = false;
  if (resume) {   // the scalars a frame hands to the next, and the item's counters so far
    if constexpr (kEr) early_rec = uni(hin.pad[0]);
    buf = uni(hin.buf); nb = uni(hin.nb); dup = uni(hin.dup) != 0; reserved0 = uni(hin.reserved0) != 0;
    n_leaves = uni(hin.n_leaves); literal_steps = uni(hin.literal_steps); dup_frames = uni(hin.dup_frames);
    why_nf = uni(hin.why_nonfinite); why_fill = uni(hin.why_fill); nrec_all = (int64_t)uni64((uint64_t)hin.records);
  }
#define CTCX_FRAME(t) (t0g + (t))   // the item's global frame index: where a record lives
#else
#define CTCX_FRAME(t) (t)
#endif
  __syncthreads();

#ifdef CTCX_PHASES
  // per-phase s_memtime accumulators (diagnostics builds only; PhaseCtr)
  const bool prof = prm.prof != nullptr;
  const PhaseCtr pc{prof ? prm.prof + (size_t)b * kPhaseN : nullptr};
  cx.prof = pc.p;
  if (prof && tid == 0)
    for (int q = 0; q < kPhaseN; ++q) pc.p[q] = 0;
#else
  const PhaseCtr pc{nullptr};
  constexpr bool prof = false;
#endif
  for (int t = 0; t < sl; ++t) {
    uint64_t t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
    // the row stage: the only read of x.  Row (t, b) starts xoff elements
    // into x (elements of prm.xfmt); everything below works on the LDS copy
    const int64_t xoff = (int64_t)t * prm.xst_t + (int64_t)b * prm.xst_b;
    const T* xr = prm.x + xoff;
    [[maybe_unused]] bool pf_hit = false;   // kRowPrefetch: this frame's row is in the other buffer already
#ifdef CTCX_GSTATE
    cx.row = const_cast<T*>(xr);   // (read in place: the host hands this tier rows of T)
#else
    // kRowPrefetch: the helper loaded this frame's row and normaliser during
    // the last frame's extract (below): switch buffers.  The word is uniform
    // over the workgroup: written before the barrier that follows exact_step,
    // read here, after the commit's closing barrier.
    if constexpr (kPf) {
      pf_hit = uni(pfw[kPfRowT]) == t;
      if (pf_hit) {
        CTCX_LDS T* const r = cx.row;
        cx.row = row2;
        row2 = r;
      }
    }
    if (kPf && pf_hit) {
    } else
    if (sizeof(T) == 4 && prm.xfmt != kInNative) {   // uniform: half-precision rows, widened into the LDS row
      if constexpr (sizeof(T) == 4)
        stage_row_half((CTCX_LDS unsigned*)cx.row, (const uint16_t*)prm.x + xoff, C, prm.xfmt == kInF16, tid, NT);
    } else if constexpr (BIG && sizeof(T) == 4) {
      // a large row: 16-byte loads, a batch of them in flight per thread
      // before the first LDS write (a load-store pair per element waited out
      // one global latency each: 16k cycles per cfg5 frame)
      if ((C & 3) == 0 && (((uintptr_t)xr) & 15) == 0) {
        const u32x4* x4 = (const u32x4*)xr;
        CTCX_LDS u32x4* r4 = (CTCX_LDS u32x4*)cx.row;
        const int C4 = C >> 2;
        constexpr int kRB = 8;
        for (int q0 = 0; q0 < C4; q0 += kRB * NT) {
          u32x4 v[kRB];
  #pragma unroll
          for (int u = 0; u < kRB; ++u) {
            const int q = q0 + u * NT + tid;
            if (q < C4) v[u] = x4[q];
          }
  #pragma unroll
          for (int u = 0; u < kRB; ++u) {
            const int q = q0 + u * NT + tid;
            if (q < C4) r4[q] = v[u];
          }
        }
      } else {
        for (int j = tid; j < C; j += NT) cx.row[j] = xr[j];
      }
    } else {
      for (int j = tid; j < C; j += NT) cx.row[j] = xr[j];
    }
#endif
    if constexpr (HW) {   // the helper's hand-over words, per frame
      if (tid < 3) cx.misc[kCtlReady + tid] = 0;
      if (tid == 3) cx.misc[kCtlBot] = (int)0xff800000u;   // -inf
      if (tid == 4) cx.misc[kCtlExt] = 0;
      if (tid == 5) cx.misc[kCtlStop] = 0;
    }
    // (a prefetched frame: its normaliser came with the row; kPf: T is float, a word)
    const T norm = (kPf && pf_hit) ? ((CTCX_LDS T*)pfw)[kPfNorm] : prm.norm[(int64_t)t * B + b];
    if constexpr (BIG) {
      // the pre-pass record of row (t, b): header, block maxima, top set
      const char* pr = prm.prep + ((int64_t)t * B + b) * (int64_t)prep_row_bytes(C, (int)sizeof(T));
      const RowHdr<T> rh = *(const RowHdr<T>*)pr;
      cx.rxmax = rh.xmax; cx.rxout = rh.xout; cx.rbad = rh.bad; cx.rns = rh.ns;
      const T* pbm = (const T*)(pr + prep_bmax_offset((int)sizeof(T)));
      CTCX_LDS T* bmx = row_bmax(cx);
      for (int k = lane; k * 64 < C; k += 64) bmx[k] = pbm[k];
      if constexpr (sizeof(T) == 4) {
        const uint2* ptop = (const uint2*)(pr + prep_top_offset(C, 4));
        CTCX_LDS float* sx = row_topx(cx);
        CTCX_LDS int* sli = (CTCX_LDS int*)(sx + kTopK);
        for (int q = lane; q < rh.ns; q += 64) {
          const uint2 e = ptop[q];
          sx[q] = __uint_as_float(e.x);
          sli[q] = (int)e.y;
        }
      }
    }
    __syncthreads();
    const bool last = (t == sl - 1);

    int n = 0;
    int why = 4;
    int nl_fast = 0;
    uint64_t t1 = prof ? __builtin_amdgcn_s_memtime() : 0;
    if (prof) pc[0] += t1 - t0;
#ifndef CTCX_GSTATE   // the global-state tier replays every frame literally
    if (!prm.force_literal && !dup)
      why = exact_step<T, RN, BIG, SC, HW, SQ>(cx, buf, nb, norm, last, prm.P, &n, &nl_fast, prof ? pc : PhaseCtr{nullptr}, tb, gq,
                                               kEr && er_hit);
#endif
    if constexpr (HW) {
      // wave 0's result for both waves; the helper stops if the grow ended
      // early (a frame handed to the literal path)
      if (tid == 0) {
        __hip_atomic_store(&cx.misc[kCtlDone], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        cx.misc[4] = why;
        cx.misc[5] = n;
        cx.misc[6] = nl_fast;
      }
      if (helper_wave() && pf_t >= 0) {   // the helper: the flush the previous commit left pending
        [[maybe_unused]] const uint64_t hf0 = CTCX_HTIME();
        ring_flush<(WC > 0 ? WC : 512) / 64, RT, true>(rg, rstream, foff, pf_t, pf_lo, pf_hi, nullptr, 0, pf_fp, nrec);
        CTCX_HPC(cx, 29, CTCX_HTIME() - hf0);
      }
#ifndef CTCX_GSTATE
      if constexpr (kPf) {
        // the helper, its ranks and flush done while wave 0 extracts: the next
        // frame's row and normaliser into the buffer this frame does not read
        // (literal_step and the commit read the current one or none), then the
        // word that names the frame held.  Only after a frame in which the
        // helper gathered, and for rows of T (half rows keep their row stage);
        // row t + 1 exists only below the item's length.
        if (helper_wave() && !prm.force_literal && !dup && nb >= W && t + 1 < sl && prm.xfmt == kInNative &&
            ctl_ld(cx.misc, kCtlDead) == 0) {
          const int64_t xoff1 = (int64_t)(t + 1) * prm.xst_t + (int64_t)b * prm.xst_b;
          if (lane < C) row2[lane] = prm.x[xoff1 + lane];   // (C <= 64)
          if (lane == 0) ((CTCX_LDS T*)pfw)[kPfNorm] = prm.norm[(int64_t)(t + 1) * B + b];
          __hip_atomic_store(&pfw[kPfRowT], t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          // kEarlyRecurse: frame t + 1's recursion from the final beam, in the
          // rest of wave 0's extract (help_early_recurse).  The row and norm it
          // reads are the two stores above (one wave: its LDS operations
          // execute in order).  Only where wave 0 published the final heap
          // (kCtlExt == 1: the frame's grow ran to its end on the heap); erw's
          // word names the frame like kPfRowT, and is read after the barrier
          // below, so the helper adds no wait of its own.
          if constexpr (kEr) {
            const int ext = ctl_ld(cx.misc, kCtlExt);   // (1: the final heap; 3: a beam no push changed)
            if (!(prm.test_flags & kTestNoEarlyRecurse) && (ext == 1 || ext == 3)) {
              [[maybe_unused]] const uint64_t he0 = CTCX_HTIME();
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
              __builtin_amdgcn_wave_barrier();
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
              help_early_recurse<T, WC>(cx, buf, row2, ((CTCX_LDS T*)pfw)[kPfNorm], erw + 4, (CTCX_LDS int*)gq.a);
              __hip_atomic_store(&erw[kErT], t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
              CTCX_HPC(cx, 23, CTCX_HTIME() - he0);   // (wave 0 leaves counter 23 alone in this kernel)
            }
          }
        }
      }
#endif
      pf_t = -1;
      __syncthreads();
      why = uni(cx.misc[4]);
      n = uni(cx.misc[5]);
      nl_fast = uni(cx.misc[6]);
    }
    __syncthreads();
    uint64_t t2 = prof ? __builtin_amdgcn_s_memtime() : 0;
    const bool ok = (why == 0);
    // kEarlyRecurse: the helper staged the next frame's recursion from this
    // frame's final beam (its word, written before the barrier above, names
    // frame t + 1), and the frame stayed on the exact path: the commit below
    // moves the staged words into place.  Uniform over the workgroup.
    [[maybe_unused]] bool er_place = false;
    if constexpr (kEr) {
      early_rec += (er_hit && ok) ? 1 : 0;
      er_place = ok && uni(erw[kErT]) == t + 1;
    }
    why_nf += (why == 1); why_fill += (why == 2);
    dup_frames += dup ? 1 : 0;
    bool dup_next = false;
    if (!ok) {
#ifdef CTCX_GSTATE
      // every frame is replayed here: wave 0 scans the offers with lane 0
      if (tid < 64) {
        int d2 = 0, nl = 0;
        const int nn = literal_step<T, SC, true>(cx, buf, nb, norm, last, prm.P, dup, &d2, &nl);
        if (tid == 0) {
          misc[0] = nn;
          misc[1] = d2;
          misc[2] = nl;
        }
      }
#else
      if (tid == 0) {
        int d2 = 0, nl = 0;
        misc[0] = literal_step<T, SC>(cx, buf, nb, norm, last, prm.P, dup, &d2, &nl);
        misc[1] = d2;
        misc[2] = nl;
      }
#endif
      __syncthreads();
      n = misc[0];
      dup_next = uni(misc[1]) != 0;   // wave-uniform: the next frame's exact_step call stays uniform
      n_leaves = misc[2];
      ++literal_steps;
    } else {
      n_leaves = nl_fast;
    }
    __syncthreads();
    uint64_t t3 = prof ? __builtin_amdgcn_s_memtime() : 0;
    if (prof) pc[5] += t3 - t2;

    // ---- commit: records + next frame's branch arrays (sorted order) ----
    // Large C: the arrays are updated in place, so every read of the
    // frame-start arrays (by source position) is taken into registers before
    // the first write (by sorted position); KM positions per lane.
    constexpr bool INPLACE = BIG;
    // staged (unrolled, KM positions per lane) for a compile-time capacity, and
    // always in place (the LDS tier: W <= 512); plain loops otherwise (any W)
    constexpr bool STAGED = WC > 0 || INPLACE;
    constexpr int KM = (WC > 0 ? WC : 512) / NT;   // positions per thread
    const int nx = INPLACE ? buf : buf ^ 1;
    for (int i = tid; i < nb; i += NT) cx.newpos[i] = -1;
    __syncthreads();
    // (an entry the beam holds twice: its first position is the canonical one,
    // the one its children link to and the hash table maps to)
    for (int k = tid; k < n; k += NT) {
      const uint32_t kd = cx.ekind[cx.sorted[k]];
      if (!dup_next) cx.alias[k] = k;
      else if (cx.alias[k] != k) continue;
      if (!(kd & 1u)) cx.newpos[kd >> 1] = k;
    }
    // kEarlyRecurse: the position of each staged entry (slot -> j is the
    // helper's map in the gather queue's offer plane, untouched until the next
    // frame's first chunk)
    [[maybe_unused]] int erj = 0;   // (n <= WC == NT: position tid is this thread's only one)
    if constexpr (kEr) {
      static_assert(!kEr || WC == NT, "one position per thread");
      if (er_place && tid < n) {
        erj = ((CTCX_LDS int*)gq.a)[kErMapSlot + cx.sorted[tid]] & (WC - 1);
        erw[4 + kErPos * WC + erj] = tid;
      }
    }
    for (int q = tid; q < cx.hts; q += NT) cx.htab[q] = -1;
    __syncthreads();
    // One position k of the commit: the new prefix hash (phase 1), then the
    // parent position and flags (phase 2), then the writes.  In place (large
    // C), every read of the frame-start arrays precedes every write (staged in
    // registers, KM positions per lane, W <= 512 on that tier); double
    // buffered, each position is read and written in one pass (any W).
    auto hash_of = [&](int k, uint64_t& ha, uint64_t& hb) {
      const int e = cx.sorted[k];
      const uint32_t kd = cx.ekind[e];
      const int src = (int)(kd >> 1);
      ha = sel(cx.ha, buf)[src];
      hb = sel(cx.hb, buf)[src];
      if (kd & 1u) hmix(ha, hb, cx.elab[e], ha, hb);
    };
    auto put_hash = [&](int k, uint64_t ha, uint64_t hb) {
      sel(cx.ha, nx)[k] = ha;
      sel(cx.hb, nx)[k] = hb;
      if ((cx.ekind[cx.sorted[k]] & 1u) && (!dup_next || cx.alias[k] == k)) {
        int q = (int)(ha & (uint64_t)(cx.hts - 1));
        int expect = -1;
        while (!__hip_atomic_compare_exchange_strong(&cx.htab[q], &expect, k, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WORKGROUP)) {
          q = (q + 1) & (cx.hts - 1);
          expect = -1;
        }
      }
    };
    auto parent_of = [&](int k, int& parent, int& fl) {
      const int e = cx.sorted[k];
      const uint32_t kd = cx.ekind[e];
      const int src = (int)(kd >> 1);
      const int pf = sel(cx.flg, buf)[src];
      if (kd & 1u) {
        parent = cx.newpos[src];
        fl = (pf & F_ROOT) ? F_PROOT : 0;
      } else {
        const int pp = sel(cx.par, buf)[src];
        parent = pp >= 0 ? cx.newpos[pp] : -1;
        fl = pf & (F_ROOT | F_PROOT);
        if (pp < 0 && !(pf & F_ROOT)) {
          // the parent node was not in the beam; it may have re-entered this
          // frame as a new child (the reference finds it through the trie)
          uint64_t pa, pb;
          hmix_inv(sel(cx.ha, nx)[k], sel(cx.hb, nx)[k], cx.elab[e], pa, pb);
          for (int q = (int)(pa & (uint64_t)(cx.hts - 1));; q = (q + 1) & (cx.hts - 1)) {
            const int c = cx.htab[q];
            if (c < 0) break;
            if (sel(cx.ha, nx)[c] == pa && sel(cx.hb, nx)[c] == pb) { parent = c; break; }
          }
        }
      }
      fl |= cx.eflg[e] & (F_HB | F_HN);
    };
    auto put_branch = [&](int k, int parent, int ef) {
      const int e = cx.sorted[k];
      const uint32_t kd = cx.ekind[e];
      sel(cx.lab, nx)[k] = cx.elab[e];
      sel(cx.par, nx)[k] = parent;
      sel(cx.flg, nx)[k] = ef;
      sel(cx.ot, nx)[k] = cx.et[e]; sel(cx.ob, nx)[k] = cx.eb[e]; sel(cx.ol, nx)[k] = cx.el[e];
      sel(cx.cb, nx)[k] = cx.ecb[e]; sel(cx.cn, nx)[k] = cx.ecn[e];
      if constexpr (SC::kStateful) sel(cx.est, nx)[k] = cx.eest[e];
      const uint32_t bpb = (ef & F_HB) ? cx.ebpb[e] : kBpNone, bpn = (ef & F_HN) ? cx.ebpn[e] : kBpNone;
#ifdef CTCX_GSTATE
      ((Rec16*)prm.rec)[((int64_t)b * prm.Tmax + CTCX_FRAME(t)) * W + k] = Rec16{kd, cx.elab[e], bpb, bpn};
#else
      const RT rc = RecOps<RT>::pack(kd, cx.elab[e], bpb, bpn);
      if (R > 0) rg.rec[(t & (R - 1)) * W + k] = rc;
      else rstream[(int64_t)CTCX_FRAME(t) * W + k] = rc;
#endif
    };
    if constexpr (STAGED) {
      // KM positions per lane, unrolled, so each phase's chains of dependent
      // LDS reads overlap across positions
      uint64_t nha[KM], nhb[KM];
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        nha[j] = nhb[j] = 0;
        if (tid + NT * j < n) hash_of(tid + NT * j, nha[j], nhb[j]);
      }
      if constexpr (INPLACE) __syncthreads();
#pragma unroll
      for (int j = 0; j < KM; ++j)
        if (tid + NT * j < n) put_hash(tid + NT * j, nha[j], nhb[j]);
      __syncthreads();
      int npar[KM], nfl[KM];
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        npar[j] = -1;
        nfl[j] = 0;
        if (tid + NT * j < n) parent_of(tid + NT * j, npar[j], nfl[j]);
      }
      if constexpr (INPLACE) __syncthreads();
#pragma unroll
      for (int j = 0; j < KM; ++j)
        if (tid + NT * j < n) put_branch(tid + NT * j, npar[j], nfl[j]);
    } else {
      for (int k = tid; k < n; k += NT) {
        uint64_t ha, hb;
        hash_of(k, ha, hb);
        put_hash(k, ha, hb);
      }
      __syncthreads();
      for (int k = tid; k < n; k += NT) {
        int parent, fl;
        parent_of(k, parent, fl);
        put_branch(k, parent, fl);
      }
    }
    if (R > 0 && tid == 0) rg.rn[t & (R - 1)] = n;
    __syncthreads();
    // kEarlyRecurse: the staged recursion into place, as recurse_wave0 would
    // leave entry k next frame.  Every read of e*[sorted[.]] above is behind
    // the barrier; nothing below reads an e* array, bst or bloom.  The two
    // back-pointers name entries by j: through the position map.
    if constexpr (kEr) {
      er_hit = er_place;
      if (er_place) {
        const CTCX_LDS int* sp = erw + 4;
        if (tid < n) {
          const int k = tid, j = erj;
          uint32_t qb = (uint32_t)sp[kErBpb * WC + j], qn = (uint32_t)sp[kErBpn * WC + j];
          if (qb < kBpRestart) qb = ((uint32_t)sp[kErPos * WC + ((qb >> 1) & (WC - 1))] << 1) | (qb & 1u);
          if (qn < kBpRestart) qn = ((uint32_t)sp[kErPos * WC + ((qn >> 1) & (WC - 1))] << 1) | (qn & 1u);
          cx.eb[k] = __uint_as_float((uint32_t)sp[kErNbk * WC + j]);
          cx.el[k] = __uint_as_float((uint32_t)sp[kErNl * WC + j]);
          cx.et[k] = __uint_as_float((uint32_t)sp[kErTot * WC + j]);
          cx.ecb[k] = __uint_as_float((uint32_t)sp[kErCb * WC + j]); cx.ebpb[k] = qb;
          cx.ecn[k] = __uint_as_float((uint32_t)sp[kErCn * WC + j]); cx.ebpn[k] = qn;
          cx.eflg[k] = sp[kErFlg * WC + j];
          cx.ekind[k] = ((uint32_t)k << 1);
          cx.elab[k] = sp[kErLab * WC + j];
          cx.bst[k] = 0;
          cx.bloom[k] = 0;
        }
      }
    }
    buf = nx;
    nb = n;
    dup = dup_next;
    for (int k = tid; k < nb; k += NT) cx.head[k] = -1;
    __syncthreads();
    for (int k = tid; k < nb; k += NT) {
      const int pp = sel(cx.par, buf)[k];
      if (pp >= 0 && (!dup || cx.alias[k] == k))
        cx.sib[k] = __hip_atomic_exchange(&cx.head[pp], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (R == 0) nrec_all += n;
    else if (t - flushed + 1 == R) {   // the ring is full: write its older half
      if constexpr (HW) {
        // the helper flushes during the next frame's grow (its rows stay intact
        // until that frame's commit, behind the barrier after exact_step)
        pf_t = t; pf_lo = flushed; pf_hi = flushed + R / 2 - 1; pf_fp = nflush;
      } else {
        ring_flush<KM>(rg, rstream, foff, t, flushed, flushed + R / 2 - 1, nullptr, 0, nflush, nrec);
      }
      flushed += R / 2;
      ++nflush;
    }
    __syncthreads();
    if (prof) { pc[4] += __builtin_amdgcn_s_memtime() - t3; pc[7] += 1; }
  }
#ifdef CTCX_PHASES
  if constexpr (HW) {   // diagnostics: where the two waves ran (HW_ID: SIMD in bits 5:4, CU in 11:8)
    if (tid == 64) misc[14] = (int)__builtin_amdgcn_s_getreg(63492);
    __syncthreads();
    if (prof) { pc[21] = (uint64_t)__builtin_amdgcn_s_getreg(63492); pc[22] = (uint64_t)(uint32_t)misc[14]; }
  }
#endif

  // TopPaths outputs (decoder.h:230-261); with no frames the root is the leaf
  if (sl == 0 && tid == 0) cx.tops[0] = 0;
  __syncthreads();
  const int np = (prm.P < n_leaves) ? prm.P : n_leaves;
  // the rest of the ring, walked from the TopPaths positions (HW: by the
  // helper, after the flush the last commit may have left pending; its
  // stream cursor is then the item's record count)
  if constexpr (HW) {
    if (R > 0 && sl > 0 && helper_wave()) {
      if (pf_t >= 0) ring_flush<(WC > 0 ? WC : 512) / 64, RT, true>(rg, rstream, foff, pf_t, pf_lo, pf_hi, nullptr, 0, pf_fp, nrec);
      ring_flush<(WC > 0 ? WC : 512) / 64, RT, true>(rg, rstream, foff, sl - 1, flushed, sl - 1, cx.tops, np, nflush, nrec);
      if (tid == 64) misc[13] = nrec;
    }
    __syncthreads();
    if (R > 0 && sl > 0) nrec = misc[13];
  } else {
    if (R > 0 && sl > 0) ring_flush<(WC > 0 ? WC : 512) / 64>(rg, rstream, foff, sl - 1, flushed, sl - 1, cx.tops, np, nflush, nrec);
  }
  for (int q = tid; q < prm.P; q += NT) {
    int pos = -1, kind = -1, opos = -1;
    T lp = T(0);
    if (q < np) {
      pos = cx.tops[q];
      opos = (R > 0 && sl > 0) ? (int)rg.sv[(nflush & 1) * W + pos] : pos;   // its record's stream position
      const int f = sel(cx.flg, buf)[pos];
      const bool hb = f & F_HB, hn = f & F_HN;
      if (hb && hn) kind = (sel(cx.cb, buf)[pos] > sel(cx.cn, buf)[pos]) ? 0 : 1;
      else if (hb) kind = 0;
      else if (hn) kind = 1;
      lp = sel(cx.ot, buf)[pos];
    }
    prm.top_pos[b * prm.P + q] = opos;
    prm.top_kind[b * prm.P + q] = kind;
    prm.log_prob[b * prm.P + q] = lp;
#ifdef CTCX_STREAM
    {   // ... and into the header, for a later push that brings this item no frame
      int32_t* hp = (int32_t*)(st_out + sizeof(CtcxStreamHdr));
      int64_t* hl = (int64_t*)(hp + 2 * prm.P);
      hp[q] = opos;
      hp[prm.P + q] = kind;
      hl[q] = 0;
      *(T*)(hl + q) = lp;
    }
#endif
  }
#ifdef CTCX_STREAM
  if (tid == 0) {
    CtcxStreamHdr ho{};
    ho.frames = t0g + sl;
    ho.buf = buf; ho.nb = nb; ho.dup = dup ? 1 : 0; ho.reserved0 = reserved0 ? 1 : 0;
    ho.n_leaves = n_leaves; ho.literal_steps = literal_steps; ho.dup_frames = dup_frames;
    ho.why_nonfinite = why_nf; ho.why_fill = why_fill; ho.records = nrec_all;
    if constexpr (kEr) ho.pad[0] = early_rec;
    *(CtcxStreamHdr*)st_out = ho;
  }
#ifndef CTCX_GSTATE
  {
    // the image: the whole LDS allocation as the chunk's last commit left it
    // (every wave is past the loop's closing barrier; nothing below writes LDS)
    char* img = st_out + st_hdr;
    const size_t nby = (size_t)prm.st.image_bytes, n16 = nby >> 4;
    for (size_t q = tid; q < n16; q += NT) ((u32x4*)img)[q] = ((const CTCX_LDS u32x4*)lds)[q];
    for (size_t q = (n16 << 2) + tid; q < (nby >> 2); q += NT) ((uint32_t*)img)[q] = ((const CTCX_LDS uint32_t*)lds)[q];
  }
#endif
#endif
  if (tid == 0) {
    ItemOut io;
    io.n_leaves = n_leaves;
    io.literal_steps = literal_steps;
    io.dup_frames = dup_frames;
    io.why_nonfinite = why_nf;
    io.why_fill = why_fill;
    io.records = R > 0 ? (int64_t)nrec : nrec_all;
#ifdef CTCX_SQ_CHECK
    io.dup_frames = cx.misc[15];
    io.why_nonfinite = g_sq_dbg[0];
    io.why_fill = g_sq_dbg[1];
    io.records = ((int64_t)(uint32_t)g_sq_dbg[2] << 32) | (uint32_t)g_sq_dbg[3];
    io.literal_steps = g_sq_dbg[4];
    io.n_leaves = n_leaves;
    io.why_nonfinite = (io.why_nonfinite & 0xffffff) | 0;
    io.dup_frames = g_sq_dbg[6];
    io.pad = 0;
    io.why_fill = (io.why_fill & 0xffffff);
    io.records = (io.records & ~0xffffffffll) | (uint32_t)g_sq_dbg[3];
    io.n_leaves = n_leaves;
    prm.log_prob[b * prm.P] = (T)__builtin_bit_cast(float, (unsigned)g_sq_dbg[7]);
#endif
    // HW kernels: a hand-over wait that gave up (the host fails the call)
    io.pad = HW ? __hip_atomic_load(&cx.misc[kCtlDead], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
    if constexpr (kEr) io.pad = (io.pad & 1) | (early_rec << 1);   // (item_early_frames)
    prm.item[b] = io;
  }
}

// ---------------------------------------------------------------------------
// Softmax normaliser per (t, b) row (decoder.h:72-80): sequential max, then a
// sequential sum of exp(x_j - max) in class order, norm = max + log(sum), with
// T's libm (float: expf/logf; double: exp/log).  Rows past an item's length
// are skipped.  The sums stay one thread per row (the reference's order), but
// the row data reaches the threads through LDS: one wave owns 64 consecutive
// rows and stages them in kNormTile-class tiles, tile rows read by coalesced
// 64-lane loads (the first build read C strided values per thread and
// reached ~0.2 TB/s).  Two passes over the tiles (max, then sum; for C > 64
// the max comes from ctcx_row_facts' header); for C <= kNormTile the row
// stays in LDS between them.  Every float term is exp of x_j - max <= 0 (or
// NaN): glibc's expf without its range branches (gm::expf_t_nonpos, checked
// against libm over every such input by tools/check_glibc_math.cpp).
__host__ __device__ __forceinline__ float norm_exp(float x) { return gm::expf(x); }
__host__ __device__ __forceinline__ double norm_exp(double x) { return gm::exp(x); }
__host__ __device__ __forceinline__ float norm_log(float x) { return gm::logf(x); }
__host__ __device__ __forceinline__ double norm_log(double x) { return gm::log(x); }

#ifndef CTCX_NORM_TILE
#define CTCX_NORM_TILE 32
#endif
// classes per tile: 32 (two rows per 64-lane load) keeps a wave's tile at 8.4
// KB of LDS (float), so LDS no longer caps the kernel at ~2 waves per SIMD
constexpr int kNormTile = CTCX_NORM_TILE;
constexpr int kNormRPL = 64 / kNormTile;   // tile rows per load instruction
constexpr int kNormNL = 64 / kNormRPL;     // load instructions per tile

// E: the element type of x in memory (T itself, or F16 / BF16 with T = float:
// widened as loaded, the arithmetic below is on the widened values)
template <typename T, typename E = T>
__global__ __launch_bounds__(64) void ctcx_row_norm(const E* __restrict__ x, const int32_t* seq_len,
                                                   T* __restrict__ norm, int64_t Tmax, int64_t B, int64_t C,
                                                   int64_t xst_t, int64_t xst_b, const char* __restrict__ prep) {
  __shared__ T tile[64][kNormTile + 1];   // [row in wave][class in tile], padded: conflict-free row reads
  __shared__ uint64_t etab[32];           // expf's 2^(i/32) table: the lanes' indices diverge
  const int lane = threadIdx.x;
  const int64_t rows = Tmax * B;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int64_t row = r0 + lane;
  if (lane < 32) etab[lane] = gm::exp2f_tab(lane);   // read after the first tile's barrier
  bool valid = false;
  int64_t off = 0;   // this lane's row, in elements of x
  if (row < rows) {
    const int64_t t = row / B, b = row - t * B;
    valid = t < seq_len[b];
    if (valid) off = t * xst_t + b * xst_b;
  }
  const uint64_t vmask = __ballot(valid);
  if (vmask == 0) return;
  // the row maximum: from the pre-pass's header (ctcx_row_facts, C > 64) when
  // the row holds no NaN / +inf (max is then order-free); otherwise pass 0
  // takes it in class order, as the reference's maxCoeff loop does
  T m = T(0), s = T(0);
  bool known = false;
  if (prep != nullptr && valid) {
    const RowHdr<T> h = *(const RowHdr<T>*)(prep + row * (int64_t)prep_row_bytes(C, (int)sizeof(T)));
    if (!h.bad) { m = h.xmax; known = true; }
  }
  const bool pass0 = __ballot(valid && !known) != 0ull;
  const int sub = lane / kNormTile, col = lane % kNormTile;   // a load's tile row (of kNormRPL) and class
  auto row_base = [&](int rr) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, rr);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)off >> 32), rr);
    return (int64_t)(((uint64_t)hi << 32) | lo);
  };
  auto load = [&](T (&v)[kNormNL], int64_t c0) {
    // tile rows q * kNormRPL + sub: one load per lane, sizeof(T) * nc
    // contiguous bytes per row (an invalid row reads x's first row instead
    // and is never used)
    const int nc = (int)(C - c0 < kNormTile ? C - c0 : kNormTile);
    const int cc = col < nc ? (int)c0 + col : 0;
#pragma unroll
    for (int q = 0; q < kNormNL; ++q) {
      int64_t base;
      if constexpr (kNormRPL == 1) {
        base = row_base(q);
      } else {
        const int64_t b0 = row_base(2 * q), b1 = row_base(2 * q + 1);
        base = sub ? b1 : b0;
      }
      v[q] = ldw<T>(x, base + cc);
    }
  };
  T v[kNormNL];
  for (int pass = pass0 ? 0 : 1; pass < 2; ++pass) {
    // the tile is (re)loaded unless C <= kNormTile and pass 0 left it in LDS;
    // the next tile's loads are issued before this tile's sums (software pipeline)
    const bool reload = pass == 0 || C > kNormTile || !pass0;
    if (reload) load(v, 0);
    for (int64_t c0 = 0; c0 < C; c0 += kNormTile) {
      const int nc = (int)(C - c0 < kNormTile ? C - c0 : kNormTile);
      if (reload) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kNormNL; ++q) tile[q * kNormRPL + sub][col] = v[q];
        __syncthreads();
        if (c0 + kNormTile < C) load(v, c0 + kNormTile);
      }
      if (valid) {
        if (pass == 0) {
          if (!known) {
            int j = 0;
            if (c0 == 0) { m = tile[lane][0]; j = 1; }
            for (; j < nc; ++j) { const T e = tile[lane][j]; m = (e > m) ? e : m; }
          }
        } else if constexpr (sizeof(T) == 4) {
          if (nc == kNormTile) {
            // a whole tile: the exp terms are independent (computed 16 at a
            // time, in flight together), only the sum is a chain, in class order
#pragma unroll
            for (int j0 = 0; j0 < kNormTile; j0 += 16) {
              T e[16];
#pragma unroll
              for (int j = 0; j < 16; ++j) e[j] = gm::expf_t_nonpos(tile[lane][j0 + j] - m, etab);
#pragma unroll
              for (int j = 0; j < 16; ++j) s += e[j];
            }
          } else {
            for (int j = 0; j < nc; ++j) s += gm::expf_t_nonpos(tile[lane][j] - m, etab);
          }
        } else {
          for (int j = 0; j < nc; ++j) s += norm_exp(tile[lane][j] - m);
        }
      }
    }
  }
  if (valid) norm[row] = m + norm_log(s);
}

// ctcx_row_norm for float rows of whole float4s (C % 4 == 0, 16-byte
// aligned): the same 32-class tiles and class-order sums, moved as 16-byte
// pieces -- a load instruction covers 8 rows (8 lanes x 16 B each), so 8 loads,
// 8 LDS writes and 8 LDS reads per lane per tile instead of 32 of each, and
// each lane's 8 row bases are fetched once, not per tile.  E = F16 / BF16:
// the four classes of a piece are 8 bytes in memory (rows 8-byte aligned),
// widened to the same float4.
constexpr int kNormTileW4 = kNormTile + 4;   // 16-byte rows; 36 words apart, b128 row reads conflict-free
template <typename E = float>
__global__ __launch_bounds__(64) void ctcx_row_norm_v4(const E* __restrict__ x, const int32_t* seq_len,
                                                      float* __restrict__ norm, int64_t Tmax, int64_t B, int64_t C,
                                                      int64_t xst_t, int64_t xst_b, const char* __restrict__ prep) {
  static_assert(kNormTile == 32, "8 lanes of 16 bytes per tile row");
  __shared__ __attribute__((aligned(16))) float tile[64][kNormTileW4];
  __shared__ uint64_t etab[32];
  const int lane = threadIdx.x;
  const int64_t rows = Tmax * B;
  const int64_t row = (int64_t)blockIdx.x * 64 + lane;
  if (lane < 32) etab[lane] = gm::exp2f_tab(lane);   // read after the first tile's barrier
  bool valid = false;
  int64_t off = 0;   // this lane's row, in floats of x (an invalid row: x's first row, never used)
  if (row < rows) {
    const int64_t t = row / B, b = row - t * B;
    valid = t < seq_len[b];
    if (valid) off = t * xst_t + b * xst_b;
  }
  if (__ballot(valid) == 0ull) return;
  float m = 0.f, s = 0.f;
  bool known = false;
  if (prep != nullptr && valid) {
    const RowHdr<float> h = *(const RowHdr<float>*)(prep + row * (int64_t)prep_row_bytes(C, 4));
    if (!h.bad) { m = h.xmax; known = true; }
  }
  const bool pass0 = __ballot(valid && !known) != 0ull;
  // every row of the wave with its maximum from the header and finite (no
  // NaN / +inf in the row, not all -inf): no term is NaN, expf_t_le0 serves
  const bool le0 = __ballot(valid && !(known && m > -__builtin_inff())) == 0ull;
  // load q covers tile rows 8 q + sub, classes c4 .. c4 + 3 of the tile
  const int sub = lane >> 3, c4 = (lane & 7) * 4;
  const E* base[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int src = 8 * q + sub;
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)off, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)off >> 32), src);
    base[q] = x + (int64_t)(((uint64_t)hi << 32) | lo) + c4;
  }
  auto load = [&](float4 (&v)[8], int64_t c0) {
    const bool in = c4 < C - c0;   // (C - c0 is a multiple of 4)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if constexpr (std::is_same<E, float>::value) {
        v[q] = in ? *(const float4*)(base[q] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const u32x2 w = in ? *(const u32x2*)(base[q] + c0) : u32x2{0u, 0u};
        unsigned f0, f1, f2, f3;
        widen2<E>(w[0], f0, f1);
        widen2<E>(w[1], f2, f3);
        v[q] = make_float4(__uint_as_float(f0), __uint_as_float(f1), __uint_as_float(f2), __uint_as_float(f3));
      }
    }
  };
  float4 v[8];
  for (int pass = pass0 ? 0 : 1; pass < 2; ++pass) {
    const bool reload = pass == 0 || C > kNormTile || !pass0;
    if (reload) load(v, 0);
    for (int64_t c0 = 0; c0 < C; c0 += kNormTile) {
      const int nc = (int)(C - c0 < kNormTile ? C - c0 : kNormTile);
      if (reload) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) *(float4*)&tile[8 * q + sub][c4] = v[q];
        __syncthreads();
        if (c0 + kNormTile < C) load(v, c0 + kNormTile);
      }
      if (valid) {
        if (pass == 0) {
          if (!known) {
            int j = 0;
            if (c0 == 0) { m = tile[lane][0]; j = 1; }
            for (; j < nc; ++j) { const float e = tile[lane][j]; m = (e > m) ? e : m; }
          }
        } else if (nc == kNormTile) {
          // a whole tile: 16 exp terms in flight at a time, the sum in class order
          auto tile_sum = [&](auto expf_fn) __attribute__((always_inline)) {
#pragma unroll
            for (int j0 = 0; j0 < kNormTile; j0 += 8) {
              float e[8];
#pragma unroll
              for (int i = 0; i < 2; ++i) {
                const float4 w = *(const float4*)&tile[lane][j0 + 4 * i];
                e[4 * i + 0] = expf_fn(w.x - m);
                e[4 * i + 1] = expf_fn(w.y - m);
                e[4 * i + 2] = expf_fn(w.z - m);
                e[4 * i + 3] = expf_fn(w.w - m);
              }
#pragma unroll
              for (int j = 0; j < 8; ++j) s += e[j];
            }
          };
          if (le0) {
            // KB terms at a time; when none lies below expf's underflow bound
            // (N(0,1) rows: x - max > -20) the core path alone, no select
            // (cfg5 6.28 -> 6.05 ms; at 164 VGPRs, three waves per SIMD: held
            // to four by a waves-per-EU bound it spills and takes 7.96)
            constexpr int KB = 16;
#pragma unroll
            for (int j0 = 0; j0 < kNormTile; j0 += KB) {
              float d[KB], e[KB];
#pragma unroll
              for (int i = 0; i < KB / 4; ++i) {
                const float4 w = *(const float4*)&tile[lane][j0 + 4 * i];
                d[4 * i + 0] = w.x - m;
                d[4 * i + 1] = w.y - m;
                d[4 * i + 2] = w.z - m;
                d[4 * i + 3] = w.w - m;
              }
              float mn = d[0];
#pragma unroll
              for (int j = 1; j < KB; ++j) mn = __builtin_fminf(mn, d[j]);
              if (__ballot(valid && mn < gm::kExpfUnder) == 0ull) {   // uniform
#pragma unroll
                for (int j = 0; j < KB; ++j) e[j] = gm::expf_t_core(d[j], etab);
              } else {
#pragma unroll
                for (int j = 0; j < KB; ++j) e[j] = gm::expf_t_le0(d[j], etab);
              }
#pragma unroll
              for (int j = 0; j < KB; ++j) s += e[j];
            }
          } else {
            tile_sum([&](float v) __attribute__((always_inline)) { return gm::expf_t_nonpos(v, etab); });
          }
        } else {
          for (int j = 0; j < nc; ++j) s += gm::expf_t_nonpos(tile[lane][j] - m, etab);
        }
      }
    }
  }
  if (valid) norm[row] = m + gm::logf(s);
}

#if CTCX_PART == 0
// ---------------------------------------------------------------------------
// Large C (> 64): everything the decode kernel needs per row that depends on
// the row alone, one wave per (t, b) row, fully parallel over rows (inside
// the decode kernel the same work sat on the one-wave T-serial chain; at
// C=5000 the top-set bisection alone took ~108k cycles per frame there):
//   * the softmax normaliser (decoder.h:72-80; replaces ctcx_row_norm for
//     these rows): the exp terms in parallel, then one lane sums them in class
//     order, as the reference does;
//   * RowHdr: the row maximum, the NaN / +inf test, |S| and the largest value
//     outside S;
//   * the 64-class block maxima;
//   * S (float rows): bisection on the order-preserving integer key of the
//     float for the smallest tau with |{non-blank x : key >= tau}| <= K =
//     kTopK; any bracket keeping cnt(lo) > K >= cnt(hi) yields the
//     same S (the row's K largest values without a tie across the boundary).
// The row is staged in LDS (batches of loads in flight) when it fits
// (kPrepLdsBytes); wider rows are read from global memory.  Rows past an
// item's length are skipped (never read).
constexpr size_t kPrepLdsBytes = 128 * 1024;
constexpr int kPrepBatch = 16;     // loads in flight per lane while staging
constexpr int kPrepCompact = 256;  // keys at or above the bracket's lower end, bisected in registers
constexpr size_t kPrepTabBytes = 256;  // LDS copy of expf's 2^(i/32) table

__device__ __forceinline__ unsigned fkey(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// fkey through the sign's arithmetic shift: u ^ (sx | 0x80000000), sx = 0 or ~0
__device__ __forceinline__ unsigned fkey_sx(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}

template <typename T, bool INLDS, typename E = T>
__global__ __launch_bounds__(64) void ctcx_row_prep(const E* __restrict__ x, const int32_t* __restrict__ seq_len,
                                                   char* __restrict__ prep, T* __restrict__ norm, int64_t B,
                                                   int64_t C, int64_t xst_t, int64_t xst_b, int blank) {
  // LDS: the expf table (32 x 8 bytes), the staged row, the compact key list
  extern __shared__ __attribute__((aligned(16))) char plds[];
  uint64_t* etab = (uint64_t*)plds;
  T* xs = (T*)(plds + kPrepTabBytes);
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t t = row / B, b = row - t * B;
  if (t >= seq_len[b]) return;
  const T NI = ninf<T>();
  const int Ci = (int)C;
  const E* xr = x + (t * xst_t + b * xst_b);   // (E = F16 / BF16: widened by every read below)
  char* pr = prep + row * (int64_t)prep_row_bytes(C, (int)sizeof(T));
  T* bm = (T*)(pr + prep_bmax_offset((int)sizeof(T)));
  const int nblk = (Ci + 63) / 64;
  constexpr bool inlds = INLDS;   // the launcher's choice: C * sizeof(T) <= kPrepLdsBytes
  if (lane < 32) etab[lane] = gm::exp2f_tab(lane);   // read after the staging barrier
  if (inlds) {
    for (int j0 = 0; j0 < Ci; j0 += 64 * kPrepBatch) {
      T v[kPrepBatch];
#pragma unroll
      for (int u = 0; u < kPrepBatch; ++u) {
        const int j = j0 + 64 * u + lane;
        v[u] = j < Ci ? ldw<T>(xr, j) : T(0);
      }
#pragma unroll
      for (int u = 0; u < kPrepBatch; ++u) {
        const int j = j0 + 64 * u + lane;
        if (j < Ci) xs[j] = v[u];
      }
    }
    __syncthreads();
  }
  auto xat = [&](int j) -> T { return inlds ? xs[j] : ldw<T>(xr, j); };
  // maximum, NaN / +inf, block maxima (block k: classes [64k, 64k + 64)),
  // and (float) the lane's largest non-blank key
  T xmax = NI, bmv = NI;
  bool bad = false, nan = false;
  unsigned lkmax = 0u;
  for (int k0 = 0; k0 < nblk; k0 += 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = (k0 + u) * 64 + lane;
      v[u] = (k0 + u < nblk && j < Ci) ? xat(j) : NI;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      if (k >= nblk) break;
      nan |= v[u] != v[u];
      bad |= (v[u] != v[u]) || (v[u] == pinf<T>());
      xmax = v[u] > xmax ? v[u] : xmax;
      if constexpr (sizeof(T) == 4) {
        const int j = k * 64 + lane;
        const unsigned kv = fkey((float)v[u]);
        if (j < Ci && j != blank && kv > lkmax) lkmax = kv;
      }
      const T m = wave_max_dpp(v[u]);
      bmv = (lane == (k & 63)) ? m : bmv;
      if ((k & 63) == 63 || k == nblk - 1) {
        if (lane <= (k & 63)) bm[(k & ~63) + lane] = bmv;
      }
    }
  }
  RowHdr<T> h;
  h.xmax = wave_max_dpp(xmax);
  h.bad = __ballot(bad) != 0ull;
  h.ns = 0;
  h.xout = pinf<T>();
  if constexpr (sizeof(T) == 4) {
    const int Cm1 = Ci - 1;
    const int K = kTopK;
    // |{non-blank labels with key >= tau}|: per-lane counts, then one wave sum
    auto cnt_ge = [&](unsigned tau) {
      int c = 0;
      int j = lane;
      for (; j + 64 * 7 < Ci; j += 64 * 8) {   // 8 reads in flight
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = xat(j + 64 * u);
#pragma unroll
        for (int u = 0; u < 8; ++u) c += (j + 64 * u != blank && fkey(v[u]) >= tau) ? 1 : 0;
      }
      for (; j < Ci; j += 64) c += (j != blank && fkey(xat(j)) >= tau) ? 1 : 0;
      return uni(wave_sum_dpp(c));
    };
    uint64_t lo = 0, hi = 0;
    if (Cm1 > K) {
      static_assert(kTopK == 64, "the bracket below takes one key per lane");
      hi = (uint64_t)fkey(h.xmax) + 1ull;   // cnt(hi) = 0
      // the smallest lane maximum km has at least 64 keys at or above it (one
      // per lane: each lane's largest); Cm1 > 64 gives every lane a label
      const unsigned km = (unsigned)uni((int)wave_min_dpp(lkmax));
      const int ckm = cnt_ge(km);
      if (ckm == K) {
        lo = km - 1;   // exactly the K largest: tau = km
        hi = km;
      } else {
        lo = km;       // cnt(km) > K
        CTCX_LDS unsigned* cks =
            (CTCX_LDS unsigned*)(plds + kPrepTabBytes + (INLDS ? ((size_t)C * sizeof(T) + 15) & ~(size_t)15 : 0));
        if (ckm <= kPrepCompact) {
          // every key >= km into a compact list (at most kPrepCompact), then
          // bisect in registers: tau > km, so S lies in the list
          int n = 0;
          for (int j0 = 0; j0 < Ci; j0 += 64) {
            const int j = j0 + lane;
            const unsigned kv = j < Ci ? fkey(xat(j)) : 0u;
            const bool in = j < Ci && j != blank && kv >= km;
            const uint64_t m = __ballot(in);
            if (in) cks[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = kv;
            n += __builtin_popcountll(m);
          }
          __syncthreads();
          unsigned ck[kPrepCompact / 64];
#pragma unroll
          for (int q = 0; q < kPrepCompact / 64; ++q) ck[q] = 64 * q + lane < n ? cks[64 * q + lane] : 0u;
          while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            int c = 0;
#pragma unroll
            for (int q = 0; q < kPrepCompact / 64; ++q) c += ck[q] >= (unsigned)mid ? 1 : 0;
            c = uni(wave_sum_dpp(c));
            if (c <= K) hi = mid;
            else lo = mid;
            if (c == K) break;
          }
        } else {
          while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            const int c = cnt_ge((unsigned)mid);
            if (c <= K) hi = mid;
            else lo = mid;
            if (c == K) break;
          }
        }
      }
    }
    const unsigned tau = (unsigned)hi;
    uint2* top = (uint2*)(pr + prep_top_offset(C, 4));
    float xo = ninf<float>();
    int n = 0;
    for (int x0 = 0; x0 < Cm1; x0 += 64) {
      const int xi = x0 + lane;
      bool in = false;
      float v = 0.f;
      if (xi < Cm1) {
        v = xat(xi + (xi >= blank ? 1 : 0));
        in = fkey(v) >= tau;
        if (!in) xo = v > xo ? v : xo;
      }
      const uint64_t m = __ballot(in);
      if (in) {
        const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        top[n + r] = make_uint2(__float_as_uint(v), (unsigned)xi);
      }
      n += __builtin_popcountll(m);
    }
    h.ns = n;
    h.xout = wave_max_dpp(xo);
  }
  if (lane == 0) *(RowHdr<T>*)pr = h;
  // the normaliser: m = the row maximum -- in class order when a NaN is
  // present (max is order-free otherwise), as ctcx_row_norm and the reference
  // take it -- then s = sum of exp(x_j - m) in class order, norm = m + log(s)
  T m = h.xmax;
  if (__ballot(nan) != 0ull) {
    m = xat(0);
    for (int j = 1; j < Ci; ++j) {
      const T v = xat(j);
      m = (v > m) ? v : m;
    }
  }
  T ssum = T(0);
  if (inlds) {
    __syncthreads();
    for (int j = lane; j < Ci; j += 64) {
      if constexpr (sizeof(T) == 4) xs[j] = gm::expf_t_nonpos(xs[j] - m, etab);   // glibc expf, its table in LDS
      else xs[j] = norm_exp(xs[j] - m);
    }
    __syncthreads();
    if (lane == 0) {
      int j = 0;
      for (; j + 16 <= Ci; j += 16) {
        T e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = xs[j + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) ssum += e[u];
      }
      for (; j < Ci; ++j) ssum += xs[j];
    }
  } else if (lane == 0) {
    for (int j = 0; j < Ci; ++j) ssum += norm_exp(ldw<T>(xr, j) - m);
  }
  if (lane == 0) norm[row] = m + norm_log(ssum);
}

// ---------------------------------------------------------------------------
// ctcx_row_facts: ctcx_row_prep's row facts (RowHdr, block maxima, the top
// set S) for float rows with C % 4 == 0 and C <= 256 * NV, with the row in
// registers instead of LDS: lane L holds classes 4 (64 u + L) + c of the row
// (float4 loads, u < NV, c < 4), all NV loads in flight at once, and every
// pass over the row (maxima, counts, S) runs on those registers.  A 64-class
// block is one 16-lane DPP row of one u, so the block maxima are DPP row
// reductions.  The normaliser is left to ctcx_row_norm (rows per lane, the
// class-order sum spread over 64 rows at a time, the maximum taken from the
// header written here): the one-lane class-order sum of ctcx_row_prep was the
// bulk of its time.  Four rows per 256-thread block, one per wave.
// keys at or above the first bracket's lower end (the smallest lane maximum)
// kept for the radix select: at C = 5000, N(0,1) rows hold ~270 of them,
// past ctcx_row_prep's 256 (whose fallback bisects over all C keys)
#ifndef CTCX_FACTS_WPE
#define CTCX_FACTS_WPE 1
#endif
// (768: the block's lists in 30 KB, five blocks per CU -- cfg5's rows
// gather ~270 keys; a row past it bisects instead.  1024 held four: c3k
// 1.07 -> 0.98 ms, cfg5 7.09 -> 6.97 ms)
#ifndef CTCX_FACTS_COMPACT
#define CTCX_FACTS_COMPACT 768
#endif
constexpr int kFactsCompact = CTCX_FACTS_COMPACT;
// The (rank)-th largest of the n keys of a wave's compact list (rank <= n):
// MSB-first radix select, 8-bit digits, a 256-bin LDS histogram per pass.
// Every key lies in [klo, khi], so the bits above their highest differing bit
// are common and skipped (three passes for the N(0,1) rows at C = 5000).
__device__ __forceinline__ unsigned radix_select_desc(const unsigned* cks, int n, int rank, unsigned klo,
                                                      unsigned khi, unsigned* hist) {
  const int lane = threadIdx.x & 63;
  const unsigned diff = klo ^ khi;
  if (diff == 0u) return klo;
  int rem = 32 - __builtin_clz(diff);   // bits below the common prefix
  unsigned pfx = rem == 32 ? 0u : (klo >> rem) << rem;
  const int nq = (n + 63) >> 6;
  auto wsync_lds = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  while (rem > 0) {
    const int wd = rem < 8 ? rem : 8;
    const int sh = rem - wd;
    ((uint4*)hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
    wsync_lds();
    for (int q = 0; q < nq; ++q) {
      const int j = 64 * q + lane;
      const unsigned kv = cks[j < n ? j : 0];
      // the key matches the digits chosen so far: its bits at and above sh + wd equal pfx's
      const bool match = j < n && (((uint64_t)(kv ^ pfx) >> (sh + wd)) == 0ull);
      if (match)
        __hip_atomic_fetch_add(&hist[(kv >> sh) & ((1u << wd) - 1u)], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    wsync_lds();
    const uint4 hb = ((const uint4*)hist)[lane];   // bins 4 lane .. 4 lane + 3
    const int tl = (int)(hb.x + hb.y + hb.z + hb.w);
    // inclusive suffix sum over lanes: the keys in bins >= 4 lane
    int sfx = tl;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(sfx, d);
      sfx += lane + d < 64 ? o : 0;
    }
    const int above = sfx - tl;   // keys in the bins of the lanes above
    const uint64_t hit = __ballot(above < rank && rank <= sfx);
    const int L = __builtin_ctzll(hit);
    int dg, ab;   // the digit, the keys in the bins above it
    if (above + (int)hb.w >= rank) { dg = 3; ab = above; }
    else if (above + (int)(hb.w + hb.z) >= rank) { dg = 2; ab = above + (int)hb.w; }
    else if (above + (int)(hb.w + hb.z + hb.y) >= rank) { dg = 1; ab = above + (int)(hb.w + hb.z); }
    else { dg = 0; ab = above + (int)(hb.w + hb.z + hb.y); }
    dg = __builtin_amdgcn_readlane(4 * lane + dg, L);
    ab = __builtin_amdgcn_readlane(ab, L);
    rank -= ab;
    pfx |= (unsigned)dg << sh;
    rem = sh;
    wsync_lds();   // the histogram is cleared again only after every lane has read it
  }
  return pfx;
}

// FUSE: the softmax normaliser too (decoder.h:72-80), from the rows the waves
// already hold, so the logits are read from HBM once (ctcx_row_norm's second
// read goes).  The sum stays in class order, one lane per row: after the
// facts, the block's rows (two per wave) pass through LDS 256 classes at a
// time as exp terms (two tile buffers; these rows bisect their top set in
// registers, with no compact list), lane q of wave 0 adding row q's tile in
// class order while the
// waves write the next one.  A row holding a NaN or +inf (max then in class
// order) is summed from global memory by its wave's lane 0.  That chain, C
// dependent adds per block, is the fused kernel's cost: the launcher fuses
// rows of up to 1024 classes (kFuseNorm; cfg4 0.90 -> 0.75 ms), and past them
// the second read is cheaper (cfg5 19.4 ms fused against 8.5 + 8.7 split).
constexpr int kNormTileW = 260;   // floats per tile row: 256 classes + 4 (rows 4 banks apart)
// f(integral_constant<int, U>) for U in the sequence, in order
template <typename F, int... U>
__device__ __forceinline__ void unroll_seq(F& f, std::integer_sequence<int, U...>) {
  (f(std::integral_constant<int, U>{}), ...);
}
// rows per wave: two for the fused kernel's small rows (NV <= 4), whose
// loads are then in flight together (twice the bytes per wave), and whose
// normaliser chains are then eight per block
template <int NV, bool FUSE>
constexpr int facts_rows_per_wave() { return (FUSE && NV <= 4) ? 2 : 1; }
// the row widths the launcher fuses the normaliser for (C <= 1024)
template <int NV>
constexpr bool kFuseNorm = NV <= 4;

// E = F16 / BF16: the row's 2-byte elements, four per lane and load (8 bytes,
// rows 8-byte aligned), widened into the same registers; all else as for float.
template <int NV, bool FUSE, typename E = float>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CTCX_FACTS_WPE, 8))) void ctcx_row_facts(
    const E* __restrict__ x, const int32_t* __restrict__ seq_len, char* __restrict__ prep, int64_t rows,
    int64_t B, int C, int64_t xst_t, int64_t xst_b, int blank, float* __restrict__ norm) {
  // per wave: the compact list of (key, label index) in label order, with one
  // dummy slot per lane (its stores are unconditional), and the radix histogram
  // (NV <= 4, C <= 1024: 16 keys per lane, bisected in registers as cheaply
  // as a radix select's fixed passes, and no LDS: more waves per SIMD)
  constexpr bool kRadix = NV > 4;
  constexpr int R = facts_rows_per_wave<NV, FUSE>();
  constexpr int NR = 4 * R;   // rows per block: row r * 4 + wave of the block's
  constexpr int kCks = FUSE ? 2 * R * kNormTileW : 1;
  static_assert(!FUSE || 4 * kCks >= 2 * NR * kNormTileW, "the tile buffers fit");
  static_assert(!(FUSE && kRadix), "the normaliser is fused for NV <= 4 only (kFuseNorm)");
  __shared__ __attribute__((aligned(16))) unsigned cks_all[4][kCks];   // FUSE: the tile buffers
  // the compact list: a key plane and a label-index plane a constant
  // 17 x 256 B apart, so each pair of stores is one ds_write2st64_b32
  constexpr int kList = kRadix ? kFactsCompact + 64 : 1;
  static_assert(!kRadix || (kList * 4) % 256 == 0, "planes 256-byte multiples apart");
  __shared__ unsigned ckl_all[4][2][kList];
  __shared__ unsigned hist_all[4][kRadix ? 256 : 1];
  __shared__ uint64_t etab[FUSE ? 32 : 1];   // expf's table (read after the first tile barrier)
  __shared__ float rmax[FUSE ? NR : 1];   // the rows' maxima, for the summing lanes
  __shared__ int rsum[FUSE ? NR : 1];     // the rows they sum (live, no NaN / +inf)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float NI = -__builtin_inff(), PI = __builtin_inff();
  const int C4 = C >> 2;
  if constexpr (FUSE) {
    if (threadIdx.x < 32) etab[threadIdx.x] = gm::exp2f_tab(threadIdx.x);
  }
  // the rows, then their keys: fkey of each non-blank class, 0 for the blank
  // and the padding (fkey is order-preserving; 0 is the key of one NaN pattern
  // only, and a row holding a NaN is decoded literally, without S)
  unsigned kr[R][NV][4];
  int64_t rrow[R];
  bool live[R], rbad[R];
  float rxmax[R], xbv[R];   // FUSE: the blank's value, whose key is 0, for its exp term
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = (int64_t)blockIdx.x * NR + r * 4 + wv;
    const int64_t t = row / B, b = row - t * B;
    rrow[r] = row;
    if constexpr (FUSE) {
      live[r] = row < rows && t < seq_len[b];   // wave-uniform; every wave reaches the tile barriers below
    } else {
      if (row >= rows) return;   // wave-uniform, and no block barrier below
      if (t >= seq_len[b]) return;
      live[r] = true;
    }
    rbad[r] = false;
    rxmax[r] = NI;
    xbv[r] = 0.f;
    if (live[r]) {
      const E* xr = x + (t * xst_t + b * xst_b);
      if constexpr (FUSE) xbv[r] = ldw<float>(xr, blank);
      // buffer loads: one lane offset and a constant row offset per load, no
      // 64-bit address per load in flight (those took 40 VGPRs at NV = 20); past
      // the row they return 0, replaced by -inf below
      // (the extent is the row's bytes: C * sizeof(E), a whole number of loads
      // per lane since C % 4 == 0, so a load lies wholly inside or outside it)
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc((void*)xr, (short)0, C * (int)sizeof(E), 0x00020000);
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        if constexpr (std::is_same<E, float>::value) {
          const auto f = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, u * 1024, 0);
          kr[r][u][0] = f[0]; kr[r][u][1] = f[1]; kr[r][u][2] = f[2]; kr[r][u][3] = f[3];
        } else {
          const auto f = __builtin_amdgcn_raw_buffer_load_b64(rs, lane * 8, u * 512, 0);
          widen2<E>(f[0], kr[r][u][0], kr[r][u][1]);
          widen2<E>(f[1], kr[r][u][2], kr[r][u][3]);
        }
      }
    }
  }
  // the facts of each row, k its values (keys after)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!live[r]) continue;   // wave-uniform
    const int64_t row = rrow[r];
    unsigned (&k)[NV][4] = kr[r];
    char* pr = prep + row * (int64_t)prep_row_bytes(C, 4);
    float* bm = (float*)(pr + prep_bmax_offset(4));
    uint2* top = (uint2*)(pr + prep_top_offset(C, 4));
    const int nblk = (C + 63) / 64;
    // maximum, NaN / +inf, the block maxima (block 4 u + (lane >> 4) is the
    // 16-lane DPP row of one u: its maximum lands on the row's lane 15), and
    // the lane's largest key
    float xmax = NI;
    bool bad = false;
    unsigned lk = 0u;
    const int bl4 = blank - 4 * lane;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      float lm = NI;
      // (a u wholly inside the row, the common case: no per-element row test)
      auto keys = [&](auto whole) __attribute__((always_inline)) {
        const bool inrow = decltype(whole)::value || 64 * u + lane < C4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float v = inrow ? __uint_as_float(k[u][c]) : NI;
          bad |= (v != v) || (v == PI);
          // the maxima by v_max_f32 (a NaN loses, as in v > lm ? v : lm; of
          // +0 / -0 either: nothing reads a maximum's zero sign)
          lm = __builtin_fmaxf(lm, v);
          // the blank's key is cleared below, in the one lane holding it
          const unsigned kv = fkey_sx(v);
          k[u][c] = inrow ? kv : 0u;
        }
      };
      if (64 * u + 64 <= C4) keys(std::true_type{});   // uniform
      else keys(std::false_type{});
      xmax = __builtin_fmaxf(xmax, lm);
      lm = row16_fmax_dpp(lm);
      const int kb = 4 * u + (lane >> 4);
      if ((lane & 15) == 15 && 64 * u < C4 && kb < nblk) bm[kb] = lm;
    }
    // the blank's key to 0 (it is no label): class 4 lane + 256 u + c, found
    // by uniform tests on u and c and one lane select (not a compare per key)
    {
      const int ub = blank >> 8, cb = blank & 3, lbk = (blank >> 2) & 63;
#pragma unroll
      for (int u = 0; u < NV; ++u)
        if (u == ub) {   // uniform
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c == cb) k[u][c] = lane == lbk ? 0u : k[u][c];
        }
    }
    auto umax = [](unsigned a, unsigned b) { return a > b ? a : b; };   // (pairs become v_max3_u32)
#pragma unroll
    for (int u = 0; u < NV; ++u) lk = umax(umax(lk, k[u][0]), umax(umax(k[u][1], k[u][2]), k[u][3]));
    RowHdr<float> h;
    h.xmax = wave_fmax_dpp(xmax);
    h.bad = __ballot(bad) != 0ull;
    const int K = kTopK;
    auto unkey = [](unsigned kv) { return kv ^ ((kv >> 31) ? 0x80000000u : 0xFFFFFFFFu); };   // fkey's inverse
    const uint64_t ltm = (1ull << lane) - 1ull;
    // S = the keys >= tau, tau the smallest threshold with |S| <= K: one past
    // the (K+1)-th largest key v, and the largest key outside S is then v
    // itself (C - 1 <= K: every label, nothing outside).  The smallest lane
    // maximum km bounds v from below: one key per lane at or above it (when
    // every lane holds a label, C >= 256; else km = 0 and the bound is 1).
    const unsigned km = (unsigned)uni((int)wave_min_dpp(lk));
    const unsigned kmx = (unsigned)uni((int)~wave_min_dpp(~lk));   // the largest key
    const unsigned kt = km > 1u ? km : 1u;
    // every key >= kt into the compact list, in label order (within a u, label
    // order is (lane, c) order): a label's slot is the count before it
    unsigned* cks = ckl_all[wv][0];   // keys; labels at cks[kList + j]
    int n = 0;   // keys >= kt
    int lb4;   // 4 lane, opaque: recomputed here, not kept from the first pass
    __asm__ volatile("v_lshlrev_b32 %0, 2, %1" : "=v"(lb4) : "v"(lane));
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (kRadix && 64 * u < C4) {   // uniform
        bool in[4];
        uint64_t mm[4];
        // the list slot of this lane's first key: n plus the keys in lower
        // lanes, the four counts chained through mbcnt's accumulator
        unsigned acc = (unsigned)n;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          in[c] = k[u][c] >= kt;
          mm[c] = __ballot(in[c]);
          acc = __builtin_amdgcn_mbcnt_hi((unsigned)(mm[c] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm[c], acc));
        }
        int at = (int)acc;
        // (room for all of this u's 256 keys: no capacity test per key)
        auto put = [&](auto room) __attribute__((always_inline)) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            // the class (4 lane + 256 u + c); its label index (less one past
            // the blank) is taken when S is written, not per key
            const int j = (in[c] && (decltype(room)::value || at < kFactsCompact)) ? at : kFactsCompact + lane;
            cks[j] = k[u][c];
            cks[kList + j] = (unsigned)(lb4 + (256 * u + c));
            at += in[c] ? 1 : 0;
          }
        };
        if (n + 256 <= kFactsCompact) put(std::true_type{});   // uniform
        else put(std::false_type{});
#pragma unroll
        for (int c = 0; c < 4; ++c) n += __builtin_popcountll(mm[c]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (kRadix && n <= kFactsCompact && (n > K || C - 1 <= K)) {
      // S from the list: all of it (C - 1 <= K), or the keys above the
      // (K+1)-th largest, found by a radix select over the list
      unsigned v = 0u;
      if (C - 1 > K) v = radix_select_desc(cks, n, K + 1, kt, kmx, hist_all[wv]);
      int ns = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const unsigned kv = j < n ? cks[j] : 0u;
        const bool in = j < n && kv > v;
        const uint64_t mm = __ballot(in);
        if (in) {
          const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm, 0u));
          const unsigned cl = cks[kList + j];
          top[ns + r] = make_uint2(unkey(kv), cl - (cl > (unsigned)blank ? 1u : 0u));
        }
        ns += __builtin_popcountll(mm);
      }
      h.ns = ns;
      h.xout = v == 0u ? NI : __uint_as_float(unkey(v));
    } else {
      // NV <= 4, and the rare shapes: exactly K keys at or above km (S is the
      // list, its outside maximum taken from the registers), or a list past its
      // capacity (tau bisected over the row's keys, S from the registers)
      auto cnt_ge = [&](unsigned tau) __attribute__((always_inline)) {
        int c2 = 0;
#pragma unroll
        for (int u = 0; u < NV; ++u)
#pragma unroll
          for (int c = 0; c < 4; ++c) c2 += k[u][c] >= tau ? 1 : 0;
        return uni(wave_sum_dpp(c2));
      };
      if constexpr (!kRadix) n = cnt_ge(kt);
      unsigned tau = kt;
      if (n > K) {
        uint64_t lo = kt - 1u, hi = (uint64_t)kmx + 1ull;   // cnt(lo) >= cnt(kt) > K >= cnt(hi) = 0
        // bisection on the counts.  Any search keeping cnt(lo) > K >= cnt(hi)
        // ends at the same tau, and a threshold with a count of K exactly
        // selects the same K keys.
        while (hi - lo > 1) {
          const uint64_t mid = (lo + hi) >> 1;
          const int c2 = cnt_ge((unsigned)mid);
          if (c2 <= K) hi = mid;
          else lo = mid;
          if (c2 == K) break;
        }
        tau = (unsigned)hi;
      }
      unsigned ko = 0u;
      int ns = 0;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        if (64 * u < C4) {   // uniform
          bool in[4];
          uint64_t mm[4];
          int before = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            in[c] = k[u][c] >= tau;
            if (!in[c]) ko = k[u][c] > ko ? k[u][c] : ko;
            mm[c] = __ballot(in[c]);
            before += __builtin_popcountll(mm[c] & ltm);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (in[c]) {
              top[ns + before] = make_uint2(unkey(k[u][c]), (unsigned)(lb4 + (256 * u + c) - (256 * u + c > bl4 ? 1 : 0)));
              ++before;
            }
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) ns += __builtin_popcountll(mm[c]);
        }
      }
      h.ns = ns;
      ko = (unsigned)uni((int)~wave_min_dpp(~ko));   // the wave's largest
      h.xout = ko == 0u ? NI : __uint_as_float(unkey(ko));
    }
    if (lane == 0) *(RowHdr<float>*)pr = h;
    rbad[r] = h.bad;
    rxmax[r] = h.xmax;
  }
  if constexpr (FUSE) {
    // the exp terms in place of the keys: for a row without NaN / +inf the
    // maximum is order-free, a key is 0 for the blank and the padding only
    // (the blank's value is xbv), and -inf gives exp 0
    auto unkey = [](unsigned kv) { return kv ^ ((kv >> 31) ? 0x80000000u : 0xFFFFFFFFu); };
    bool sum_row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      sum_row[r] = live[r] && !rbad[r];   // wave-uniform
      if (lane == 0) {
        rmax[r * 4 + wv] = rxmax[r];
        rsum[r * 4 + wv] = sum_row[r] ? 1 : 0;
      }
    }
    float* const tiles = (float*)&cks_all[0][0];   // [2][NR][kNormTileW]
    const int bl4 = blank - 4 * lane;
    __syncthreads();   // etab, rmax and rsum are visible
    float s = 0.f;
    // the terms of tile u of row r, in place of its keys
    // (a finite maximum: no term is NaN, expf_t_le0 serves; an all -inf row:
    // every term NaN, as the reference's)
    auto terms = [&](const int r, const int u) __attribute__((always_inline)) {
      const bool inrow = 64 * u + lane < C4;
      const bool fin = rxmax[r] > -__builtin_inff();   // wave-uniform
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = (256 * u + c == bl4) ? xbv[r] : __uint_as_float(unkey(kr[r][u][c]));
        const float e = fin ? gm::expf_t_le0(v - rxmax[r], etab) : gm::expf_t_nonpos(v - rxmax[r], etab);
        kr[r][u][c] = __float_as_uint(inrow ? e : 0.f);
      }
    };
    // row lane's 256 terms of one tile in class order (zeros past the row add
    // nothing), the reads one batch ahead of the adds
    auto chain = [&](const float* tr0) __attribute__((always_inline)) {
      const float4* tr = (const float4*)tr0;
      float4 a[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[0][i] = tr[i];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (q + 1 < 16) {
#pragma unroll
          for (int i = 0; i < 4; ++i) a[(q + 1) & 1][i] = tr[4 * (q + 1) + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s += a[q & 1][i].x;
          s += a[q & 1][i].y;
          s += a[q & 1][i].z;
          s += a[q & 1][i].w;
        }
      }
    };
    // one step per tile (u a compile-time index: the rows stay in registers; a
    // plain loop is not fully unrolled at NV >= 24 and put kr on the stack)
    auto step = [&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      if (64 * u >= C4) return;   // block-uniform
      float* const tb = tiles + (u & 1) * NR * kNormTileW;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (sum_row[r]) {
          terms(r, u);
          *(float4*)(tb + (r * 4 + wv) * kNormTileW + 4 * lane) =
              make_float4(__uint_as_float(kr[r][u][0]), __uint_as_float(kr[r][u][1]), __uint_as_float(kr[r][u][2]),
                          __uint_as_float(kr[r][u][3]));
        }
      }
      __syncthreads();   // tile u written; tile u - 1's buffer free again
      if (wv == 0 && lane < NR) chain(tb + lane * kNormTileW);
    };
    unroll_seq(step, std::make_integer_sequence<int, NV>{});
    // (rows with NaN / +inf leave theirs to their own wave, below)
    if (wv == 0 && lane < NR && rsum[lane]) norm[(int64_t)blockIdx.x * NR + lane] = rmax[lane] + gm::logf(s);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (live[r] && rbad[r] && lane == 0) {
        // the reference's order for both: maxCoeff's loop, then the sum
        const int64_t row = rrow[r], t = row / B, b = row - t * B;
        const E* xr1 = x + (t * xst_t + b * xst_b);
        float m = ldw<float>(xr1, 0);
        for (int j = 1; j < C; ++j) {
          const float v = ldw<float>(xr1, j);
          m = (v > m) ? v : m;
        }
        float s1 = 0.f;
        for (int j = 0; j < C; ++j) s1 += gm::expf_t(ldw<float>(xr1, j) - m, etab);
        norm[row] = m + gm::logf(s1);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Backward walks over the records.  which = 0: decoded labels (LabelSeq,
// ctc_beam_entry.h:123-136); which = 1: best alignment (AlignmentLabelSeq +
// the candidate chain, ctc_beam_entry.h:137-152, 190-228).  Output reversed.
__global__ __launch_bounds__(256) void ctcx_traceback(TraceParams tp) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = tp.B * tp.P * 2;
  if (tid >= nthreads) return;
  const int which = (int)(tid & 1);
  const int64_t bp = tid >> 1;
  const int64_t b = bp / tp.P;
  const int p = (int)(bp - b * tp.P);
  const int sl = tp.seq_len[b] > 0 ? tp.seq_len[b] : 0;
  int32_t* out = tp.seq + (bp * 2 + which) * tp.Tmax;
  int len = 0;
  int k = tp.top_pos[bp];
  if (sl > 0 && k >= 0 && p < tp.item[b].n_leaves) {
    // record (t, k) unpacked: link, label, the two alignment back-pointers.
    // With the record ring, frame t's first record is foff[t]: independent of
    // the chain, so it is read one step ahead (fo), and each step waits on one
    // load, not two (cfg3 2.17 -> 1.80 ms); without it the plain walk
    const int32_t* fof = tp.foff ? tp.foff + b * tp.Tmax : nullptr;
    auto walk = [&](auto ring) {
      constexpr bool RING = decltype(ring)::value;
      int fo = RING ? fof[sl - 1] : 0;
      auto rd = [&](int t, uint32_t& link, int& lab, uint32_t& bpb, uint32_t& bpn) {
        int64_t at;
        if constexpr (RING) {
          at = b * tp.Tmax * tp.W + fo + k;
          fo = t > 0 ? fof[t - 1] : 0;
        } else {
          at = (b * tp.Tmax + t) * tp.W + k;
        }
        if (tp.rec_fmt == kRecFmt128) {
          const Rec16 r = ((const Rec16*)tp.rec)[at];
          link = r.link; lab = r.label; bpb = r.bpb; bpn = r.bpn;
        } else if (tp.rec_fmt == kRecFmt32) {
          const Rec32 r = ((const Rec32*)tp.rec)[at];
          link = r & 255u; lab = (int)((r >> 8) & 63u); bpb = rec32_unbp9((r >> 14) & 511u);
          bpn = rec32_unbp9(r >> 23);
        } else {
          const Rec r = tp.rec[at];
          link = rec_link(r); lab = rec_label(r); bpb = rec_bp_blank(r); bpn = rec_bp_nblank(r);
        }
      };
      if (which == 0) {
        int prev = -1;
        for (int t = sl - 1; t >= 0; --t) {
          uint32_t link, bpb, bpn;
          int lab;
          rd(t, link, lab, bpb, bpn);
          if (link & 1u) {
            if (!tp.merge || lab != prev) out[len++] = lab;
            prev = lab;
          }
          k = (int)(link >> 1);
        }
      } else {
        int kind = tp.top_kind[bp];
        for (int t = sl - 1; t >= 0 && kind >= 0; --t) {
          uint32_t link, bpb, bpn;
          int lab;
          rd(t, link, lab, bpb, bpn);
          out[len++] = kind == 0 ? tp.blank_label : lab;
          const uint32_t q = kind == 0 ? bpb : bpn;
          if (q >= kBpRestart) break;
          k = (int)(q >> 1);
          kind = (int)(q & 1u);
        }
      }
    };
    if (fof) walk(std::true_type{});
    else walk(std::false_type{});
  }
  tp.len[((int64_t)p * 2 + which) * tp.len_stride + b] = len;
}

// The same walks, one 256-thread block per item (2P <= 256 walkers), through
// LDS copies of the item's records: every walker of an item is at the same
// frame at every step (each step goes one frame back), so the records of G
// frames at a time -- one contiguous range of the item's stream, the ring's
// compacted frames or [t][W] -- are copied in with 16-byte loads and the
// walkers step through LDS, where ctcx_traceback waits out one dependent
// global load per frame (~1.1 us at cfg3: 1.74 ms for 1500 frames).  Two
// buffers: the next segment's loads are in flight, in registers, while the
// walkers step through the current one.
// (static LDS stays within the 64 KB a plain launch gets without an
// attribute: two 24-KB buffers and the offsets, 56 KB; a first 72-KB version
// was cut to this while its real fault, the ring's frame order, was found)
constexpr int kTbBufBytes = 24 * 1024;           // one segment buffer
constexpr int kTbLoads = kTbBufBytes / 16 / 256;  // 16-byte loads per thread per segment
static_assert(kTbLoads * 16 * 256 == kTbBufBytes, "whole loads");
constexpr int kTbMaxG = 1024;                     // frames per segment at most (the offsets' buffer)
__device__ __forceinline__ void tb_rec(const uint32_t* w, int rb, uint32_t& link, int& lab, uint32_t& bpb,
                                       uint32_t& bpn) {   // one record from its first word in LDS
  if (rb == 16) {
    const uint4 r = *(const uint4*)w;
    link = r.x; lab = (int)r.y; bpb = r.z; bpn = r.w;
  } else if (rb == 4) {
    const uint32_t r = w[0];
    link = r & 255u; lab = (int)((r >> 8) & 63u); bpb = rec32_unbp9((r >> 14) & 511u); bpn = rec32_unbp9(r >> 23);
  } else {
    const uint2 u = *(const uint2*)w;
    const Rec r = (Rec)u.x | ((Rec)u.y << 32);
    link = rec_link(r); lab = rec_label(r); bpb = rec_bp_blank(r); bpn = rec_bp_nblank(r);
  }
}
__global__ __launch_bounds__(256) void ctcx_traceback_seg(TraceParams tp) {
  __shared__ __attribute__((aligned(16))) uint32_t buf[2][kTbBufBytes / 4];
  __shared__ int32_t fbuf[2][kTbMaxG];   // (ring) the segment's frame offsets
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int rb = tp.rec_fmt == kRecFmt128 ? 16 : tp.rec_fmt == kRecFmt32 ? 4 : 8;
  const int rw = rb >> 2;   // words per record
  const int W = tp.W;
  const int sl = tp.seq_len[b] > 0 ? tp.seq_len[b] : 0;
  const int32_t* fof = tp.foff ? tp.foff + b * tp.Tmax : nullptr;
  // frames per segment: G frames of at most W records, plus the 16-byte
  // alignment slack, fit one buffer
  const int G = (kTbBufBytes - 16) / (W * rb) < kTbMaxG ? (kTbBufBytes - 16) / (W * rb) : kTbMaxG;
  const uint32_t* recw = (const uint32_t*)tp.rec;
  const int64_t item_w = b * tp.Tmax * (int64_t)W * rw;   // the item's first word (16-byte aligned: tp.rec is)
  // walkers
  const bool walker = tid < 2 * tp.P;
  const int which = tid & 1;
  const int p = tid >> 1;
  const int64_t bp = b * tp.P + p;
  int32_t* const out = tp.seq + (bp * 2 + which) * tp.Tmax;
  int len = 0, k = -1, kind = 0, prev = -1;
  bool act = false;
  if (walker) {
    k = tp.top_pos[bp];
    act = sl > 0 && k >= 0 && p < tp.item[b].n_leaves;
    if (which == 1) {
      kind = tp.top_kind[bp];
      act = act && kind >= 0;
    }
  }
  // the segment below frame hi: frames [lo, hi] and words [a0, a1) of the
  // stream (absolute, a0 aligned down to 16 bytes).  [t][W]: G frames.  The
  // record ring: each flush appends its frames newest first (ring_flush), so
  // a flush's frames lie in one block at offsets that grow as t falls, and
  // the block of the flush before starts lower; a segment is the frames of
  // one block (of up to 256 and G frames) -- thread j tests frame hi - j
  __shared__ int seg_len;
  auto seg = [&](int hi_, int& lo, int& hi, int64_t& a0, int64_t& a1) {
    hi = hi_;
    int64_t w0, w1;
    if (fof) {
      if (tid == 0) seg_len = 256 < G ? 256 : G;
      __syncthreads();
      const int t = hi - tid;
      const int fh = fof[hi];
      bool stop = t < 0;
      if (!stop && tid > 0)
        stop = fof[t] < fof[t + 1] || ((int64_t)fof[t] + W - fh) * rb > kTbBufBytes - 16;
      if (stop && tid < 256) __hip_atomic_fetch_min(&seg_len, tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __syncthreads();
      lo = hi - seg_len + 1;
      __syncthreads();   // (seg_len read by every thread before the next segment's reset)
      w0 = (int64_t)fh * rw;
      w1 = ((int64_t)fof[lo] + W) * rw;   // (a frame holds at most W records)
    } else {
      lo = hi - G + 1 > 0 ? hi - G + 1 : 0;
      w0 = (int64_t)lo * W * rw;
      w1 = (int64_t)(hi + 1) * W * rw;
    }
    a0 = (item_w + w0) & ~(int64_t)3;
    a1 = item_w + w1;
  };
  uint4 ld[kTbLoads];
  auto load = [&](int64_t a0, int64_t a1) {   // into registers; the last piece word by word (never past a1)
#pragma unroll
    for (int q = 0; q < kTbLoads; ++q) {
      const int64_t w = a0 + 4 * ((int64_t)q * 256 + tid);
      if (w + 4 <= a1) {
        ld[q] = *(const uint4*)(recw + w);
      } else if (w < a1) {
        ld[q].x = recw[w];
        ld[q].y = w + 1 < a1 ? recw[w + 1] : 0u;
        ld[q].z = w + 2 < a1 ? recw[w + 2] : 0u;
        ld[q].w = 0u;
      }
    }
  };
  auto store = [&](int bi, int64_t a0, int64_t a1, int lo, int hi) {
#pragma unroll
    for (int q = 0; q < kTbLoads; ++q) {
      const int64_t w = a0 + 4 * ((int64_t)q * 256 + tid);
      if (w < a1) *(uint4*)&buf[bi][4 * (q * 256 + tid)] = ld[q];
    }
    if (fof)
      for (int f = lo + tid; f <= hi; f += 256) fbuf[bi][f - lo] = fof[f];
  };
  int lo = 0, hi = -1, lo1 = 0, hi1 = 0;
  int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  if (sl > 0) {
    seg(sl - 1, lo, hi, a0, a1);
    load(a0, a1);
    store(0, a0, a1, lo, hi);
    __syncthreads();
  }
  for (int s = 0; hi >= 0; ++s) {   // (block-uniform: sl is the item's)
    const int bi = s & 1;
    const bool more = lo > 0;
    if (more) {   // the next segment's loads in flight during this one's walk
      seg(lo - 1, lo1, hi1, b0, b1);
      load(b0, b1);
    }
    if (act) {
      for (int t = hi; t >= lo; --t) {
        const int64_t wr = item_w + (fof ? (int64_t)fbuf[bi][t - lo] * rw : (int64_t)t * W * rw) + (int64_t)k * rw;
        uint32_t link, bpb, bpn;
        int lab;
        tb_rec(&buf[bi][wr - a0], rb, link, lab, bpb, bpn);
        if (which == 0) {
          if (link & 1u) {
            if (!tp.merge || lab != prev) out[len++] = lab;
            prev = lab;
          }
          k = (int)(link >> 1);
        } else {
          out[len++] = kind == 0 ? tp.blank_label : lab;
          const uint32_t q = kind == 0 ? bpb : bpn;
          if (q >= kBpRestart) { act = false; break; }
          k = (int)(q >> 1);
          kind = (int)(q & 1u);
        }
      }
    }
    if (more) store(bi ^ 1, b0, b1, lo1, hi1);
    __syncthreads();   // the next buffer written; this one free for the segment after
    if (!more) break;
    lo = lo1; hi = hi1; a0 = b0; a1 = b1;
  }
  if (walker) tp.len[((int64_t)p * 2 + which) * tp.len_stride + b] = len;
}

// Exclusive scan of lengths per (path, kind); also totals and maxima.
// One 256-thread block per (path, kind).  res[(p*2+w)*2 + 0] = total, +1 = max.
__global__ __launch_bounds__(256) void ctcx_scan(const int32_t* len, int64_t* off, int64_t* res, int64_t B) {
  __shared__ int64_t s_sum[256];
  __shared__ int64_t s_max[256];
  const int64_t pw = blockIdx.x;
  const int32_t* l = len + pw * B;
  int64_t* o = off + pw * B;
  int64_t carry = 0, mx = 0;
  for (int64_t base = 0; base < B; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = (i < B) ? l[i] : 0;
    s_sum[threadIdx.x] = v;
    s_max[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t a = (threadIdx.x >= (unsigned)d) ? s_sum[threadIdx.x - d] : 0;
      const int64_t m2 = (threadIdx.x >= (unsigned)d) ? s_max[threadIdx.x - d] : 0;
      __syncthreads();
      s_sum[threadIdx.x] += a;
      s_max[threadIdx.x] = s_max[threadIdx.x] > m2 ? s_max[threadIdx.x] : m2;
      __syncthreads();
    }
    if (i < B) o[i] = carry + s_sum[threadIdx.x] - v;
    carry += s_sum[255];
    mx = mx > s_max[255] ? mx : s_max[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) { res[pw * 2] = carry; res[pw * 2 + 1] = mx; }
}

// SparseTensor components (kernels.cc:225-254): one block per (item, path, kind).
__global__ __launch_bounds__(64) void ctcx_pack(PackParams pp) {
  const int64_t g = blockIdx.x;                 // ((b * P) + p) * 2 + w
  const int w = (int)(g & 1);
  const int64_t bpp = g >> 1;
  const int64_t b = bpp / pp.P;
  const int p = (int)(bpp - b * pp.P);
  const int64_t lidx = ((int64_t)p * 2 + w) * pp.B + b;
  const int n = pp.len[lidx];
  const int64_t o = pp.off[lidx];
  const int32_t* s = pp.seq + (bpp * 2 + w) * pp.Tmax;
  int64_t* idx = pp.idx[p * 2 + w];
  int64_t* val = pp.val[p * 2 + w];
  for (int i = threadIdx.x; i < n; i += 64) {
    idx[(o + i) * 2] = b;
    idx[(o + i) * 2 + 1] = i;
    val[o + i] = s[n - 1 - i];
  }
}

// ---- the dense, enqueue-only path (ctcext_decode_dense): everything the
// synchronous call decides on the host from data, decided here instead

// check_table_t's rule on the device table: *bad becomes nonzero if an entry
// is > 0 or NaN (the host's memset node zeroes it before the launch).
template <typename T>
__global__ __launch_bounds__(256) void ctcx_dense_table_scan(const T* tab, int64_t n, int32_t* bad) {
  int any = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    any |= !(tab[i] <= T(0)) ? 1 : 0;
  if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(bad, 1);
}

// check_lengths on the device: the lengths the kernels read (a length above
// Tmax, and every length under a bad table, is 0; a negative one stays, the
// kernels read it as 0) and the status bits known before the decode.
__global__ __launch_bounds__(256) void ctcx_dense_prologue(DensePrologueParams pp) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= pp.B) return;
  const int32_t v = pp.seq_len[b];
  int32_t st = 0;
  if (pp.table_bad && *pp.table_bad) st |= kItemTable;
  if (v > pp.Tmax) st |= kItemLength;
  pp.sl[b] = st ? 0 : v;
  pp.pre[b] = st;
}

// The padded outputs: one block per (item, path, kind) row of Tmax int64.
// Element i is the traceback's reversed walk read backwards below the row's
// length and pad_value from there on.  A row starts on an 8-byte boundary
// (odd Tmax, or an output view): the element before the first 16-byte
// boundary and the one after the last pair are written alone, the pairs
// between them as 16-byte stores.  An item with any status bit is empty.
__global__ __launch_bounds__(256) void ctcx_pack_dense(PackDenseParams pp) {
  typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
  const int64_t g = blockIdx.x;                 // ((b * P) + p) * 2 + w
  const int w = (int)(g & 1);
  const int64_t bpp = g >> 1;
  const int64_t b = bpp / pp.P;
  const int p = (int)(bpp - b * pp.P);
  const int64_t T_ = pp.Tmax;
  int32_t st = pp.pre[b];
  if ((pp.item[b].pad & kItemDeadMask) != 0) st |= kItemHelperTimeout;
  if (!(st & (kItemLength | kItemTable)) && pp.item[b].n_leaves < pp.P) st |= kItemFewLeaves;
  int64_t n = st ? 0 : pp.len[((int64_t)p * 2 + w) * pp.B + b];
  n = n < 0 ? 0 : n > T_ ? T_ : n;
  const int32_t* s = pp.seq + g * T_;
  int64_t* out = (w ? pp.alignment : pp.decoded) + bpp * T_;
  const int64_t pad = pp.pad_value;
  auto at = [&](int64_t i) -> int64_t { return i < n ? (int64_t)s[n - 1 - i] : pad; };
  const int64_t head = (int64_t)(((uintptr_t)out >> 3) & 1) < T_ ? (int64_t)(((uintptr_t)out >> 3) & 1) : T_;
  const int64_t pairs = (T_ - head) >> 1;
  for (int64_t q = threadIdx.x; q < pairs; q += 256) {
    const int64_t i = head + 2 * q;
    i64x2 v;
    v.x = at(i);
    v.y = at(i + 1);
    *(i64x2*)(out + i) = v;
  }
  if (threadIdx.x == 0) {
    if (head) out[0] = at(0);
    const int64_t tail = head + 2 * pairs;
    if (tail < T_) out[tail] = at(tail);
    (w ? pp.alignment_length : pp.decoded_length)[bpp] = (int32_t)n;
    if (w == 0) {
      if (pp.f64) ((double*)pp.out_log_prob)[bpp] = st ? -__builtin_inf() : ((const double*)pp.log_prob)[bpp];
      else ((float*)pp.out_log_prob)[bpp] = st ? -__builtin_inff() : ((const float*)pp.log_prob)[bpp];
      if (p == 0) {
        pp.status[b] = st;
        pp.status_ws[b] = st;
      }
    }
  }
}

#endif  // CTCX_PART == 0 (the non-template kernels)

}  // namespace ctcx

// ---------------------------------------------------------------------------
// Launchers (called by the C-ABI layer).
namespace ctcx {

template <typename T, int RN, int WC, bool BIG, class SC, bool HW = false, bool SQ = false>
hipError_t launch_decode_c(const DecodeParams<T>& p, hipStream_t s) {
  // the decode layout, then (HW) the score table or gather queue, then the
  // record ring (its size by the same functions as the host's checks)
  size_t lds = decode_lds_bytes(WC > 0 ? WC : p.W, p.C, (int)sizeof(T), SC::kStateful);
  if (HW)
    lds = ((lds + 15) & ~(size_t)15) + ((BIG || SQ) ? gq_lds_bytes(SQ, SQ ? sq_slots(WC) : kQSlots) : tab_lds_bytes()) +
          ((SQ && !BIG) ? sq_rowpf_bytes(p.C) + sq_stage_bytes(WC, p.C) : 0);
  if (p.ring > 0) lds = ((lds + 15) & ~(size_t)15) + ring_lds_bytes(p.ring, p.W, HW && !BIG ? 4 : 8);
  if (lds > kLdsBytes) return hipErrorInvalidValue;
#ifdef CTCX_STREAM
  // the image is this allocation: the host asks for its size at open (query),
  // and a push must bring exactly that (a stream runs one kernel for its life)
  if (p.st.query) {
    *p.st.query = (int64_t)lds;
    ctcx_launch_note()[0] = ctcx_decode_kernel_id(false, (int)sizeof(T), SC::kStateful, RN, WC, BIG, HW, SQ) | kStreamKernelBit;
    return hipSuccess;
  }
  if (p.ring != 0 || p.st.image_bytes != (int64_t)lds) return hipErrorInvalidValue;
#endif
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)ctcx_beam_decode<T, RN, WC, BIG, SC, HW, SQ>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((ctcx_beam_decode<T, RN, WC, BIG, SC, HW, SQ>), dim3((unsigned)p.B), dim3(HW ? 128 : 64), lds,
                     s, p);
  ctcx_launch_note()[0] = ctcx_decode_kernel_id(false, (int)sizeof(T), SC::kStateful, RN, WC, BIG, HW, SQ);
#ifdef CTCX_STREAM
  ctcx_launch_note()[0] |= kStreamKernelBit;
#endif
  return hipGetLastError();
}

// The decode kernel's instantiations are split over several compilations of
// this file (CTCX_PART, csrc/Makefile), so the build runs them in parallel:
// part 0 holds everything else and the dispatcher; parts 1..6 one group of
// kernel instantiations each.
#define CTCX_DECODE_INSTANCES(X)                                                              \
  X(1, float, 1, 128, false, BaseBeamScorer<float>) X(1, float, 1, 0, false, BaseBeamScorer<float>) \
  X(1, float, 2, 256, false, BaseBeamScorer<float>) X(1, float, 2, 0, false, BaseBeamScorer<float>) \
  X(1, float, 4, 0, false, BaseBeamScorer<float>)                                             \
  X(2, float, 1, 128, true, BaseBeamScorer<float>) X(2, float, 1, 0, true, BaseBeamScorer<float>)   \
  X(3, float, 2, 256, true, BaseBeamScorer<float>) X(3, float, 2, 0, true, BaseBeamScorer<float>)   \
  X(3, float, 4, 0, true, BaseBeamScorer<float>)                                              \
  X(4, double, 1, 128, false, BaseBeamScorer<double>) X(4, double, 1, 0, false, BaseBeamScorer<double>) \
  X(4, double, 2, 256, false, BaseBeamScorer<double>) X(4, double, 2, 0, false, BaseBeamScorer<double>) \
  X(4, double, 4, 0, false, BaseBeamScorer<double>)                                           \
  X(5, double, 1, 128, true, BaseBeamScorer<double>) X(5, double, 1, 0, true, BaseBeamScorer<double>) \
  X(5, double, 2, 256, true, BaseBeamScorer<double>) X(5, double, 2, 0, true, BaseBeamScorer<double>) \
  X(5, double, 4, 0, true, BaseBeamScorer<double>)                                            \
  X(6, float, 1, 128, false, BigramBeamScorer<float>) X(6, float, 1, 0, false, BigramBeamScorer<float>) \
  X(6, float, 2, 256, false, BigramBeamScorer<float>) X(6, float, 2, 0, false, BigramBeamScorer<float>) \
  X(6, float, 4, 0, false, BigramBeamScorer<float>)                                           \
  X(6, float, 1, 128, true, BigramBeamScorer<float>) X(6, float, 1, 0, true, BigramBeamScorer<float>) \
  X(6, float, 2, 256, true, BigramBeamScorer<float>) X(6, float, 2, 0, true, BigramBeamScorer<float>) \
  X(6, float, 4, 0, true, BigramBeamScorer<float>)                                            \
  X(7, double, 1, 128, false, BigramBeamScorer<double>) X(7, double, 1, 0, false, BigramBeamScorer<double>) \
  X(7, double, 2, 256, false, BigramBeamScorer<double>) X(7, double, 2, 0, false, BigramBeamScorer<double>) \
  X(7, double, 4, 0, false, BigramBeamScorer<double>)                                         \
  X(7, double, 1, 128, true, BigramBeamScorer<double>) X(7, double, 1, 0, true, BigramBeamScorer<double>) \
  X(7, double, 2, 256, true, BigramBeamScorer<double>) X(7, double, 2, 0, true, BigramBeamScorer<double>) \
  X(7, double, 4, 0, true, BigramBeamScorer<double>)

#ifndef CTCX_PART
#define CTCX_PART 0
#endif
#define CTCX_IF_1(...)
#define CTCX_IF_2(...)
#define CTCX_IF_3(...)
#define CTCX_IF_4(...)
#define CTCX_IF_5(...)
#define CTCX_IF_6(...)
#define CTCX_IF_7(...)
#define CTCX_IF_8(...)
#define CTCX_IF_10(...)
#define CTCX_IF_11(...)
#define CTCX_IF_12(...)
#define CTCX_IF_13(...)
#if CTCX_PART == 1
#undef CTCX_IF_1
#define CTCX_IF_1(...) __VA_ARGS__
#elif CTCX_PART == 2
#undef CTCX_IF_2
#define CTCX_IF_2(...) __VA_ARGS__
#elif CTCX_PART == 3
#undef CTCX_IF_3
#define CTCX_IF_3(...) __VA_ARGS__
#elif CTCX_PART == 4
#undef CTCX_IF_4
#define CTCX_IF_4(...) __VA_ARGS__
#elif CTCX_PART == 5
#undef CTCX_IF_5
#define CTCX_IF_5(...) __VA_ARGS__
#elif CTCX_PART == 6
#undef CTCX_IF_6
#define CTCX_IF_6(...) __VA_ARGS__
#elif CTCX_PART == 7
#undef CTCX_IF_7
#define CTCX_IF_7(...) __VA_ARGS__
#elif CTCX_PART == 8
#undef CTCX_IF_8
#define CTCX_IF_8(...) __VA_ARGS__
#elif CTCX_PART == 10
#undef CTCX_IF_10
#define CTCX_IF_10(...) __VA_ARGS__
#elif CTCX_PART == 11
#undef CTCX_IF_11
#define CTCX_IF_11(...) __VA_ARGS__
#elif CTCX_PART == 12
#undef CTCX_IF_12
#define CTCX_IF_12(...) __VA_ARGS__
#elif CTCX_PART == 13
#undef CTCX_IF_13
#define CTCX_IF_13(...) __VA_ARGS__
#endif
#define CTCX_IF_PART(P, ...) CTCX_IF_##P(__VA_ARGS__)
#if CTCX_PART == 0
#define CTCX_X(P, T, RN, WC, BIG, SC) \
  extern template hipError_t launch_decode_c<T, RN, WC, BIG, SC>(const DecodeParams<T>&, hipStream_t);
#else
#define CTCX_X(P, T, RN, WC, BIG, SC) \
  CTCX_IF_PART(P, template hipError_t launch_decode_c<T, RN, WC, BIG, SC>(const DecodeParams<T>&, hipStream_t);)
#endif
CTCX_DECODE_INSTANCES(CTCX_X)
#undef CTCX_X
// the two-wave (helper) kernels: the cfg2/cfg3 class (part 8), large C (part 10)
#if CTCX_PART == 0
extern template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);
#else
CTCX_IF_PART(8, template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true>(
                    const DecodeParams<float>&, hipStream_t);)
CTCX_IF_PART(10, template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true>(
                     const DecodeParams<float>&, hipStream_t);)
CTCX_IF_PART(10, template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true>(
                     const DecodeParams<float>&, hipStream_t);)
// the scored gather queue (beams <= 128): small C (part 11), large C (part 12)
CTCX_IF_PART(11, template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true, true>(
                     const DecodeParams<float>&, hipStream_t);)
CTCX_IF_PART(12, template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true, true>(
                     const DecodeParams<float>&, hipStream_t);)
// ... and for beams of 129..256 at large C, one slot (part 13)
CTCX_IF_PART(13, template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true, true>(
                     const DecodeParams<float>&, hipStream_t);)
#endif

#if CTCX_PART == 0
// BIG (C > 64): the grow loop's branch/window skipping by row-block maxima is
// compiled in; small-C builds keep the leaner loop (its register allocation is
// what cfg3 runs on)
template <typename T, int RN, int WC, class SC = BaseBeamScorer<T>>
static hipError_t launch_decode_r(const DecodeParams<T>& p, hipStream_t s) {
  return p.C > 64 ? launch_decode_c<T, RN, WC, true, SC>(p, s) : launch_decode_c<T, RN, WC, false, SC>(p, s);
}

// The two-wave kernel a shape can run (helper_kind; 0: none): 1 the score
// table (float, beams <= 128, C <= 64; 4-byte records), 2 the gather queue
// (float, beams <= 256, C > 64), 3 the scored gather queue (float, beams <=
// 128, any C; 4-byte records for C <= 64).  The base scorer only.  mode (the
// host's, once per call in enqueue_shard): kHelperNone (CTCEXT_HELPER=0, or
// the one-wave re-decode after a helper timeout), kHelperLegacy (kinds 1 and
// 2 only), kHelperScored (kind 3 where it applies).
template <typename T>
int helper_kind(const DecodeParams<T>& p, int mode) {
  // (C == 1: no label offers; the one-wave kernel's literal path, ctcext_capi)
  if (mode == kHelperNone || sizeof(T) != 4 || p.scorer_tab != nullptr || p.C < 2) return 0;
  if ((mode == kHelperScored || mode == kHelperScoredWide) && p.C <= kSqMaxClasses &&
      (p.W <= 128 || (mode == kHelperScoredWide && p.W <= 256 && p.C > 64)))
    return 3;
  if (p.C <= kRec32MaxClasses) return p.W <= kRec32MaxBeam ? 1 : 0;
  return p.W <= 256 ? 2 : 0;
}
__host__ inline int helper_wc(int W) { return W <= 128 ? 128 : 256; }
// LDS bytes before the record ring: the decode layout and the helper's table
// or gather queue
template <typename T>
size_t pre_ring_lds_bytes(const DecodeParams<T>& p, int hk, int wc) {
  const size_t b = (decode_lds_bytes(wc, p.C, (int)sizeof(T), p.scorer_tab != nullptr) + 15) & ~(size_t)15;
  return hk == 1   ? b + tab_lds_bytes()
         : hk == 2 ? b + gq_lds_bytes(false)
         : hk == 3 ? b + gq_lds_bytes(true, sq_slots(wc)) + (p.C <= 64 ? sq_rowpf_bytes(p.C) + sq_stage_bytes(wc, p.C) : 0)
                   : b;
}
// the two-wave kernel this call runs (0: none), given the kind the host chose
// (hk): its layout and ring must fit
template <typename T>
int use_helper_kernel(const DecodeParams<T>& p, int hk) {
  if (hk == 0) return 0;
  size_t b = pre_ring_lds_bytes(p, hk, helper_wc(p.W));
  if (p.ring > 0) b = ((b + 15) & ~(size_t)15) + ring_lds_bytes(p.ring, p.W, helper_rec32(hk, p.C) ? 4 : 8);
  return b <= kLdsBytes ? hk : 0;
}
template int use_helper_kernel<float>(const DecodeParams<float>&, int);
template int use_helper_kernel<double>(const DecodeParams<double>&, int);
template int helper_kind<float>(const DecodeParams<float>&, int);
template int helper_kind<double>(const DecodeParams<double>&, int);

template <typename T>
hipError_t launch_decode(const DecodeParams<T>& p, hipStream_t s) {
  if (p.B == 0) return hipSuccess;
  // RN registers per lane hold the min-child of the (W + 1) / 2 internal heap
  // nodes; the compile-time layouts (WC) are used whenever they fit the LDS
  if (p.scorer_tab) {   // the bigram scorer: the same compile-time layouts (with its state arrays)
    using SC = BigramBeamScorer<T>;
    auto fits_s = [&](int wc) { return decode_lds_bytes(wc, p.C, (int)sizeof(T), true) <= kLdsBytes; };
    if (p.W <= 128) return fits_s(128) ? launch_decode_r<T, 1, 128, SC>(p, s) : launch_decode_r<T, 1, 0, SC>(p, s);
    if (p.W <= 256) return fits_s(256) ? launch_decode_r<T, 2, 256, SC>(p, s) : launch_decode_r<T, 2, 0, SC>(p, s);
    return launch_decode_r<T, 4, 0, SC>(p, s);
  }
  auto fits = [&](int wc) { return decode_lds_bytes(wc, p.C, (int)sizeof(T), false) <= kLdsBytes; };
  if constexpr (sizeof(T) == 4) {
    // p.helper: the host's one decision (use_helper_kernel), checked again here
    const int hk = p.helper;
    if (hk != 0 && use_helper_kernel(p, hk) != hk) return hipErrorInvalidValue;
    if (hk == 1) return launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true>(p, s);
    if (hk == 2)
      return p.W <= 128 ? launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true>(p, s)
                        : launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true>(p, s);
    if (hk == 3)
      return p.C <= 64   ? launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true, true>(p, s)
             : p.W <= 128 ? launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true, true>(p, s)
                          : launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true, true>(p, s);
  }
  if (p.W <= 128) return fits(128) ? launch_decode_r<T, 1, 128>(p, s) : launch_decode_r<T, 1, 0>(p, s);
  if (p.W <= 256) return fits(256) ? launch_decode_r<T, 2, 256>(p, s) : launch_decode_r<T, 2, 0>(p, s);
  return launch_decode_r<T, 4, 0>(p, s);
}

template hipError_t launch_decode<float>(const DecodeParams<float>&, hipStream_t);
template hipError_t launch_decode<double>(const DecodeParams<double>&, hipStream_t);

// Frames of the record ring for launch_decode's choice of kernel (0: none):
// the largest power of two in [8, cap] whose ring fits beside the decode
// layout: within the CU's LDS when the batch has at most one item per CU (or
// the layout alone already takes more than half a CU), else within 80 KB, so
// two items still share a CU.  The stream offsets (foff) are int32.
template <typename T>
int ring_frames(const DecodeParams<T>& p, int cus, int cap, int hk) {
  const bool scored = p.scorer_tab != nullptr;
  auto fits = [&](int wc) { return decode_lds_bytes(wc, p.C, (int)sizeof(T), scored) <= kLdsBytes; };
  const int wcap = (p.W <= 128 && fits(128)) ? 128 : (p.W > 128 && p.W <= 256 && fits(256)) ? 256 : p.W;
  if ((int64_t)p.Tmax * p.W > 0x7fffffffLL) return 0;
  // the two-wave kernel the host chose (hk), when its layout and a ring fit
  // (the score table's records are 4 bytes)
  if (hk && pre_ring_lds_bytes(p, hk, helper_wc(p.W)) + ring_lds_bytes(8, p.W, helper_rec32(hk, p.C) ? 4 : 8) >
                kLdsBytes)
    hk = 0;
  const int rb = helper_rec32(hk, p.C) ? 4 : 8;
  const size_t base = pre_ring_lds_bytes(p, hk, hk ? helper_wc(p.W) : wcap);
  const size_t budget = (base > 80 * 1024 || p.B <= cus) ? kLdsBytes : 80 * 1024;
  // the kernel addresses ring rows by t & (R - 1): R must be a power of two
  if (cap < 8) return 0;
  cap = 1 << (31 - __builtin_clz((unsigned)cap));
  for (int r = cap; r >= 8; r >>= 1) {
    // ring_flush's stamps are fp * 4096 + (step + 1), fp the flush count
    // (<= Tmax / (R / 2) + 1): they must stay below INT32_MAX
    if (((int64_t)p.Tmax / (r / 2) + 2) * 4096 > 0x7fffffffLL) continue;
    if (base + ring_lds_bytes(r, p.W, rb) <= budget) return r;
  }
  return 0;
}
template int ring_frames<float>(const DecodeParams<float>&, int, int, int);
template int ring_frames<double>(const DecodeParams<double>&, int, int, int);

template <int NV, typename E>
static hipError_t launch_row_facts(const E* x, const int32_t* sl, char* prep, float* norm, int64_t rows, int64_t B,
                                   int C, int64_t xst_t, int64_t xst_b, int blank, bool& fuse, hipStream_t s) {
  // the normaliser fused for rows of up to 1024 classes only: past them the
  // block's class-order chain (C dependent adds per four rows) costs more than
  // the second read it saves (cfg5: 19.4 ms fused, 8.5 + 8.7 split)
  if constexpr (kFuseNorm<NV>) {
    if (fuse) {
      constexpr int nr = 4 * facts_rows_per_wave<NV, true>();
      hipLaunchKernelGGL((ctcx_row_facts<NV, true, E>), dim3((unsigned)((rows + nr - 1) / nr)), dim3(256), 0, s, x,
                         sl, prep, rows, B, C, xst_t, xst_b, blank, norm);
      ctcx_launch_note()[1] = kPrepFactsFused;
      return hipGetLastError();
    }
  }
  fuse = false;
  constexpr int nr = 4 * facts_rows_per_wave<NV, false>();
  hipLaunchKernelGGL((ctcx_row_facts<NV, false, E>), dim3((unsigned)((rows + nr - 1) / nr)), dim3(256), 0, s, x, sl,
                     prep, rows, B, C, xst_t, xst_b, blank, (float*)nullptr);
  return hipGetLastError();
}

// CTCEXT_NORM_V4=0: ctcx_row_norm instead of ctcx_row_norm_v4 (A/B runs)
static bool norm_v4() {
  static const bool v = [] {
    const char* e = getenv("CTCEXT_NORM_V4");
    return !(e != nullptr && e[0] == '0');
  }();
  return v;
}

// CTCEXT_PREP_SPLIT=1: the facts and ctcx_row_norm as two kernels (two reads
// of the logits), the round-4 form, for A/B runs
static bool prep_split() {
  static const bool v = [] {
    const char* e = getenv("CTCEXT_PREP_SPLIT");
    return e != nullptr && e[0] == '1';
  }();
  return v;
}

// The pre-pass over rows of E in memory (T itself, or F16 / BF16 with T =
// float), row (t, b) at x + t * xst_t + b * xst_b.
template <typename T, typename E>
static hipError_t launch_row_prep_e(const E* x, const int32_t* sl, char* prep, T* norm, int64_t T_, int64_t B,
                                    int64_t C, int64_t xst_t, int64_t xst_b, int blank, hipStream_t s) {
  const int64_t rows = T_ * B;
  if (rows == 0 || C <= 64) return hipSuccess;
  if constexpr (sizeof(T) == 4) {
    // float rows of whole four-class pieces, every row start aligned to a
    // piece (16 bytes of float, 8 of a half format: the base and both
    // strides): the register-resident row facts, with the normaliser from the
    // same registers (one read) where that pays, else followed by ctcx_row_norm
    const bool pieces = C % 4 == 0 && ((uintptr_t)x & (4 * sizeof(E) - 1)) == 0 && xst_t % 4 == 0 && xst_b % 4 == 0;
    if (pieces && C <= 256 * 32) {   // NV <= 32 pieces per lane
      const int c4 = (int)(C / 4);
      bool fuse = !prep_split();   // (cleared by the launcher where it does not fuse)
      float* nf = (float*)norm;
      hipError_t e;
#define CTCX_FACTS(NV) launch_row_facts<NV, E>(x, sl, prep, nf, rows, B, (int)C, xst_t, xst_b, blank, fuse, s)
      if (c4 <= 64) e = CTCX_FACTS(1);
      else if (c4 <= 128) e = CTCX_FACTS(2);
      else if (c4 <= 256) e = CTCX_FACTS(4);
      else if (c4 <= 512) e = CTCX_FACTS(8);
      else if (c4 <= 768) e = CTCX_FACTS(12);
      else if (c4 <= 1024) e = CTCX_FACTS(16);
      else if (c4 <= 1280) e = CTCX_FACTS(20);
      else if (c4 <= 1536) e = CTCX_FACTS(24);
      else e = CTCX_FACTS(32);
#undef CTCX_FACTS
      if (e != hipSuccess || fuse) return e;
      ctcx_launch_note()[1] = kPrepFactsNorm;
      if (norm_v4())
        hipLaunchKernelGGL(ctcx_row_norm_v4<E>, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, x, sl, nf, T_, B,
                           C, xst_t, xst_b, (const char*)prep);
      else
        hipLaunchKernelGGL((ctcx_row_norm<T, E>), dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, x, sl, norm,
                           T_, B, C, xst_t, xst_b, (const char*)prep);
      return hipGetLastError();
    }
  }
  const size_t row_b = (size_t)C * sizeof(T);   // (staged widened)
  // the expf table, the row, then the compact key list
  const size_t lds = kPrepTabBytes + ((row_b + 15) & ~(size_t)15) + 4 * kPrepCompact;
  if (row_b > kPrepLdsBytes) {   // the row is read from global memory
    hipLaunchKernelGGL((ctcx_row_prep<T, false, E>), dim3((unsigned)rows), dim3(64),
                       kPrepTabBytes + 4 * kPrepCompact, s, x, sl, prep, norm, B, C, xst_t, xst_b, blank);
    ctcx_launch_note()[1] = kPrepRowGlobal;
    return hipGetLastError();
  }
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)ctcx_row_prep<T, true, E>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((ctcx_row_prep<T, true, E>), dim3((unsigned)rows), dim3(64), lds, s, x, sl, prep, norm, B, C,
                     xst_t, xst_b, blank);
  ctcx_launch_note()[1] = kPrepRowLds;
  return hipGetLastError();
}

// x holds elements of xfmt (kInNative: of T; the half formats with T = float only)
template <typename T>
hipError_t launch_row_prep(const void* x, int xfmt, const int32_t* sl, char* prep, T* norm, int64_t T_, int64_t B,
                           int64_t C, int64_t xst_t, int64_t xst_b, int blank, hipStream_t s) {
  if constexpr (sizeof(T) == 4) {
    if (xfmt == kInF16)
      return launch_row_prep_e<T, F16>((const F16*)x, sl, prep, norm, T_, B, C, xst_t, xst_b, blank, s);
    if (xfmt == kInBF16)
      return launch_row_prep_e<T, BF16>((const BF16*)x, sl, prep, norm, T_, B, C, xst_t, xst_b, blank, s);
  }
  if (xfmt != kInNative) return hipErrorInvalidValue;
  return launch_row_prep_e<T, T>((const T*)x, sl, prep, norm, T_, B, C, xst_t, xst_b, blank, s);
}
template hipError_t launch_row_prep<float>(const void*, int, const int32_t*, char*, float*, int64_t, int64_t, int64_t,
                                           int64_t, int64_t, int, hipStream_t);
template hipError_t launch_row_prep<double>(const void*, int, const int32_t*, char*, double*, int64_t, int64_t,
                                            int64_t, int64_t, int64_t, int, hipStream_t);

template <typename T>
hipError_t launch_row_norm(const void* x, int xfmt, const int32_t* sl, T* norm, int64_t T_, int64_t B, int64_t C,
                           int64_t xst_t, int64_t xst_b, hipStream_t s) {
  const int64_t rows = T_ * B;
  if (rows == 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + 63) / 64));
  if (sizeof(T) == 4 && xfmt == kInF16) {
    if constexpr (sizeof(T) == 4)
      hipLaunchKernelGGL((ctcx_row_norm<T, F16>), grid, dim3(64), 0, s, (const F16*)x, sl, norm, T_, B, C, xst_t,
                         xst_b, (const char*)nullptr);
  } else if (sizeof(T) == 4 && xfmt == kInBF16) {
    if constexpr (sizeof(T) == 4)
      hipLaunchKernelGGL((ctcx_row_norm<T, BF16>), grid, dim3(64), 0, s, (const BF16*)x, sl, norm, T_, B, C, xst_t,
                         xst_b, (const char*)nullptr);
  } else if (xfmt != kInNative) {
    return hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((ctcx_row_norm<T, T>), grid, dim3(64), 0, s, (const T*)x, sl, norm, T_, B, C, xst_t, xst_b,
                       (const char*)nullptr);
  }
  ctcx_launch_note()[1] = kPrepNormOnly;
  return hipGetLastError();
}
template hipError_t launch_row_norm<float>(const void*, int, const int32_t*, float*, int64_t, int64_t, int64_t,
                                           int64_t, int64_t, hipStream_t);
template hipError_t launch_row_norm<double>(const void*, int, const int32_t*, double*, int64_t, int64_t, int64_t,
                                            int64_t, int64_t, hipStream_t);

// Half-precision rows (t, b) at x + t * xst_t + b * xst_b, widened into the
// dense float tensor out[T_][B][C]: the global-state tier reads its rows in
// place, as floats, so the host widens a half shard into workspace first.
template <typename E>
__global__ __launch_bounds__(256) void ctcx_widen_rows(const E* __restrict__ x, float* __restrict__ out, int64_t B,
                                                      int64_t C, int64_t xst_t, int64_t xst_b) {
  const int64_t row = blockIdx.x;
  const int64_t t = row / B, b = row - t * B;
  const E* xr = x + (t * xst_t + b * xst_b);
  float* o = out + row * C;
  for (int64_t j = threadIdx.x; j < C; j += 256) o[j] = ldw<float>(xr, j);
}
hipError_t launch_widen_rows(const void* x, int xfmt, float* out, int64_t T_, int64_t B, int64_t C, int64_t xst_t,
                             int64_t xst_b, hipStream_t s) {
  const int64_t rows = T_ * B;
  if (rows == 0 || C == 0) return hipSuccess;
  if (rows > 0x7fffffffLL) return hipErrorInvalidValue;
  if (xfmt == kInF16)
    hipLaunchKernelGGL(ctcx_widen_rows<F16>, dim3((unsigned)rows), dim3(256), 0, s, (const F16*)x, out, B, C, xst_t,
                       xst_b);
  else if (xfmt == kInBF16)
    hipLaunchKernelGGL(ctcx_widen_rows<BF16>, dim3((unsigned)rows), dim3(256), 0, s, (const BF16*)x, out, B, C,
                       xst_t, xst_b);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_traceback(const TraceParams& tp, hipStream_t s) {
  const int64_t n = tp.B * tp.P * 2;
  if (n == 0) return hipSuccess;
  // the segmented walk (ctcx_traceback_seg) when an item's walkers fit one
  // block and a segment holds at least one frame; CTCEXT_TRACEBACK=0
  // (diagnostics) the one-thread-per-walk kernel
  const int rb = tp.rec_fmt == kRecFmt128 ? 16 : tp.rec_fmt == kRecFmt32 ? 4 : 8;
  const char* ev = getenv("CTCEXT_TRACEBACK");
  if (2 * (int64_t)tp.P <= 256 && (int64_t)tp.W * rb <= kTbBufBytes - 16 && !(ev && ev[0] == '0')) {
    hipLaunchKernelGGL(ctcx_traceback_seg, dim3((unsigned)tp.B), dim3(256), 0, s, tp);
    ctcx_launch_note()[2] = kTbSegmented;
    return hipGetLastError();
  }
  hipLaunchKernelGGL(ctcx_traceback, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tp);
  ctcx_launch_note()[2] = kTbOneThread;
  return hipGetLastError();
}

hipError_t launch_scan(const int32_t* len, int64_t* off, int64_t* res, int64_t B, int P, hipStream_t s) {
  hipLaunchKernelGGL(ctcx_scan, dim3((unsigned)(P * 2)), dim3(256), 0, s, len, off, res, B);
  return hipGetLastError();
}

hipError_t launch_pack(const PackParams& pp, hipStream_t s) {
  const int64_t n = pp.B * pp.P * 2;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(ctcx_pack, dim3((unsigned)n), dim3(64), 0, s, pp);
  return hipGetLastError();
}

// The dense path's prologue: with a bigram table (table_n entries of float,
// or double with f64) its scan into *bad first, then the lengths.
hipError_t launch_dense_prologue(DensePrologueParams pp, const void* table, int64_t table_n, int f64, int32_t* bad,
                                 hipStream_t s) {
  if (pp.B == 0) return hipSuccess;
  if (pp.B > 0x7fffffffLL) return hipErrorInvalidValue;
  pp.table_bad = nullptr;
  if (table && table_n > 0) {
    hipError_t e = hipMemsetAsync(bad, 0, 4, s);
    if (e != hipSuccess) return e;
    const int64_t blocks = (table_n + 255) / 256 < 1024 ? (table_n + 255) / 256 : 1024;
    if (f64)
      hipLaunchKernelGGL(ctcx_dense_table_scan<double>, dim3((unsigned)blocks), dim3(256), 0, s, (const double*)table,
                         table_n, bad);
    else
      hipLaunchKernelGGL(ctcx_dense_table_scan<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)table,
                         table_n, bad);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    pp.table_bad = bad;
  }
  hipLaunchKernelGGL(ctcx_dense_prologue, dim3((unsigned)((pp.B + 255) / 256)), dim3(256), 0, s, pp);
  return hipGetLastError();
}

hipError_t launch_pack_dense(const PackDenseParams& pp, hipStream_t s) {
  const int64_t n = pp.B * pp.P * 2;
  if (n == 0) return hipSuccess;
  if (n > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_pack_dense, dim3((unsigned)n), dim3(256), 0, s, pp);
  return hipGetLastError();
}
#endif  // CTCX_PART == 0

}  // namespace ctcx

#ifdef CTCX_GSTATE
// ---------------------------------------------------------------------------
// The global-state tier (this file compiled once more with CTCX_GSTATE, the
// generic address space for the state and namespace ctcx_gs; csrc/Makefile):
// shapes whose beam state or row does not fit the LDS (beam_width above the
// LDS-resident limit, num_classes above the 8-byte record's 65535 or the
// LDS row) decode with the state in global memory, 16-byte records and the
// literal path for every frame -- the reference's own algorithm, one lane.
namespace ctcx {
template <typename T, class SC>
static hipError_t launch_decode_gs_t(const DecodeParams<T>& p, hipStream_t s) {
  hipLaunchKernelGGL((ctcx_beam_decode<T, 1, 0, false, SC, false>), dim3((unsigned)p.B), dim3(64), 0, s, p);
  ctcx_launch_note()[0] = ctcx_decode_kernel_id(true, (int)sizeof(T), SC::kStateful, 1, 0, false, false, false);
#ifdef CTCX_STREAM
  ctcx_launch_note()[0] |= kStreamKernelBit;
#endif
  return hipGetLastError();
}
}  // namespace ctcx

#ifndef CTCX_STREAM
// Called by the C-ABI layer with its DecodeParams<T> (the same header, so the
// same layout, in namespace ctcx there).
hipError_t ctcx_gstate_launch_decode(const void* p, int is_f64, int scored, hipStream_t s) {
  if (is_f64) {
    const auto& q = *(const ctcx::DecodeParams<double>*)p;
    if (q.B == 0) return hipSuccess;
    return scored ? ctcx::launch_decode_gs_t<double, ctcx::BigramBeamScorer<double>>(q, s)
                  : ctcx::launch_decode_gs_t<double, ctcx::BaseBeamScorer<double>>(q, s);
  }
  const auto& q = *(const ctcx::DecodeParams<float>*)p;
  if (q.B == 0) return hipSuccess;
  return scored ? ctcx::launch_decode_gs_t<float, ctcx::BigramBeamScorer<float>>(q, s)
                : ctcx::launch_decode_gs_t<float, ctcx::BaseBeamScorer<float>>(q, s);
}
#endif  // !CTCX_STREAM
#endif

#ifdef CTCX_STREAM
// ---------------------------------------------------------------------------
// The stream builds (this file compiled once more per part with CTCX_STREAM,
// namespace ctcx_st, and once more as the global-state tier with both macros,
// namespace ctcx_gs_st; csrc/Makefile).  The C-ABI layer passes its
// DecodeParams<T> -- the default build's struct, which is this one without
// its last member -- and the stream's parameters beside it.
namespace ctcx {
template <typename T>
static DecodeParams<T> stream_params(const void* p, const CtcxStreamParams* sp) {
  static_assert(offsetof(DecodeParams<T>, st) + sizeof(CtcxStreamParams) == sizeof(DecodeParams<T>), "st is the last member");
  static_assert(offsetof(DecodeParams<T>, st) == kCtcxDecodeParamsBytes, "the host layer's DecodeParams<T> ends where st begins");
  DecodeParams<T> q{};
  memcpy((void*)&q, p, offsetof(DecodeParams<T>, st));
  q.st = *sp;
  return q;
}
}  // namespace ctcx

#ifdef CTCX_GSTATE
hipError_t ctcx_gstate_stream_launch_decode(const void* p, const CtcxStreamParams* sp, int is_f64, int scored,
                                            hipStream_t s) {
  if (is_f64) {
    const auto q = ctcx::stream_params<double>(p, sp);
    if (q.B == 0) return hipSuccess;
    return scored ? ctcx::launch_decode_gs_t<double, ctcx::BigramBeamScorer<double>>(q, s)
                  : ctcx::launch_decode_gs_t<double, ctcx::BaseBeamScorer<double>>(q, s);
  }
  const auto q = ctcx::stream_params<float>(p, sp);
  if (q.B == 0) return hipSuccess;
  return scored ? ctcx::launch_decode_gs_t<float, ctcx::BigramBeamScorer<float>>(q, s)
                : ctcx::launch_decode_gs_t<float, ctcx::BaseBeamScorer<float>>(q, s);
}
#elif CTCX_PART == 14
// Part 14 of the stream build: the dispatcher over the instantiations of
// parts 1..13 (launch_decode's choices, with the two-wave kernel as the host
// decided it in p.helper at open).
namespace ctcx {
#define CTCX_X(P, T, RN, WC, BIG, SC) \
  extern template hipError_t launch_decode_c<T, RN, WC, BIG, SC>(const DecodeParams<T>&, hipStream_t);
CTCX_DECODE_INSTANCES(CTCX_X)
#undef CTCX_X
extern template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, false, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 1, 128, true, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);
extern template hipError_t launch_decode_c<float, 2, 256, true, BaseBeamScorer<float>, true, true>(
    const DecodeParams<float>&, hipStream_t);

template <typename T, int RN, int WC, class SC>
static hipError_t stream_decode_r(const DecodeParams<T>& p, hipStream_t s) {
  return p.C > 64 ? launch_decode_c<T, RN, WC, true, SC>(p, s) : launch_decode_c<T, RN, WC, false, SC>(p, s);
}
template <typename T, class SC>
static hipError_t stream_decode_w(const DecodeParams<T>& p, hipStream_t s) {
  auto fits = [&](int wc) { return decode_lds_bytes(wc, p.C, (int)sizeof(T), SC::kStateful) <= kLdsBytes; };
  if (p.W <= 128) return fits(128) ? stream_decode_r<T, 1, 128, SC>(p, s) : stream_decode_r<T, 1, 0, SC>(p, s);
  if (p.W <= 256) return fits(256) ? stream_decode_r<T, 2, 256, SC>(p, s) : stream_decode_r<T, 2, 0, SC>(p, s);
  return stream_decode_r<T, 4, 0, SC>(p, s);
}
template <typename T>
static hipError_t stream_decode(const DecodeParams<T>& p, hipStream_t s) {
  if (p.B == 0 && !p.st.query) return hipSuccess;
  if (p.scorer_tab) return stream_decode_w<T, BigramBeamScorer<T>>(p, s);
  if constexpr (sizeof(T) == 4) {
    const int hk = p.helper;
    using SC = BaseBeamScorer<float>;
    if (hk == 1) return launch_decode_c<float, 1, 128, false, SC, true>(p, s);
    if (hk == 2)
      return p.W <= 128 ? launch_decode_c<float, 1, 128, true, SC, true>(p, s)
                        : launch_decode_c<float, 2, 256, true, SC, true>(p, s);
    if (hk == 3)
      return p.C <= 64   ? launch_decode_c<float, 1, 128, false, SC, true, true>(p, s)
             : p.W <= 128 ? launch_decode_c<float, 1, 128, true, SC, true, true>(p, s)
                          : launch_decode_c<float, 2, 256, true, SC, true, true>(p, s);
  }
  return stream_decode_w<T, BaseBeamScorer<T>>(p, s);
}
}  // namespace ctcx

hipError_t ctcx_stream_launch_decode(const void* p, const CtcxStreamParams* sp, int is_f64, hipStream_t s) {
  if (is_f64) return ctcx::stream_decode<double>(ctcx::stream_params<double>(p, sp), s);
  return ctcx::stream_decode<float>(ctcx::stream_params<float>(p, sp), s);
}
#endif
#endif  // CTCX_STREAM
