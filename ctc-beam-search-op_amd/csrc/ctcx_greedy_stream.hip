// ctcx_greedy_stream.hip — the push of a greedy stream (include/ctcext.h,
// "Streaming: greedy"): one launch takes a chunk of frames per item and leaves
// every output of the greedy decode, its token times and its token scores as
// they are over all frames the item has taken since its last reset.  A
// translation unit of its own: it includes the libm replicas and no decode
// header.
//
// Work split: one workgroup per item, which owns the item for the whole push --
// the state, the decisions, the rows.  Nothing crosses a workgroup, so there is
// no second launch.  Under the lane-per-row evaluator the workgroup is one
// wave; under the wide-row evaluator it is eight, and wave 0 is that one wave.
//
// 1. Decide (every lane reads the item's 48 bytes of state and its length).
//    reset[b] pads the item's rows back up to their old lengths and clears the
//    state; a length above chunk_time or past max_frames sets the status bit,
//    and the item then takes no frame: state and rows stay.
// 2. Rows, 64 of the item's chunk frames per step, one per lane -- so the
//    frames of one item lie in adjacent lanes, in frame order.  They reach the
//    lanes through an LDS tile of 64 rows by 32 classes, padded to 33 words; a
//    64-lane load covers two tile rows of 32 contiguous classes, and the next
//    tile's 32 loads are issued before this tile's arithmetic.  A lane walks its
//    row in class order twice: the max pass with the index (strictly greater
//    wins, a leading NaN stays), the sum pass over exp(x_j - max) with the
//    glibc replicas; norm = max + log(sum), lp = max - norm.  This is
//    ctcx_greedy_frames' arithmetic operation for operation, hence its bits.
//    That is the lane-per-row evaluator.  The wide-row evaluator (rows of many
//    classes) gives the item eight waves, each a chunk row at a time: a lane takes
//    every 64th class, and the max pass becomes a reduction over (value,
//    index) -- a NaN cell never enters, the greater value wins, of two values
//    that compare equal the lower index (so a zero's sign is that index's),
//    and a NaN in class 0 wins outright with k = 0: what the serial pass
//    gives.  The exp terms of 64 consecutive classes are evaluated at once,
//    go through the wave's 64 LDS words, and every lane adds them from there
//    in class order: the same chain of rounded adds as the serial sum, so the
//    same bits.  Lane 0 leaves k and lp in LDS, and wave 0 picks them up, a
//    frame per lane, for the one collapse both evaluators share.
// 3. Collapse, on the lanes that hold the frames: a frame is a candidate when
//    its k is no blank and differs from the frame before (the lane below; for
//    lane 0 the carried prev_k); the previous candidate is the highest set bit
//    of the candidate ballot below the lane (else the carried prev_lab), and a
//    candidate is kept unless merge_repeated and it equals that label.  A kept
//    label's position is the decoded length plus the prefix popcount of the
//    keep ballot: the rows are forward, so it is known at once and each label,
//    alignment cell and start is written once.  Every non-blank frame belongs
//    to the token at (kept at or below it) - 1; the last such frame of a token
//    in the step writes the token's end and score cells, so a token that goes
//    on in a later step or push has them overwritten by a later frame.
// 4. The float chains -- log_probability and the open token's logp_sum /
//    logp_min -- are one rounded operation per frame in frame order: a uniform
//    loop reads lp lane by lane.  The chain of the open token runs on through
//    the blanks behind its last run and is stored only at the token's frames:
//    that is the "carry beside the committed value" a merged A-blank-A needs,
//    with the committed value being the cell itself.
//
// Nothing is trusted beyond the stream's own state: lengths are clamped, a
// frame is read only below the item's length of this push, and every position
// written is below frames + n <= max_frames.  Every uniform value goes out
// through a lane's vector store.
#include "ctcx_greedy_stream.h"

#include "glibc_math.h"
#include "glibc_math_f64.h"

namespace {

namespace gm = ctcx::gm;

constexpr int kTile = kGreedyStreamTile;
constexpr int kRPL = 64 / kTile;    // tile rows per load instruction
constexpr int kNL = 64 / kRPL;      // load instructions per tile
static_assert(kRPL == 2 && kGreedyStreamRows == 64, "a 64-lane load covers two tile rows");

// element idx of x, widened as the decode kernels widen it (fp16: the hardware
// convert; bf16: the bits, 16 to the left)
template <typename T, int Fmt>
__device__ __forceinline__ T elem(const void* x, int64_t idx) {
  if constexpr (Fmt == kGreedyStreamInF16)
    return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)x)[idx]);
  else if constexpr (Fmt == kGreedyStreamInBF16)
    return (T)__uint_as_float((unsigned)((const uint16_t*)x)[idx] << 16);
  else
    return ((const T*)x)[idx];
}

__device__ __forceinline__ float row_log(float s) { return gm::logf(s); }
__device__ __forceinline__ double row_log(double s) { return gm::log(s); }

__device__ __forceinline__ float lane_value(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

// a state word as the compute dtype and back (a float32 in the low half)
__device__ __forceinline__ void from_word(uint64_t w, float& v) { v = __uint_as_float((uint32_t)w); }
__device__ __forceinline__ void from_word(uint64_t w, double& v) { v = __longlong_as_double((long long)w); }
__device__ __forceinline__ uint64_t to_word(float v) { return (uint64_t)__float_as_uint(v); }
__device__ __forceinline__ uint64_t to_word(double v) { return (uint64_t)__double_as_longlong(v); }

__device__ __forceinline__ float row_term(float d, const uint64_t* etab) { return gm::expf_t_nonpos(d, etab); }
__device__ __forceinline__ double row_term(double d, const uint64_t*) { return gm::exp(d); }

// orders a wave's LDS writes before its own later reads (and the other way round) for the compiler; the
// hardware runs one wave's LDS operations in order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

constexpr int kWideWaves = kGreedyStreamWideWaves;
constexpr int32_t kNone = 0x7fffffff;   // the index of a lane that has seen no value yet

template <typename T, int Fmt, bool Wide>
__global__ __launch_bounds__(Wide ? 64 * kWideWaves : 64) void ctcx_greedy_push(CtcxGreedyStreamParams p) {
  // lane per row: [chunk row of the step][class in tile]; wide rows: [wave][term of the 64 classes]
  __shared__ T tile[Wide ? kWideWaves : kGreedyStreamRows][Wide ? 64 : kTile + 1];
  __shared__ uint64_t etab[32];                      // expf's 2^(i/32) table: the lanes' indices diverge
  __shared__ int32_t s_k[Wide ? kGreedyStreamRows : 1];   // wide rows: the step's k and lp, a frame per word
  __shared__ T s_lp[Wide ? kGreedyStreamRows : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // (wave 0 decides, collapses and stores)
  const int64_t b = blockIdx.x, C = p.C, F = p.max_frames;
  const bool times = (p.want & kGreedyStreamTimes) != 0, scores = (p.want & kGreedyStreamScores) != 0;
  if (threadIdx.x < 32) etab[lane] = gm::exp2f_tab(lane);   // read after the first barrier
  int64_t* const dec = p.decoded + b * F;
  int64_t* const ali = p.alignment + b * F;
  int32_t* const tstart = times ? p.start + b * F : nullptr;
  int32_t* const tend = times ? p.end + b * F : nullptr;
  T* const lsum = scores ? (T*)p.logp_sum + b * F : nullptr;
  T* const lmin = scores ? (T*)p.logp_min + b * F : nullptr;
  const uint64_t self = 1ull << lane, below_lane = self - 1;

  // 1. the item's state and what this push does with it
  CtcxGreedyStreamItem it = p.item[b];
  int32_t frames = __builtin_amdgcn_readfirstlane(it.frames);
  int32_t dec_len = __builtin_amdgcn_readfirstlane(it.dec_len);
  frames = frames < 0 ? 0 : frames > F ? (int32_t)F : frames;
  dec_len = dec_len < 0 ? 0 : dec_len > frames ? frames : dec_len;
  int32_t prev_k = __builtin_amdgcn_readfirstlane(it.prev_k1) - 1;
  int32_t prev_lab = __builtin_amdgcn_readfirstlane(it.prev_lab1) - 1;
  int32_t trailing = __builtin_amdgcn_readfirstlane(it.trailing);
  T logp, ch_sum, ch_min;
  from_word(it.logp, logp);
  from_word(it.ch_sum, ch_sum);
  from_word(it.ch_min, ch_min);
  if constexpr (Wide) __syncthreads();   // every wave has read the state wave 0 stores at the end; etab is there
  if (p.reset && p.reset[b] != 0) {
    // a new utterance: the rows go back to padding up to their old lengths
    if (wave == 0) {
      const int64_t pad = p.pad_value;
      const T nan = (T)__builtin_nanf("");
      for (int i = lane; i < dec_len; i += 64) {
        dec[i] = pad;
        if (times) { tstart[i] = -1; tend[i] = -1; }
        if (scores) { lsum[i] = nan; lmin[i] = nan; }
      }
      for (int i = lane; i < frames; i += 64) ali[i] = pad;
      __threadfence();   // (the appends below write the same cells from other lanes)
    }
    frames = dec_len = trailing = 0;
    prev_k = prev_lab = -1;
    logp = ch_sum = ch_min = T(0);
  }
  int64_t v = p.chunk_length ? (int64_t)p.chunk_length[b] : p.chunk_time;
  v = v < 0 ? 0 : v;
  int32_t st = 0;
  if (v > p.chunk_time) st |= kGreedyStreamItemLength;
  if ((int64_t)frames + v > F) st |= kGreedyStreamItemCapacity;
  const int n = __builtin_amdgcn_readfirstlane(st ? 0 : (int)v);   // <= chunk_time, and frames + n <= F
  if (st && threadIdx.x == 0) {
    CtcxGreedyStreamAcc a = p.acc[b];
    if ((st & kGreedyStreamItemLength) && !(a.status & kGreedyStreamItemLength)) a.len_chunk = p.chunk_time;
    if ((st & kGreedyStreamItemCapacity) && !(a.status & kGreedyStreamItemCapacity))
      a.cap_total = (int32_t)(frames + v < 0x7fffffffLL ? frames + v : 0x7fffffffLL);
    a.status |= st;
    p.acc[b] = a;
  }

  const int sub = lane / kTile, col = lane % kTile;   // a load's tile row (of two) and class
  const bool resident = C <= kTile;                   // the row stays in LDS between the passes
  for (int r0 = 0; r0 < n; r0 += kGreedyStreamRows) {
    // 2. norm, k and lp of chunk rows r0 .. r0 + cnt - 1, one per lane
    const int cnt = n - r0 < kGreedyStreamRows ? n - r0 : kGreedyStreamRows;
    const bool valid = lane < cnt;
    T lp = T(0);
    int32_t k = 0;
    if constexpr (Wide) {
      // 2. (wide rows) norm, k and lp of chunk row r0 + r on wave r mod 8, 64 classes at a time
      for (int r = wave; r < cnt; r += kWideWaves) {
        const int64_t base = (int64_t)(r0 + r) * p.xst_t + b * p.xst_b;
        T mv = T(0);
        int32_t mi = kNone;
#pragma unroll 4
        for (int64_t c = lane; c < C; c += 64) {
          const T e = elem<T, Fmt>(p.x, base + c);
          const bool take = e == e && (mi == kNone || e > mv);   // a NaN cell never enters; ties keep the lower index
          mv = take ? e : mv;
          mi = take ? (int32_t)c : mi;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const T ov = __shfl_xor(mv, d);
          const int32_t oi = __shfl_xor(mi, d);
          const bool take = oi != kNone && (mi == kNone || ov > mv || (ov == mv && oi < mi));
          mv = take ? ov : mv;
          mi = take ? oi : mi;
        }
        const T x0 = elem<T, Fmt>(p.x, base);
        const bool lead = x0 != x0 || mi == kNone;   // a NaN in class 0 stays, with k = 0
        const T m = lead ? x0 : mv;
        const int32_t kr = lead ? 0 : mi;
        T s = T(0);
        T e = lane < C ? row_term(elem<T, Fmt>(p.x, base + lane) - m, etab) : T(0);
        for (int64_t c0 = 0; c0 < C; c0 += 64) {
          const int nc = (int)(C - c0 < 64 ? C - c0 : 64);
          wave_sync();   // the last group's readers are done
          tile[wave][lane] = e;
          wave_sync();
          // the next group's terms: independent of this group's chain
          if (c0 + 64 < C) e = c0 + 64 + lane < C ? row_term(elem<T, Fmt>(p.x, base + c0 + 64 + lane) - m, etab) : T(0);
          if (nc == 64) {
            // (sixteen LDS words ahead of the chain)
#pragma unroll 1
            for (int l0 = 0; l0 < 64; l0 += 16) {
#pragma unroll
              for (int l = 0; l < 16; ++l) s += tile[wave][l0 + l];
            }
          } else {
            for (int l = 0; l < nc; ++l) s += tile[wave][l];
          }
        }
        if (lane == 0) {
          s_k[r] = kr;
          s_lp[r] = m - (m + row_log(s));
        }
      }
      __syncthreads();
      if (wave == 0 && valid) {
        k = s_k[lane];
        lp = s_lp[lane];
      }
    } else {
      // (a lane past the step's rows loads the step's first row instead, and uses nothing of it)
      const int64_t off = (int64_t)(r0 + (valid ? lane : 0)) * p.xst_t + b * p.xst_b;
      auto row_base = [&](int rr) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, rr);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)off >> 32), rr);
        return (int64_t)(((uint64_t)hi << 32) | lo);
      };
      // tile rows 2 q + sub, classes c0 + col: a class past C reads the row's first, which is not used
      auto load = [&](T (&w)[kNL], int64_t c0) {
        const int nc = (int)(C - c0 < kTile ? C - c0 : kTile);
        const int64_t cc = col < nc ? c0 + col : 0;
  #pragma unroll
        for (int q = 0; q < kNL; ++q) {
          const int64_t b0 = row_base(2 * q), b1 = row_base(2 * q + 1);
          w[q] = elem<T, Fmt>(p.x, (sub ? b1 : b0) + cc);
        }
      };
      T m = T(0), s = T(0);
      int32_t kr = 0;
      T w[kNL];
      for (int pass = 0; pass < 2; ++pass) {
        const bool reload = pass == 0 || !resident;
        if (reload) load(w, 0);
        for (int64_t c0 = 0; c0 < C; c0 += kTile) {
          const int nc = (int)(C - c0 < kTile ? C - c0 : kTile);
          if (reload) {
            __syncthreads();   // the tile's readers are done
  #pragma unroll
            for (int q = 0; q < kNL; ++q) tile[q * kRPL + sub][col] = w[q];
            __syncthreads();
            if (c0 + kTile < C) load(w, c0 + kTile);   // in flight during this tile's arithmetic
          }
          if (!valid) continue;
          if (pass == 0) {
            int j = 0;
            if (c0 == 0) { m = tile[lane][0]; j = 1; }
            for (; j < nc; ++j) {
              const T e = tile[lane][j];
              const bool up = e > m;   // false for a NaN on either side
              m = up ? e : m;
              kr = up ? (int32_t)(c0 + j) : kr;
            }
          } else if constexpr (sizeof(T) == 4) {
            if (nc == kTile) {
              // a whole tile: the exp terms are independent (16 in flight
              // together), only the sum is a chain, in class order
  #pragma unroll
              for (int j0 = 0; j0 < kTile; j0 += 16) {
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
            for (int j = 0; j < nc; ++j) s += gm::exp(tile[lane][j] - m);
          }
        }
      }
      lp = valid ? m - (m + row_log(s)) : T(0);
      k = kr;
    }

    if constexpr (Wide) {
      if (wave != 0) {   // (the other waves wait for wave 0 to have read the step's k and lp)
        if (r0 + kGreedyStreamRows < n) __syncthreads();
        continue;
      }
    }
    // 3. the collapse of these frames against what the item carries
    const int32_t blank = p.blank_index;
    const int32_t kk = valid ? k : -1;
    int32_t kp = __shfl_up(kk, 1);
    if (lane == 0) kp = prev_k;
    const bool nonblank = valid && kk != blank;
    const bool cand = nonblank && kk != kp;
    const uint64_t cb = __ballot(cand);
    // The definition sets prev_lab at every candidate, kept or dropped, so the
    // previous candidate's label is what a candidate compares with.
    const uint64_t cbelow = cb & below_lane;
    const int32_t from = __shfl(kk, cbelow ? 63 - __clzll((long long)cbelow) : lane);
    const bool keep = cand && !(p.merge && kk == (cbelow ? from : prev_lab));
    const uint64_t kb = __ballot(keep), nb = __ballot(nonblank);
    const int gf = frames + r0 + lane;                              // the frame on the item's time axis, < F
    const int tok = dec_len + __popcll(kb & (below_lane | self)) - 1;   // the token a non-blank frame belongs to
    // ... whose last frame of this step it is: no non-blank frame above, or the next one opens a token
    const uint64_t above = nb & ~(below_lane | self);
    const bool last = nonblank && tok >= 0 && (above == 0 || ((kb >> __builtin_ctzll(above)) & 1));
    if (valid) ali[gf] = kk == blank ? (int64_t)p.blank_label : (int64_t)kk;
    if (keep) {   // tok < dec_len + kept <= frames + n
      dec[tok] = kk;
      if (times) tstart[tok] = gf;
    }
    if (times && last) tend[tok] = gf;

    // 4. the chains, one rounded operation per frame in frame order
    T my_sum = T(0), my_min = T(0);
    int l = 0;
    if (frames + r0 == 0) {   // the first frame ever sets logp (lp, not 0 + lp); it opens a token or belongs to none
      logp = ch_sum = ch_min = lane_value(lp, 0);
      my_sum = ch_sum; my_min = ch_min;
      l = 1;
    }
    if (scores) {
      for (; l < cnt; ++l) {
        const T u = lane_value(lp, l);
        const bool opens = (kb >> l) & 1;
        logp = logp + u;
        ch_sum = opens ? u : ch_sum + u;
        ch_min = opens ? u : (u < ch_min ? u : ch_min);   // a NaN never replaces, a leading NaN stays
        if (lane == l) { my_sum = ch_sum; my_min = ch_min; }
      }
      if (last) { lsum[tok] = my_sum; lmin[tok] = my_min; }
    } else {
      for (; l < cnt; ++l) logp = logp + lane_value(lp, l);
    }

    // what the next step, or the next push, compares with
    prev_k = __builtin_amdgcn_readlane(kk, cnt - 1);
    if (cb) prev_lab = __builtin_amdgcn_readlane(kk, 63 - __clzll((long long)cb));
    dec_len += __popcll(kb);
    trailing = nb ? cnt - 1 - (63 - __clzll((long long)nb)) : trailing + cnt;
    if (r0 + kGreedyStreamRows < n) {
      __threadfence();   // (a token's end and score cells are written again below)
      if constexpr (Wide) __syncthreads();
    }
  }
  frames += n;

  if (threadIdx.x == 0) {
    it.frames = frames; it.dec_len = dec_len;
    it.prev_k1 = prev_k + 1; it.prev_lab1 = prev_lab + 1;
    it.trailing = trailing; it.pad = 0;
    it.logp = to_word(logp); it.ch_sum = to_word(ch_sum); it.ch_min = to_word(ch_min);
    p.item[b] = it;
    p.decoded_length[b] = dec_len;
    p.alignment_length[b] = frames;
    ((T*)p.log_probability)[b] = logp;
    p.status[b] = st;
    p.frames[b] = frames;
    if (times) p.trailing_blank[b] = trailing;
  }
}

template <typename T, bool Wide>
hipError_t launch_push(const CtcxGreedyStreamParams& p, hipStream_t s) {
  const dim3 grid((unsigned)p.B), block(Wide ? 64 * kWideWaves : 64);
  if (p.xfmt == kGreedyStreamInNative) {
    hipLaunchKernelGGL((ctcx_greedy_push<T, kGreedyStreamInNative, Wide>), grid, block, 0, s, p);
  } else if constexpr (sizeof(T) == 4) {
    if (p.xfmt == kGreedyStreamInF16) hipLaunchKernelGGL((ctcx_greedy_push<T, kGreedyStreamInF16, Wide>), grid, block, 0, s, p);
    else if (p.xfmt == kGreedyStreamInBF16) hipLaunchKernelGGL((ctcx_greedy_push<T, kGreedyStreamInBF16, Wide>), grid, block, 0, s, p);
    else return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;   // half-precision rows are float32 compute
  }
  return hipGetLastError();
}

}  // namespace

hipError_t ctcx_launch_greedy_push(const CtcxGreedyStreamParams& p, hipStream_t s) {
  if (p.B == 0) return hipSuccess;
  if (p.B < 0 || p.B > 0x7fffffffLL || p.C <= 0 || p.chunk_time < 0 || p.max_frames < 0 || p.max_frames > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (p.wide) return p.f64 ? launch_push<double, true>(p, s) : launch_push<float, true>(p, s);
  return p.f64 ? launch_push<double, false>(p, s) : launch_push<float, false>(p, s);
}
