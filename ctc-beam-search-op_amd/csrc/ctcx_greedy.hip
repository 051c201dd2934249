// ctcx_greedy.hip — the greedy (best-path) decode (include/ctcext.h, "Greedy
// decode"): per frame the class of the largest logit, collapsed over time.  A
// translation unit of its own: the decode objects neither see nor depend on it.
// It fills the buffers the decode's follow-up kernels read -- the normaliser,
// the reversed walks and their lengths, the status words -- so that token
// times, token scores, path scores and path alignments run after it unchanged.
//
// Kernel 1 (ctcx_greedy_frames<T, Fmt>): norm, k and lp of every (t, b) row.
// The normaliser's work split: a wave owns 64 consecutive rows, the workgroup
// is that wave.  The rows reach the lanes through an LDS tile of 64 rows by 32
// classes, padded to 33 words so that the lanes' row reads are conflict-free.
// A 64-lane load covers two tile rows of 32 contiguous classes; the 32 loads of
// the next tile are issued before this tile's arithmetic.  One lane then walks
// one row in class order, twice: the max pass (which here also carries the
// index of the maximum, strictly greater wins, so the lowest index of a tie
// stays and a leading NaN stays) and the sum pass over exp(x_j - max) with the
// glibc replicas.  A row of up to 32 classes stays in LDS between the two
// passes and is read from memory once; wider rows are read once per pass.  The
// arithmetic is the decoder's normaliser's, operation for operation, so norm is
// its normaliser bit for bit; lp = max - norm is one more rounded subtraction.
//
// Kernel 2 (ctcx_greedy_collapse<T>): one workgroup of five waves per item,
// frames in ascending tiles of 256.  Waves 0..3 compact: a frame is a
// candidate when its k is no blank and differs from the frame before; a
// candidate is kept unless merge_repeated and its label equals the previous
// candidate's.  Within a wave the previous candidate is the highest set bit of
// the candidate ballot below the lane, and its k comes by a cross-lane fetch;
// across waves the last candidate's label goes through LDS, across tiles in a
// register every thread keeps.  A kept label's position is the prefix popcount
// of the keep ballot plus the earlier waves' counts plus the earlier tiles'.
// The reversed decoded walk needs the item's total before its first write:
// the item is swept twice over its k row (count, then write), so no output
// element is written twice and nothing is staged.  Wave 4 adds up the item's lp
// values in frame order during the count sweep: it loads a tile's 256 values
// four per lane (the next tile's before it adds this one's) and feeds them to
// the chain by lane reads, one rounded add per frame.
//
// Nothing is trusted: lengths are clamped to [0, Tmax], every read of k and lp
// is of a frame below the item's length, and every position is below the total
// the count sweep found over the same data.  Every uniform value goes out
// through a lane's vector store.
#include "ctcx_greedy.h"

#include "glibc_math.h"
#include "glibc_math_f64.h"

namespace {

namespace gm = ctcx::gm;

constexpr int kTile = kGreedyTile;
constexpr int kRPL = 64 / kTile;    // tile rows per load instruction
constexpr int kNL = 64 / kRPL;      // load instructions per tile
static_assert(kRPL == 2 && kGreedyRows == 64, "a 64-lane load covers two tile rows");

// element idx of x, widened as the decode kernels widen it (fp16: the hardware
// convert; bf16: the bits, 16 to the left)
template <typename T, int Fmt>
__device__ __forceinline__ T elem(const void* x, int64_t idx) {
  if constexpr (Fmt == kGreedyInF16)
    return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)x)[idx]);
  else if constexpr (Fmt == kGreedyInBF16)
    return (T)__uint_as_float((unsigned)((const uint16_t*)x)[idx] << 16);
  else
    return ((const T*)x)[idx];
}

__device__ __forceinline__ float row_log(float s) { return gm::logf(s); }
__device__ __forceinline__ double row_log(double s) { return gm::log(s); }

template <typename T, int Fmt>
__global__ __launch_bounds__(64) void ctcx_greedy_frames(CtcxGreedyParams p) {
  __shared__ T tile[kGreedyRows][kTile + 1];   // [row in wave][class in tile]
  __shared__ uint64_t etab[32];                // expf's 2^(i/32) table: the lanes' indices diverge
  const int lane = threadIdx.x;
  const int64_t B = p.B, C = p.C;
  const int64_t rows = p.Tmax * B;
  const int64_t row = (int64_t)blockIdx.x * kGreedyRows + lane;
  if (lane < 32) etab[lane] = gm::exp2f_tab(lane);   // read after the first tile's barrier
  bool valid = false;
  int64_t off = 0;   // this lane's row, in elements of x
  if (row < rows) {
    const int64_t t = row / B, b = row - t * B;
    valid = t < p.sl[b];
    if (valid) off = t * p.xst_t + b * p.xst_b;
  }
  if (__ballot(valid) == 0) return;   // a wave of skipped rows (the workgroup is this wave)
  const int sub = lane / kTile, col = lane % kTile;   // a load's tile row (of two) and class
  auto row_base = [&](int rr) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, rr);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)off >> 32), rr);
    return (int64_t)(((uint64_t)hi << 32) | lo);
  };
  // tile rows 2 q + sub, classes c0 + col: a skipped row reads x's first row
  // instead, a class past C the row's first, and neither is used
  auto load = [&](T (&v)[kNL], int64_t c0) {
    const int nc = (int)(C - c0 < kTile ? C - c0 : kTile);
    const int64_t cc = col < nc ? c0 + col : 0;
#pragma unroll
    for (int q = 0; q < kNL; ++q) {
      const int64_t b0 = row_base(2 * q), b1 = row_base(2 * q + 1);
      v[q] = elem<T, Fmt>(p.x, (sub ? b1 : b0) + cc);
    }
  };
  const bool resident = C <= kTile;   // the row stays in LDS between the passes
  T m = T(0), s = T(0);
  int32_t k = 0;
  T v[kNL];
  for (int pass = 0; pass < 2; ++pass) {
    const bool reload = pass == 0 || !resident;
    if (reload) load(v, 0);
    for (int64_t c0 = 0; c0 < C; c0 += kTile) {
      const int nc = (int)(C - c0 < kTile ? C - c0 : kTile);
      if (reload) {
        __syncthreads();   // the tile's readers are done
#pragma unroll
        for (int q = 0; q < kNL; ++q) tile[q * kRPL + sub][col] = v[q];
        __syncthreads();
        if (c0 + kTile < C) load(v, c0 + kTile);   // in flight during this tile's arithmetic
      }
      if (!valid) continue;
      if (pass == 0) {
        int j = 0;
        if (c0 == 0) { m = tile[lane][0]; j = 1; }
        for (; j < nc; ++j) {
          const T e = tile[lane][j];
          const bool up = e > m;   // false for a NaN on either side
          m = up ? e : m;
          k = up ? (int32_t)(c0 + j) : k;
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
  if (valid) {
    const T nm = m + row_log(s);
    ((T*)p.norm)[row] = nm;
    p.k[row] = k;
    ((T*)p.lp)[row] = m - nm;
  }
}

__device__ __forceinline__ float lane_value(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

template <typename T>
__global__ __launch_bounds__(kGreedyThreads) void ctcx_greedy_collapse(CtcxGreedyParams p) {
  // the label of each wave's last candidate of a tile (-1: the wave has none),
  // by tile parity: a tile's words are read while the next tile's are written
  __shared__ int32_t s_lab[2][4];
  __shared__ int32_t s_cnt[4];   // labels each wave keeps: of the tile (write sweep), of the item (after the count sweep)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool compacts = wave < 4;
  const int64_t b = blockIdx.x, B = p.B, Tmax = p.Tmax;
  const int32_t st = p.pre[b];
  int64_t n = st ? 0 : (int64_t)p.sl[b];
  n = n < 0 ? 0 : n > Tmax ? Tmax : n;
  const int ntiles = (int)((n + kGreedyFrames - 1) / kGreedyFrames);
  const int32_t* const krow = p.k + b;          // frame f at krow[f * B]
  const T* const lprow = (const T*)p.lp + b;
  int32_t* const walk0 = p.seq + (b * 2) * Tmax;
  int32_t* const walk1 = walk0 + Tmax;
  int64_t* const dec = p.decoded + b * Tmax;
  int64_t* const ali = p.alignment + b * Tmax;
  const uint64_t below_lane = (1ull << lane) - 1;

  // wave 4: four frames of a tile per lane, frame f0 + 64 q + lane in v[q]
  auto load_lp = [&](T (&v)[4], int64_t f0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t f = f0 + 64 * q + lane;
      v[q] = f < n ? lprow[f * B] : T(0);
    }
  };
  T acc = T(0), nxt[4] = {T(0), T(0), T(0), T(0)};
  if (!compacts && ntiles > 0) load_lp(nxt, 0);

  int total = 0, mine = 0;   // the item's kept labels (known after the count sweep); this wave's share
  for (int sweep = 0; sweep < 2; ++sweep) {
    const bool write = sweep == 1;
    int32_t carry_lab = -1;   // the label of the last candidate before the tile (-1: none yet; a k is never negative)
    int pos0 = 0;             // labels kept before the tile
    for (int ti = 0; ti < ntiles; ++ti) {
      const int64_t f = (int64_t)ti * kGreedyFrames + tid;
      const bool in = compacts && f < n;
      int32_t kk = -1;
      bool cand = false;
      uint64_t cb = 0;
      if (compacts) {
        kk = in ? krow[f * B] : -1;
        // the frame before: the lane below, and for lane 0 a read of its own
        // (the wave below publishes only its candidates' labels)
        int32_t kp = __shfl_up(kk, 1);
        if (lane == 0) kp = (in && f > 0) ? krow[(f - 1) * B] : -1;
        cand = in && kk != p.blank_index && kk != kp;
        cb = __ballot(cand);
        const int32_t last = __shfl(kk, cb ? 63 - __clzll((long long)cb) : 0);
        if (lane == 0) s_lab[ti & 1][wave] = cb ? last : -1;
      }
      __syncthreads();
      bool keep = false;
      int rank = 0;
      if (compacts) {
        int32_t in_lab = carry_lab;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int32_t l = s_lab[ti & 1][w];
          if (w < wave && l >= 0) in_lab = l;
          if (l >= 0) carry_lab = l;
        }
        // The definition sets prev_lab at every candidate, kept or dropped, so
        // the previous candidate's label is what it compares with.  That is
        // also the previous kept label: a candidate is dropped only when it
        // equals prev_lab, which by induction is the last kept label already.
        const uint64_t below = cb & below_lane;
        const int32_t from = __shfl(kk, below ? 63 - __clzll((long long)below) : lane);
        const int32_t prev_lab = below ? from : in_lab;
        keep = cand && !(p.merge && kk == prev_lab);
        const uint64_t kb = __ballot(keep);
        rank = __popcll(kb & below_lane);
        const int kept = __popcll(kb);
        if (write) {
          if (lane == 0) s_cnt[wave] = kept;
        } else {
          mine += kept;
        }
      }
      if (write) {
        __syncthreads();
        if (compacts) {
          int offset = pos0;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int c = s_cnt[w];
            if (w < wave) offset += c;
            pos0 += c;
          }
          if (in) {
            const int32_t a = kk == p.blank_index ? p.blank_label : kk;
            ali[f] = a;
            walk1[n - 1 - f] = a;
          }
          if (keep) {
            const int pos = offset + rank;   // < total: the count sweep saw the same k
            dec[pos] = kk;
            walk0[total - 1 - pos] = kk;
          }
        }
      } else if (!compacts) {
        // the frame-order sum: logp = lp[0], then one rounded add per frame
        T cur[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        if (ti + 1 < ntiles) load_lp(nxt, (int64_t)(ti + 1) * kGreedyFrames);
        const int64_t left = n - (int64_t)ti * kGreedyFrames;
        const int cnt = (int)(left < kGreedyFrames ? left : kGreedyFrames);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = cnt - 64 * q < 64 ? cnt - 64 * q : 64;
          if (m == 64 && (ti > 0 || q > 0)) {
            // 64 whole frames: constant lane reads, which do not wait on the chain, and no branch per add
#pragma unroll
            for (int l = 0; l < 64; ++l) acc = acc + lane_value(cur[q], l);
            continue;
          }
          int l = 0;
          if (ti == 0 && q == 0) {
            acc = lane_value(cur[0], 0);
            l = 1;
          }
          for (; l < m; ++l) acc = acc + lane_value(cur[q], l);
        }
      }
    }
    if (!write) {
      if (compacts && lane == 0) s_cnt[wave] = mine;
      __syncthreads();
      total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();   // (the write sweep reuses s_cnt)
    }
  }

  // padding, lengths, status: disjoint from what the write sweep stored
  const int64_t pad = p.pad_value;
  for (int64_t i = total + tid; i < Tmax; i += kGreedyThreads) dec[i] = pad;
  for (int64_t i = n + tid; i < Tmax; i += kGreedyThreads) ali[i] = pad;
  if (tid < kGreedyItemWords) p.item[b * kGreedyItemWords + tid] = 0;
  if (tid == 64) {
    p.decoded_length[b] = total;
    p.alignment_length[b] = (int32_t)n;
    p.len[b] = total;
    p.len[B + b] = (int32_t)n;
    p.top_kind[b] = 0;
    p.status[b] = st;
    p.status_ws[b] = st;
  }
  if (tid == 4 * 64) ((T*)p.log_probability)[b] = st ? (T)(-__builtin_inff()) : acc;
}

template <typename T>
hipError_t launch_frames(const CtcxGreedyParams& p, hipStream_t s) {
  const int64_t rows = p.Tmax * p.B;
  const dim3 grid((unsigned)((rows + kGreedyRows - 1) / kGreedyRows)), block(64);
  if (p.xfmt == kGreedyInNative) {
    hipLaunchKernelGGL((ctcx_greedy_frames<T, kGreedyInNative>), grid, block, 0, s, p);
  } else if constexpr (sizeof(T) == 4) {
    if (p.xfmt == kGreedyInF16) hipLaunchKernelGGL((ctcx_greedy_frames<T, kGreedyInF16>), grid, block, 0, s, p);
    else if (p.xfmt == kGreedyInBF16) hipLaunchKernelGGL((ctcx_greedy_frames<T, kGreedyInBF16>), grid, block, 0, s, p);
    else return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;   // half-precision rows are float32 compute
  }
  return hipGetLastError();
}

}  // namespace

hipError_t ctcx_launch_greedy_frames(const CtcxGreedyParams& p, hipStream_t s) {
  const int64_t rows = p.Tmax * p.B;
  if (rows <= 0 || p.C <= 0) return rows == 0 ? hipSuccess : hipErrorInvalidValue;
  if ((rows + kGreedyRows - 1) / kGreedyRows > 0x7fffffffLL) return hipErrorInvalidValue;
  return p.f64 ? launch_frames<double>(p, s) : launch_frames<float>(p, s);
}

hipError_t ctcx_launch_greedy_collapse(const CtcxGreedyParams& p, hipStream_t s) {
  if (p.B == 0) return hipSuccess;
  if (p.B < 0 || p.B > 0x7fffffffLL || p.Tmax <= 0 || p.Tmax > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.B), block(kGreedyThreads);
  if (p.f64) hipLaunchKernelGGL(ctcx_greedy_collapse<double>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(ctcx_greedy_collapse<float>, grid, block, 0, s, p);
  return hipGetLastError();
}
