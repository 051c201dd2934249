// ctcx_align.hip — the Viterbi alignment of every returned path
// (include/ctcext.h, "Path alignments"): the single most likely CTC alignment of
// the decoded row y over all of the item's frames, from the row the traceback
// leaves in the workspace (walk 0), the decoder's normaliser and the logits
// where the decode read them.  A translation unit of its own: the decode
// objects neither see nor depend on it.
//
// Three launches: the forward trellis, which keeps a decision per state and
// frame; the walk back through those decisions; the emit, which un-reverses the
// walk into the padded output.  The unchanged token-times and token-scores
// kernels then run over the walk buffer the second one writes.
//
// Forward (ctcx_path_align_reg<T, Fmt, K>): the path scores' work split, because
// the data movement is the same problem.  One wave64 per (item, path) row, the
// workgroup is that wave, no barrier in the time loop.  The m labels are dealt
// to the lanes in contiguous blocks of K: lane l holds labels [l K, l K + K),
// and for each the pair (blank state 2j, label state 2j + 1) in registers.  The
// lane of the last label holds the final blank: slot m of its own block where
// the block has room, the register vF where label m - 1 is its block's last.  A
// row runs in the smallest instantiation with 64 K >= m, every instantiation is
// launched over all rows, and foreign rows return at once.  One DPP wave_shr:1
// a frame brings the previous lane's last label state; frame f + 1's gathers are
// issued before frame f's arithmetic.
//
// What happens to a state is the definition, literally: two compares, two
// selects and one add, in the compute dtype, nothing contracted, no
// renormalisation.  A lane packs its decisions of a frame -- bit 3 i: slot i's
// blank state took s - 1; bits 3 i + 1, 3 i + 2: slot i's label state took
// s - 1, s - 2; bit 3 K: the final blank in vF -- into ceil((3 K + 1) / 32)
// words and stores each word plane with one coalesced store:
// bp[row][frame][word][lane].
//
// Band.  States s < S - 2 (frames - f) cannot reach the end any more; a lane
// whose block lies wholly below skips the arithmetic and stores decision 0.
// What its stale states feed lies below the band as well, and the walk back
// never leaves the band.  The other side of the band (states no alignment has
// reached yet) is NOT skipped: the definition gives such a state -inf + lp, and
// a NaN or +inf cell makes that a NaN which stays in the state for good and
// reaches logp when the state is the last one.  Skipping would return -inf
// where the definition says NaN.
//
// Wide rows (ctcx_path_align_lds<T, Fmt>): states and labels in LDS, slot j on
// lane j mod 64, in place from the last chunk of 64 slots down, a barrier
// between a chunk's reads and its writes.  A lane gathers the three bits of ten
// consecutive chunks into one word before it stores it.
//
// Walk back (ctcx_path_align_back): one wave per row, the state uniform.  A
// frame's words sit where the walk does not decide, so every lane loads its own
// words of the next kAlignPrefetch frames while the wave consumes the last
// kAlignPrefetch: the dependent chain per frame is a lane read of the owner's
// word, a shift and a subtraction.  Lane i mod 64 keeps element i (the state)
// and the wave turns 64 of them into labels and stores them as one block.
//
// Nothing is trusted: lengths are clamped to [0, Tmax], a label outside [0, C)
// makes the row a NaN before any logit is read, every logit read is frame
// f < frames <= Tmax of item b, and every state index is clamped into [0, S)
// before it addresses anything.  Every uniform value goes out through a lane's
// vector store.
#include "ctcx_align.h"

#include <atomic>

namespace {

constexpr int kD = kAlignPrefetch;
static_assert(2 * kD <= 64, "the LDS layout's two candidate word planes cover 2 kD frames of drift");

template <typename T>
__device__ __forceinline__ T ninf() { return (T)(-__builtin_inff()); }

// element idx of the row at `row`, widened as the decode kernels' row stage
// widens it (fp16: the hardware convert; bf16: the bits, 16 to the left)
template <typename T, int Fmt>
__device__ __forceinline__ T row_at(const void* row, uint32_t idx) {
  if constexpr (Fmt == kAlignInF16)
    return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)row)[idx]);
  else if constexpr (Fmt == kAlignInBF16)
    return (T)__uint_as_float((unsigned)((const uint16_t*)row)[idx] << 16);
  else
    return ((const T*)row)[idx];
}
template <int Fmt, typename T>
__device__ __forceinline__ const void* row_ptr(const void* x, int64_t off) {
  if constexpr (Fmt == kAlignInNative) return (const T*)x + off;
  else return (const uint16_t*)x + off;
}

template <int Ctrl>
__device__ __forceinline__ int dpp_keep(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, Ctrl, 0xf, 0xf, false);   // a lane without a source keeps `old`
}
// lane l receives lane l - 1's v, lane 0 -inf (wave_shr:1)
__device__ __forceinline__ float from_prev_lane(float v) {
  return __int_as_float(dpp_keep<0x138>(__float_as_int(ninf<float>()), __float_as_int(v)));
}
__device__ __forceinline__ double from_prev_lane(double v) {
  const double o = ninf<double>();
  return __hiloint2double(dpp_keep<0x138>(__double2hiint(o), __double2hiint(v)),
                          dpp_keep<0x138>(__double2loint(o), __double2loint(v)));
}

// the instantiation of a row of m labels: its block size, or 0 for the LDS one
__host__ __device__ constexpr int block_of(int64_t m) {
  return m <= 64 ? 1 : m <= 128 ? 2 : m <= 256 ? 4 : m <= 512 ? 8 : m <= 1024 ? 16 : m <= 1536 ? 24 : 0;
}
static_assert(block_of(64 * kAlignMaxBlock) == kAlignMaxBlock && block_of(64 * kAlignMaxBlock + 1) == 0,
              "block_of, launch_all and the walk back's switch spell the blocks out");
// words a lane stores per frame in the register layout of block K
__host__ __device__ constexpr int reg_words(int K) { return (3 * K + 1 + 31) / 32; }
// ... and in the LDS layout of rows of up to Tmax labels (slots 0 .. Tmax)
__host__ __device__ constexpr int64_t lds_words(int64_t Tmax) {
  return ((Tmax + 1 + 63) / 64 + kAlignLdsChunksPerWord - 1) / kAlignLdsChunksPerWord;
}
__host__ __device__ constexpr int64_t ws_words(int64_t Tmax) {
  const int64_t r = block_of(Tmax) ? reg_words(block_of(Tmax)) : 0, l = lds_words(Tmax);
  return r > l ? r : l;
}
static_assert(ws_words(1500) == 3 && ws_words(64) == 1 && ws_words(1024) == 2 && ws_words(13000) == 21,
              "the workspace formula of the header");

struct Row {
  int64_t bp, b;
  int pth, m, frames;
  bool empty;
};
__device__ __forceinline__ Row read_row(const CtcxAlignParams& p) {
  Row r;
  r.bp = blockIdx.x;
  r.b = r.bp / p.P;
  r.pth = (int)(r.bp - r.b * p.P);
  const int Tmax = (int)p.Tmax;
  auto clampT = [&](int v) { return v < 0 ? 0 : v > Tmax ? Tmax : v; };
  r.empty = p.status && p.status[r.b] != 0;
  r.frames = clampT(p.frames[r.b]);
  r.m = r.empty ? 0 : clampT(p.len[((int64_t)r.pth * 2 + 0) * p.B + r.b]);
  return r;
}

// the forward's two results of a row, through lane 0's vector store
template <typename T>
__device__ __forceinline__ void put_fin(const CtcxAlignParams& p, int64_t bp, T last, T before) {
  T* const fin = (T*)p.fin + bp * 2;
  fin[0] = last;
  fin[1] = before;
}

template <typename T, int Fmt, int K>
__global__ __launch_bounds__(64) void ctcx_path_align_reg(CtcxAlignParams p) {
  const Row r = read_row(p);
  if (p.force_lds || block_of(r.m) != K) return;   // (uniform) another instantiation's row
  const int lane = threadIdx.x;
  const T NINF = ninf<T>(), QNAN = (T)__builtin_nanf("");
  if (r.empty) {
    if (lane == 0) put_fin<T>(p, r.bp, QNAN, QNAN);
    return;
  }
  const int m = r.m, frames = r.frames;
  const int32_t* const d_rev = p.seq + (r.bp * 2 + 0) * p.Tmax;   // token j is element m - 1 - j
  const int j0 = lane * K;
  const int nl = m - j0 < 0 ? 0 : m - j0 > K ? K : m - j0;   // labels of this lane
  uint32_t lab[K];
  unsigned skipm = 0;   // bit i: the s - 2 step into label i is allowed
  bool bad = false;
  int prev = (nl > 0 && j0 > 0) ? d_rev[m - j0] : -1;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    int v = 0;
    if (i < nl) {
      v = d_rev[m - 1 - (j0 + i)];
      bad |= v < 0 || v >= p.C;
      if (j0 + i > 0 && v != prev) skipm |= 1u << i;
      prev = v;
    }
    lab[i] = (uint32_t)v;
  }
  if (__any(bad)) {
    if (lane == 0) put_fin<T>(p, r.bp, QNAN, QNAN);
    return;
  }
  if (frames == 0) {
    if (lane == 0) put_fin<T>(p, r.bp, m == 0 ? (T)0 : NINF, NINF);
    return;
  }
  const T* const nb = (const T*)p.norm + r.b;
  const uint32_t blank = (uint32_t)p.blank_index;
  auto gather = [&](int f, T (&v)[K], T& vb, T& vn) {
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + r.b * p.xst_b);   // uniform
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < nl) v[i] = row_at<T, Fmt>(row, lab[i]);
    vb = row_at<T, Fmt>(row, blank);
    vn = nb[(int64_t)f * p.B];
  };

  const int last_lane = m > 0 ? (m - 1) / K : 0;
  const int li = m - 1 - last_lane * K;   // the last label's slot in its lane; -1: no label
  const bool need_f = li == K - 1;        // (uniform) the final blank has no slot of its own
  const int S = 2 * m + 1;
  const int hi = 2 * (j0 + K) - 1;        // this lane's last label state
  const bool owns = lane == 0 || j0 < m;
  constexpr int NW = reg_words(K);
  const int64_t NWs = ws_words(p.Tmax);
  uint32_t* const bpw = p.bp + r.bp * p.Tmax * NWs * 64 + lane;

  // frame 0 is the definition's v_0
  T cur[K], curB = (T)0, curN = (T)0;
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = NINF;
  gather(0, cur, curB, curN);
  T vB[K], vL[K], vF = NINF;
#pragma unroll
  for (int i = 0; i < K; ++i) vB[i] = vL[i] = NINF;
  if (lane == 0) {
    vB[0] = curB - curN;
    if (m > 0) vL[0] = cur[0] - curN;
  }
  if (frames > 1) gather(1, cur, curB, curN);
  for (int f = 1; f < frames; ++f) {
    T nxt[K], nxtB = curB, nxtN = curN;
#pragma unroll
    for (int i = 0; i < K; ++i) nxt[i] = cur[i];
    if (f + 1 < frames) gather(f + 1, nxt, nxtB, nxtN);
    const T from_prev = from_prev_lane(vL[K - 1]);
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0;
    if (owns && hi >= S - 2 * (frames - f)) {
      const T lpB = curB - curN;
      T pl = from_prev;   // v_{f-1} of the label state in front of slot i's pair
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const T oB = vB[i], oL = vL[i];
        const T lp = i < nl ? cur[i] - curN : NINF;
        const bool b1 = pl > oB;
        vB[i] = (b1 ? pl : oB) + lpB;
        const bool l1 = oB > oL;
        const T best = l1 ? oB : oL;
        const bool l2 = ((skipm >> i) & 1u) && pl > best;
        vL[i] = (l2 ? pl : best) + lp;
        w[(3 * i) >> 5] |= (uint32_t)b1 << ((3 * i) & 31);
        w[(3 * i + 1) >> 5] |= (uint32_t)(l1 && !l2) << ((3 * i + 1) & 31);
        w[(3 * i + 2) >> 5] |= (uint32_t)l2 << ((3 * i + 2) & 31);
        pl = oL;
      }
      if (need_f) {
        const bool b1 = pl > vF;
        vF = (b1 ? pl : vF) + lpB;
        w[(3 * K) >> 5] |= (uint32_t)b1 << ((3 * K) & 31);
      }
    }
    uint32_t* const at = bpw + (int64_t)f * NWs * 64;
#pragma unroll
    for (int k = 0; k < NW; ++k) at[k * 64] = w[k];
#pragma unroll
    for (int i = 0; i < K; ++i) cur[i] = nxt[i];
    curB = nxtB;
    curN = nxtN;
  }
  if (lane == last_lane) {
    T fb = NINF, fl = NINF;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (i == li + 1) fb = vB[i];
      if (i == li) fl = vL[i];
    }
    if (need_f) fb = vF;
    put_fin<T>(p, r.bp, fb, fl);
  }
}

// The pairs in LDS: sB[j] / sL[j] are states 2j / 2j + 1 (slot m holds the final
// blank), sY[j] label j with the s - 2 permission in the sign bit.
template <typename T, int Fmt>
__global__ __launch_bounds__(64) void ctcx_path_align_lds(CtcxAlignParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  const Row r = read_row(p);
  if (!p.force_lds && block_of(r.m) != 0) return;   // (uniform) a register instantiation's row
  const int lane = threadIdx.x;
  const T NINF = ninf<T>(), QNAN = (T)__builtin_nanf("");
  if (r.empty) {
    if (lane == 0) put_fin<T>(p, r.bp, QNAN, QNAN);
    return;
  }
  const int m = r.m, frames = r.frames;
  const int W = (int)p.Tmax + 1;   // m <= Tmax
  T* const sB = (T*)s_mem;
  T* const sL = sB + W;
  int32_t* const sY = (int32_t*)(sL + W);
  const int32_t* const d_rev = p.seq + (r.bp * 2 + 0) * p.Tmax;
  bool bad = false;
  for (int j = lane; j <= m; j += 64) {
    int v = 0;
    if (j < m) {
      v = d_rev[m - 1 - j];
      bad |= v < 0 || v >= p.C;
      if (j > 0 && v != d_rev[m - j]) v |= (int)0x80000000u;
    }
    sY[j] = v;
    sB[j] = NINF;
    sL[j] = NINF;
  }
  __syncthreads();
  if (__any(bad)) {
    if (lane == 0) put_fin<T>(p, r.bp, QNAN, QNAN);
    return;
  }
  if (frames == 0) {
    if (lane == 0) put_fin<T>(p, r.bp, m == 0 ? (T)0 : NINF, NINF);
    return;
  }
  const T* const nb = (const T*)p.norm + r.b;
  const int S = 2 * m + 1;
  const int64_t NWs = ws_words(p.Tmax);
  uint32_t* const bpw = p.bp + r.bp * p.Tmax * NWs * 64 + lane;
  if (lane == 0) {   // frame 0 is the definition's v_0
    const void* const row = row_ptr<Fmt, T>(p.x, r.b * p.xst_b);
    const T nrm = nb[0];
    sB[0] = row_at<T, Fmt>(row, (uint32_t)p.blank_index) - nrm;
    if (m > 0) sL[0] = row_at<T, Fmt>(row, (uint32_t)sY[0] & 0x7fffffffu) - nrm;
  }
  __syncthreads();
  const int ctop = m / 64;   // the chunk of slot m
  for (int f = 1; f < frames; ++f) {
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + r.b * p.xst_b);
    const T nrm = nb[(int64_t)f * p.B];
    const T lpB = row_at<T, Fmt>(row, (uint32_t)p.blank_index) - nrm;
    // the slots that can still reach the end: 2j + 1 >= S - 2 (frames - f)
    const int lo_s = S - 2 * (frames - f);
    const int jlo = lo_s <= 1 ? 0 : lo_s / 2;
    uint32_t* const at = bpw + (int64_t)f * NWs * 64;
    for (int wd = ctop / kAlignLdsChunksPerWord; wd >= 0; --wd) {
      uint32_t acc = 0;
      const int c0 = wd * kAlignLdsChunksPerWord;
      int c = c0 + kAlignLdsChunksPerWord - 1;
      if (c > ctop) c = ctop;
      for (; c >= c0 && c >= jlo / 64; --c) {
        const int j = c * 64 + lane;
        const bool act = j >= jlo && j <= m;
        T oB = NINF, oL = NINF, pl = NINF;
        if (act) {
          oB = sB[j];
          oL = sL[j];
          if (j > 0) pl = sL[j - 1];
        }
        __syncthreads();
        if (act) {
          const bool b1 = pl > oB;
          sB[j] = (b1 ? pl : oB) + lpB;
          uint32_t bits = (uint32_t)b1;
          if (j < m) {
            const int y = sY[j];
            const T lp = row_at<T, Fmt>(row, (uint32_t)y & 0x7fffffffu) - nrm;
            const bool l1 = oB > oL;
            const T best = l1 ? oB : oL;
            const bool l2 = y < 0 && pl > best;
            sL[j] = (l2 ? pl : best) + lp;
            bits |= (uint32_t)(l1 && !l2) << 1 | (uint32_t)l2 << 2;
          }
          acc |= bits << (3 * (c - c0));
        }
        __syncthreads();
      }
      at[wd * 64] = acc;
    }
  }
  if (lane == 0) put_fin<T>(p, r.bp, sB[m], m > 0 ? sL[m - 1] : NINF);
}

// ---------------------------------------------------------------------------
// The walk back.  K: the row's forward layout (0: the LDS one).

template <int K>
__device__ __forceinline__ void walk_back(const CtcxAlignParams& p, const Row& r, int s, int32_t* const v_rev,
                                          const int32_t* const d_rev) {
  constexpr int NQ = K ? reg_words(K) : 2;   // word planes of a frame a lane holds ahead of the walk
  const int lane = threadIdx.x;
  const int m = r.m, frames = r.frames, S = 2 * m + 1;
  const int64_t NWs = ws_words(p.Tmax);
  const uint32_t* const bpw = p.bp + r.bp * p.Tmax * NWs * 64 + lane;
  const int n = frames - 1;   // steps: step t reads frame frames - 1 - t's decision
  const int blank_label = p.blank_label;
  auto lds_word = [&](int st) { return ((st >> 1) >> 6) / kAlignLdsChunksPerWord; };
  // a lane's own words of the kD frames of group g; the LDS layout takes the word plane of state `st` and the one below
  auto fetch = [&](int g, int st, uint32_t (&q)[kD][NQ], int& wb) {
    wb = K ? 0 : lds_word(st);
#pragma unroll
    for (int d = 0; d < kD; ++d) {
      const int t = g * kD + d;
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const int plane = K ? k : wb - 1 + k;
        q[d][k] = (t < n && plane >= 0) ? bpw[((int64_t)(frames - 1 - t) * NWs + plane) * 64] : 0u;
      }
    }
  };
  auto label_of = [&](int st) { return (st & 1) ? d_rev[m - 1 - (st >> 1)] : blank_label; };
  int keep = s;   // element e of the walk is the state of frame frames - 1 - e; lane e mod 64 keeps it
  uint32_t qa[kD][NQ], qb[kD][NQ];
  int wa = 0, wbn = 0;
  fetch(0, s, qa, wa);
  for (int g = 0; g * kD < n; ++g) {
    fetch(g + 1, s, qb, wbn);
#pragma unroll
    for (int d = 0; d < kD; ++d) {
      const int t = g * kD + d;
      if (t < n) {   // (uniform)
        const int j = s >> 1, odd = s & 1;
        int owner, pos;
        uint32_t r0, r1 = 0, r2 = 0;
        if constexpr (K == 0) {
          owner = j & 63;
          const int c = j >> 6, wd = c / kAlignLdsChunksPerWord;
          pos = 3 * (c - wd * kAlignLdsChunksPerWord) + odd;
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)qa[d][0], owner);
          const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)qa[d][1], owner);
          r0 = wd == wa ? hi : wd == wa - 1 ? lo : 0u;
        } else {
          if (j == m && m > 0 && m % K == 0) {
            owner = (m - 1) / K;
            pos = 3 * K;
          } else {
            owner = j / K;
            pos = 3 * (j - owner * K) + odd;
          }
          r0 = (uint32_t)__builtin_amdgcn_readlane((int)qa[d][0], owner);
          if constexpr (NQ > 1) r1 = (uint32_t)__builtin_amdgcn_readlane((int)qa[d][1], owner);
          if constexpr (NQ > 2) r2 = (uint32_t)__builtin_amdgcn_readlane((int)qa[d][2], owner);
        }
        const uint64_t lo64 = (uint64_t)r0 | (uint64_t)r1 << 32, hi64 = (uint64_t)r1 | (uint64_t)r2 << 32;
        const uint32_t two = (uint32_t)(pos < 32 ? lo64 >> pos : hi64 >> (pos - 32)) & 3u;
        const int dec = odd ? (two & 2u ? 2 : (int)(two & 1u)) : (int)(two & 1u);
        s -= dec;
        s = s < 0 ? 0 : s > S - 1 ? S - 1 : s;
        const int e = t + 1;
        if ((e & 63) == 0) {   // (uniform) elements e - 64 .. e - 1 are complete
          v_rev[e - 64 + lane] = label_of(keep);
          keep = s;
        }
        if (lane == (e & 63)) keep = s;
      }
    }
#pragma unroll
    for (int d = 0; d < kD; ++d)
#pragma unroll
      for (int k = 0; k < NQ; ++k) qa[d][k] = qb[d][k];
    wa = wbn;
  }
  // the last block: elements [frames - 1 - (frames - 1) % 64 .. frames)
  const int e0 = (frames - 1) & ~63;
  if (e0 + lane < frames) v_rev[e0 + lane] = label_of(keep);
}

template <typename T>
__global__ __launch_bounds__(64) void ctcx_path_align_back(CtcxAlignParams p) {
  const Row r = read_row(p);
  const int lane = threadIdx.x;
  const int m = r.m, frames = r.frames, S = 2 * m + 1;
  const int32_t* const d_rev = p.seq + (r.bp * 2 + 0) * p.Tmax;
  int32_t* const v_dec = p.vseq + (r.bp * 2 + 0) * p.Tmax;
  int32_t* const v_rev = p.vseq + (r.bp * 2 + 1) * p.Tmax;
  for (int i = lane; i < m; i += 64) v_dec[i] = d_rev[i];
  const T* const fin = (const T*)p.fin + r.bp * 2;
  const T last = fin[0], before = fin[1];
  const bool second = m > 0 && before > last;
  const T logp = second ? before : last;
  const bool aligned = logp > ninf<T>();   // (false for a NaN)
  if (lane == 0) {
    ((T*)p.logp)[r.bp] = logp;
    p.vlen[((int64_t)r.pth * 2 + 0) * p.B + r.b] = m;
    p.vlen[((int64_t)r.pth * 2 + 1) * p.B + r.b] = aligned ? frames : 0;
  }
  if (!aligned || frames == 0) return;
  const int s = __builtin_amdgcn_readfirstlane(second ? S - 2 : S - 1);
  const int K = p.force_lds ? 0 : block_of(m);
  switch (K) {
    case 1: walk_back<1>(p, r, s, v_rev, d_rev); break;
    case 2: walk_back<2>(p, r, s, v_rev, d_rev); break;
    case 4: walk_back<4>(p, r, s, v_rev, d_rev); break;
    case 8: walk_back<8>(p, r, s, v_rev, d_rev); break;
    case 16: walk_back<16>(p, r, s, v_rev, d_rev); break;
    case 24: walk_back<24>(p, r, s, v_rev, d_rev); break;
    default: walk_back<0>(p, r, s, v_rev, d_rev); break;
  }
}

// One thread per element of the padded output, and per row for its length.
__global__ __launch_bounds__(256) void ctcx_path_align_emit(CtcxAlignParams p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rows = p.B * p.P;
  auto length = [&](int64_t bp) {
    const int64_t b = bp / p.P, pth = bp - b * p.P;
    int f = p.frames[b];
    f = f < 0 ? 0 : f > p.Tmax ? (int)p.Tmax : f;
    const int L = p.vlen[(pth * 2 + 1) * p.B + b];
    return L < 0 ? 0 : L > f ? f : L;
  };
  if (idx < rows) p.alignment_length[idx] = length(idx);
  if (idx < rows * p.Tmax) {
    const int64_t bp = idx / p.Tmax;
    const int t = (int)(idx - bp * p.Tmax);
    const int L = length(bp);
    p.alignment[idx] = t < L ? (int64_t)p.vseq[(bp * 2 + 1) * p.Tmax + (L - 1 - t)] : p.pad_value;
  }
}

template <typename T>
constexpr size_t lds_bytes(int64_t Tmax) { return (size_t)(Tmax + 1) * (2 * sizeof(T) + 4); }

template <typename T, int Fmt>
hipError_t launch_all(const CtcxAlignParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(p.B * p.P)), block(64);
  bool lds = p.force_lds != 0;
  if (!lds) {
    // every register instantiation a row of at most Tmax labels can need
    hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 1>), grid, block, 0, s, p);
    if (p.Tmax > 64 * 1) hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 2>), grid, block, 0, s, p);
    if (p.Tmax > 64 * 2) hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 4>), grid, block, 0, s, p);
    if (p.Tmax > 64 * 4) hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 8>), grid, block, 0, s, p);
    if (p.Tmax > 64 * 8) hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 16>), grid, block, 0, s, p);
    if (p.Tmax > 64 * 16) hipLaunchKernelGGL((ctcx_path_align_reg<T, Fmt, 24>), grid, block, 0, s, p);
    lds = p.Tmax > 64 * kAlignMaxBlock;
  }
  if (lds) {
    const size_t bytes = lds_bytes<T>(p.Tmax);
    if (bytes > 64 * 1024) {
      // dynamic LDS above the default limit is allowed once per device and instantiation, for the widest row
      // (a host-side attribute of the function: no stream operation, nothing a capture sees)
      static std::atomic<uint64_t> allowed{0};
      int dev = 0;
      hipError_t e = hipGetDevice(&dev);
      if (e != hipSuccess) return e;
      const uint64_t bit = 1ull << (dev & 63);
      if (!(allowed.load() & bit)) {
        e = hipFuncSetAttribute((const void*)ctcx_path_align_lds<T, Fmt>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes<T>(sizeof(T) == 8 ? kAlignMaxLdsT64 : kAlignMaxLdsT32));
        if (e != hipSuccess) return e;
        allowed.fetch_or(bit);
      }
    }
    hipLaunchKernelGGL((ctcx_path_align_lds<T, Fmt>), grid, block, bytes, s, p);
  }
  return hipGetLastError();
}

}  // namespace

bool ctcx_path_align_fits(int64_t Tmax, int32_t f64, int32_t force_lds) {
  const bool lds = force_lds || Tmax > 64 * kAlignMaxBlock;
  return !lds || Tmax <= (f64 ? kAlignMaxLdsT64 : kAlignMaxLdsT32);
}

int64_t ctcx_align_words(int64_t Tmax) { return ws_words(Tmax < 0 ? 0 : Tmax); }

static bool params_ok(const CtcxAlignParams& p) {
  return !(p.B * p.P > 0x7fffffffLL || p.Tmax < 0 || p.Tmax > 0x7fffffffLL || p.C <= 0 || p.C > 0x7fffffffLL ||
           p.blank_index < 0 || p.blank_index >= p.C || !p.seq || !p.len || !p.frames || !p.fin || !p.vseq ||
           !p.vlen || !p.logp || !p.alignment || !p.alignment_length ||
           (p.Tmax > 0 && (!p.x || !p.norm || !p.bp)) ||
           (p.xfmt != kAlignInNative && (p.f64 || (p.xfmt != kAlignInF16 && p.xfmt != kAlignInBF16))) ||
           !ctcx_path_align_fits(p.Tmax, p.f64, p.force_lds));
}

hipError_t ctcx_launch_path_align(const CtcxAlignParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (!params_ok(p)) return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kAlignInNative>(p, s);
  if (p.xfmt == kAlignInF16) return launch_all<float, kAlignInF16>(p, s);
  if (p.xfmt == kAlignInBF16) return launch_all<float, kAlignInBF16>(p, s);
  return launch_all<float, kAlignInNative>(p, s);
}

hipError_t ctcx_launch_path_align_back(const CtcxAlignParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (!params_ok(p)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.B * p.P)), block(64);
  if (p.f64) hipLaunchKernelGGL(ctcx_path_align_back<double>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(ctcx_path_align_back<float>, grid, block, 0, s, p);
  return hipGetLastError();
}

hipError_t ctcx_launch_path_align_emit(const CtcxAlignParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (!params_ok(p)) return hipErrorInvalidValue;
  const int64_t rows = p.B * p.P, n = rows * (p.Tmax > 0 ? p.Tmax : 1);
  if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_path_align_emit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}
