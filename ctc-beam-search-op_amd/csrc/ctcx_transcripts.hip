// ctcx_transcripts.hip — the forced Viterbi alignment of whole transcripts the
// caller supplies (include/ctcext.h, "Transcript alignments"): the definition of
// the path alignments over one label row of up to 2047 labels per target, with
// the walk back, the token times and the token scores in the same launch.  A
// translation unit of its own: the decode objects neither see nor depend on it.
//
// Work split (ctcx_transcript_align<T, Fmt, K>).  One workgroup of 256 threads
// (four waves, one per SIMD) per target.  Thread t holds the K label pairs
// [t K, t K + K) in registers: slot j is the pair (blank state 2j, label state
// 2j + 1), slot m the final blank.  The call's max_target picks K, the smallest
// of 1, 2, 4, 8 with 256 K > max_target, so slot m always has a register.
//
// Forward, time-skewed across the waves.  Within a wave the step is that of
// ctcx_path_align_reg: one DPP wave_shr:1 a frame, per state two strict
// compares, two selects and one add in the definition's order, frame 0 written,
// frame f + 1's gathers issued before frame f's arithmetic.  The only thing a
// wave needs from another is the previous frame's value of the last label state
// of the wave below.  Frames 1 .. frames - 1 are cut into blocks of
// kTranscriptBlockFrames; in phase p wave w runs block p - w.  Before it updates
// frame f, lane 63 of wave w writes that state into edge[w][block parity]
// [f within the block]; lane 0 of wave w + 1 reads it one phase later in place
// of the DPP's -inf.  One __syncthreads() separates the phases: one barrier per
// twenty frames.  Every wave runs blocks + active_waves - 1 phases, uniform per
// workgroup; no wave polls or spins.  Two parities are enough: wave w writes
// block k + 2 into the buffer of block k in the phase after wave w + 1 read it.
//
// Band.  States s < S - 2 (frames - f) cannot reach the end any more; a thread
// whose slots lie wholly below skips the arithmetic and stores decision 0.  The
// other side of the band is not skipped (ctcx_align.hip's header comment says
// why: -inf + NaN is the definition's NaN).
//
// Decisions.  Per slot three bits a frame, as ctcx_talign.hip lays them out: bit
// 0 for the blank state (1: from the label in front), bits 1..2 for the label
// state (1: from its blank, 2: the skip).  A thread packs 32 / (3 K) frames into
// a word and stores bp[target][frame / frames_per_word][thread]: one coalesced
// 1 KiB store per workgroup per word.
//
// Walk back, after one __syncthreads(): the words were written by this
// workgroup, so the barrier is all the ordering there is.  Wave 0 walks with
// the state uniform.  The frames are cut into groups of kGF (30 or 32) frames,
// whole words.  The state drops by at most two a frame, so the owner thread
// moves down by at most kGF / K + 1 threads per group: lane i loads the group's
// words of thread base - i, where base is the owner when the loads are issued,
// one group ahead of their use (at most 61 lanes of drift).  A step is a
// readlane from lane base - owner, a shift and a subtraction; the state is
// clamped into [0, S) and written into an LDS row, uint16 [frames].
//
// Epilogue, all 256 threads.  Over frames: where a label state begins or ends
// its run, start[j] / end[j]; the frame's class into the alignment row; the
// first frame of the final blank gives trailing_blank.  Over labels, after a
// barrier: lp[f][y[j]] summed over the span in frame order, one rounded
// subtraction and one rounded add per frame, and the minimum.
//
// Nothing is trusted: frames are clamped to [0, Tmax]; a length outside
// [0, max_target] or a label outside [0, C) makes the target NaN before any
// logit is read with it; every logit read is frame f < frames <= Tmax of item
// b, class c < C; a readlane's lane is masked into the wave; every LDS index
// is below its array's size; every store goes to the target's own cells or the
// thread's own words.
#include "ctcx_transcripts.h"

#include "ctcx_lse.h"
#include "ctcx_paths.h"   // kPathsIn*

namespace {

static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");
constexpr int kF = kTranscriptBlockFrames;

template <typename T>
__device__ __forceinline__ T qnan() { return (T)__builtin_nanf(""); }

// the dynamic LDS of a launch: the edge buffers [3][2][kF], the forward's two results, the walk's states
template <typename T>
constexpr size_t lds_bytes(int64_t Tmax) { return (size_t)(3 * 2 * kF + 2) * sizeof(T) + (((size_t)Tmax * 2 + 15) & ~(size_t)15); }

template <typename T, int Fmt, int K>
__global__ __launch_bounds__(kTranscriptThreads) void ctcx_transcript_align(CtcxTalignParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  constexpr int kLogK = K == 1 ? 0 : K == 2 ? 1 : K == 4 ? 2 : 3;
  constexpr int kFpw = ctcx_transcript_word_frames_of(K);        // frames per decision word
  constexpr int kNwg = K == 1 ? 3 : K == 2 ? 6 : K == 4 ? 16 : 32;   // words of a walk group
  constexpr int kGF = kNwg * kFpw;                               // its frames: 30, 30, 32, 32
  static_assert((1 << kLogK) == K && 2 * kGF / K + 1 < 64, "two groups of drift stay inside the wave");
  const CtcxTargetsParams& p = q.t;
  T* const edge = (T*)s_mem;
  T* const fin = edge + 3 * 2 * kF;
  uint16_t* const st = (uint16_t*)(fin + 2);   // [Tmax]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t row = blockIdx.x;              // b * N + n
  const int64_t b = row / p.N, ti = p.shared ? row - b * p.N : row;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax, L = (int)p.L;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;

  for (int j = tid; j < L; j += kTranscriptThreads) {   // (the epilogue overwrites the cells of timed labels)
    q.start[row * L + j] = -1;
    q.end[row * L + j] = -1;
  }

  // the target: its length, this thread's labels and their s - 2 permissions
  auto label_at = [&](int j) -> int64_t {   // j < m <= L
    return p.labels_i64 ? ((const int64_t*)p.targets)[ti * L + j] : (int64_t)((const int32_t*)p.targets)[ti * L + j];
  };
  bool nan = p.status && p.status[b] != 0;
  const int32_t len = p.target_length[ti];
  if (len < 0 || len > L) nan = true;
  int m = nan ? 0 : len;
  const int j0 = tid * K;
  int nl = m - j0 < 0 ? 0 : m - j0 > K ? K : m - j0;   // labels of this thread
  uint32_t lab[K];
  unsigned skipm = 0;   // bit i: the s - 2 step into label i is allowed
  bool bad = false;
  {
    int64_t prev = (nl > 0 && j0 > 0) ? label_at(j0 - 1) : -1;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      int64_t v = 0;
      if (i < nl) {
        v = label_at(j0 + i);
        if (j0 + i > 0 && v != prev) skipm |= 1u << i;
        prev = v;
      }
      const bool out = v < 0 || v >= p.C;
      bad |= out;
      lab[i] = out ? 0u : (uint32_t)v;
    }
  }
  if (__syncthreads_or(bad ? 1 : 0)) nan = true;   // (uniform) one bad label makes the target NaN
  if (nan) m = nl = 0;

  const int S = 2 * m + 1;
  const int hi = 2 * (j0 + K) - 1;                 // this thread's last label state
  const bool owns = !nan && j0 <= m;               // a thread with a slot of the target
  const int aw = (m >> kLogK) / 64 + 1;            // waves with such a thread: <= 4, as m <= L < 256 K
  const int nblocks = !nan && frames > 1 ? (frames - 1 + kF - 1) / kF : 0;
  const int phases = nblocks ? nblocks + aw - 1 : 0;   // (uniform)
  const int64_t nwords = ((int64_t)Tmax + kFpw - 1) / kFpw;
  uint32_t* const bpw = q.bp + (size_t)row * (size_t)nwords * kTranscriptThreads;
  const T* const nb = (const T*)p.norm + b;
  const uint32_t blank = (uint32_t)p.blank_index;
  auto gather = [&](int f, T (&v)[K], T& vb, T& vn) {   // f < frames
    const void* const xr = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);   // uniform
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < nl) v[i] = row_at<T, Fmt>(xr, lab[i]);
    vb = row_at<T, Fmt>(xr, blank);
    vn = nb[(int64_t)f * p.B];
  };

  // ---- forward.  "Frame -1" is what frames == 0 ends with; frame 0 is the definition's v_0
  T vB[K], vL[K], cur[K], curB = (T)0, curN = (T)0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    vB[i] = vL[i] = NINF;
    cur[i] = (T)0;
  }
  if (tid == 0) vB[0] = (T)0;
  if (tid == 0 && !nan && frames > 0) {
    gather(0, cur, curB, curN);
    vB[0] = curB - curN;
    if (m > 0) vL[0] = cur[0] - curN;
  }
  if (owns && frames > 1) gather(1, cur, curB, curN);
  uint32_t acc = 0;
  int pos = 1 % kFpw;   // frame 1's place in its word
  for (int ph = 0; ph < phases; ++ph) {
    const int k = ph - w;   // this wave's block
    if (w < aw && k >= 0 && k < nblocks) {   // (uniform in the wave)
      const int f0 = 1 + k * kF;
      const int f1 = frames - 1 < f0 + kF - 1 ? frames - 1 : f0 + kF - 1;
      const T* const ein = edge + ((w > 0 ? w - 1 : 0) * 2 + (k & 1)) * kF;   // read with w > 0
      T* const eout = edge + ((w < 3 ? w : 0) * 2 + (k & 1)) * kF;            // written with w < 3
      T ecur = w > 0 ? ein[0] : NINF;
      for (int f = f0; f <= f1; ++f) {
        const int fi = f - f0;   // < kF
        T nxt[K], nxtB = curB, nxtN = curN;
#pragma unroll
        for (int i = 0; i < K; ++i) nxt[i] = cur[i];
        if (owns && f + 1 < frames) gather(f + 1, nxt, nxtB, nxtN);
        const T enxt = (w > 0 && f < f1) ? ein[fi + 1] : NINF;
        const T got = from_prev_lane(vL[K - 1]);   // (every lane: the DPP move is no place to diverge)
        if (lane == 63 && w < 3) eout[fi] = vL[K - 1];
        uint32_t bits = 0;
        if (owns && hi >= S - 2 * (frames - f)) {
          const T lpB = curB - curN;
          T pl = lane == 0 ? ecur : got;   // v_{f-1} of the label state in front of slot i's pair
#pragma unroll
          for (int i = 0; i < K; ++i) {
            const T oB = vB[i], oL = vL[i];
            const T lp = i < nl ? cur[i] - curN : NINF;
            const bool b1 = pl > oB;
            vB[i] = (b1 ? pl : oB) + lpB;
            const bool l1 = oB > oL;
            const T mid = l1 ? oB : oL;
            const bool l2 = ((skipm >> i) & 1u) && pl > mid;
            vL[i] = (l2 ? pl : mid) + lp;
            bits |= ((b1 ? 1u : 0u) | (l2 ? 4u : l1 ? 2u : 0u)) << (3 * i);
            pl = oL;
          }
        }
        if (owns) {
          acc |= bits << (3 * K * pos);
          ++pos;
          if (pos == kFpw || f == frames - 1) {
            bpw[(size_t)(f / kFpw) * kTranscriptThreads + tid] = acc;   // f / kFpw < nwords
            acc = 0;
            pos = pos == kFpw ? 0 : pos;
          }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) cur[i] = nxt[i];
        curB = nxtB;
        curN = nxtN;
        ecur = enxt;
      }
    }
    __syncthreads();   // the phase's edge values are whole; the buffers of two phases ago are free
  }

  // ---- the end state: slot m holds the final blank, the slot in front of it the last label
  {
    const int tm = m >> kLogK, im = m & (K - 1), tl = (m - 1) >> kLogK, il = (m - 1) & (K - 1);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (tid == tm && i == im) fin[0] = vB[i];
      if (m > 0 && tid == tl && i == il) fin[1] = vL[i];
    }
  }
  __syncthreads();   // ... and every decision word of the workgroup is written
  const T last = fin[0], before = m > 0 ? fin[1] : NINF;
  const bool second = m > 0 && before > last;
  T logp = second ? before : last;
  if (nan) logp = qnan<T>();
  const bool aligned = logp > NINF;   // (uniform; false for a NaN)

  // ---- walk back: wave 0, the state uniform
  if (w == 0 && aligned && frames > 0) {
    int s = __builtin_amdgcn_readfirstlane(second ? S - 2 : S - 1);
    const int wlast = (frames - 1) / kFpw;   // the last word the forward stored
    auto fetch = [&](int g, int base, uint32_t (&qq)[kNwg]) {   // lane i: the group's words of thread base - i
      const int th = base - lane;   // base <= m / K <= 255
#pragma unroll
      for (int c = 0; c < kNwg; ++c) {
        const int wi = g * kNwg + c;
        qq[c] = (g >= 0 && th >= 0 && wi <= wlast) ? bpw[(size_t)wi * kTranscriptThreads + th] : 0u;
      }
    };
    uint32_t qa[kNwg], qb[kNwg];
    int g = (frames - 1) / kGF;
    int base_a = (s >> 1) >> kLogK;
    fetch(g, base_a, qa);
    for (; g >= 0; --g) {
      const int base_b = (s >> 1) >> kLogK;
      fetch(g - 1, base_b, qb);
#pragma unroll
      for (int d = kGF - 1; d >= 0; --d) {
        const int f = g * kGF + d;
        if (f < frames) {   // (uniform)
          if (lane == 0) st[f] = (uint16_t)s;   // f < frames <= Tmax
          const int j = s >> 1;
          const int src = (base_a - (j >> kLogK)) & 63;
          const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)qa[d / kFpw], src);
          const uint32_t two = word >> (3 * K * (d % kFpw) + 3 * (j & (K - 1)));
          const int dec = (s & 1) ? (int)((two >> 1) & 3u) : (int)(two & 1u);   // (frame 0's bits are 0)
          s -= dec;
          s = s < 0 ? 0 : s > S - 1 ? S - 1 : s;
        }
      }
#pragma unroll
      for (int c = 0; c < kNwg; ++c) qa[c] = qb[c];
      base_a = base_b;
    }
  }
  __syncthreads();

  // ---- epilogue over frames: the spans' ends, the alignment row, the trailing blanks
  const bool walked = aligned && frames > 0;
  int32_t* const ali = q.alignment ? q.alignment + row * p.Tmax : nullptr;
  for (int f = tid; f < Tmax; f += kTranscriptThreads) {
    int cls = -1;
    if (walked && f < frames) {
      const int s = st[f];   // in [0, S)
      const int sp = f > 0 ? (int)st[f - 1] : -1, sn = f + 1 < frames ? (int)st[f + 1] : -1;
      if (s & 1) {           // label j = s >> 1 < m
        const int j = s >> 1;
        if (sp != s) q.start[row * L + j] = f;
        if (sn != s) q.end[row * L + j] = f;
        cls = ali ? (int)label_at(j) : 0;
      } else {
        cls = (int)blank;
      }
      if (s == 2 * m && sp != s) q.trailing_blank[row] = frames - f;
    }
    if (ali) ali[f] = cls;
  }
  if (tid == 0) {
    ((T*)p.out)[row] = logp;
    if (!(walked && (int)st[frames - 1] == 2 * m)) q.trailing_blank[row] = 0;
  }
  if (!q.logp_sum && !q.logp_min) return;   // (uniform)
  __syncthreads();   // the workgroup's start and end cells are written

  // ---- epilogue over labels: the scores of each label's span
  for (int j = tid; j < L; j += kTranscriptThreads) {
    const int64_t cell = row * L + j;
    T sum = qnan<T>(), mn = qnan<T>();
    if (walked && j < m) {
      const int sa = q.start[cell], en = q.end[cell];
      if (sa >= 0 && sa <= en && en < frames) {
        const uint32_t c = (uint32_t)label_at(j);   // checked above: < C
        for (int f = sa; f <= en; ++f) {
          const void* const xr = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
          const T lp = row_at<T, Fmt>(xr, c) - nb[(int64_t)f * p.B];
          if (f == sa) {
            sum = mn = lp;
          } else {
            sum = sum + lp;
            if (lp < mn) mn = lp;
          }
        }
      }
    }
    if (q.logp_sum) ((T*)q.logp_sum)[cell] = sum;
    if (q.logp_min) ((T*)q.logp_min)[cell] = mn;
  }
}

template <typename T, int Fmt, int K>
hipError_t launch_block(const CtcxTalignParams& q, hipStream_t s) {
  hipLaunchKernelGGL((ctcx_transcript_align<T, Fmt, K>), dim3((unsigned)(q.t.B * q.t.N)), dim3(kTranscriptThreads),
                     lds_bytes<T>(q.t.Tmax), s, q);
  return hipGetLastError();
}

template <typename T, int Fmt>
hipError_t launch_all(const CtcxTalignParams& q, hipStream_t s) {
  switch (ctcx_transcript_block(q.t.L)) {
    case 1: return launch_block<T, Fmt, 1>(q, s);
    case 2: return launch_block<T, Fmt, 2>(q, s);
    case 4: return launch_block<T, Fmt, 4>(q, s);
    case 8: return launch_block<T, Fmt, 8>(q, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

static_assert(ctcx_transcript_bytes(1, 1, 7, 10) == 1024 && ctcx_transcript_bytes(2, 3, 256, 11) == 6 * 3 * 1024 &&
                  ctcx_transcript_bytes(1, 1, 1023, 3) == 2 * 1024 && ctcx_transcript_bytes(1, 1, 2047, 3) == 3 * 1024 &&
                  ctcx_transcript_bytes(1, 1, 2048, 1) == -1,
              "a workgroup stores 1 KiB per word");
static_assert(lds_bytes<double>(kTranscriptMaxTime) <= 64 * 1024, "the dynamic LDS stays below the default limit");

hipError_t ctcx_launch_transcript_align(const CtcxTalignParams& q, hipStream_t s) {
  const CtcxTargetsParams& p = q.t;
  if (p.B <= 0 || p.N <= 0) return hipSuccess;
  if (p.Tmax < 0 || p.Tmax > kTranscriptMaxTime || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 ||
      p.blank_index >= p.C || !p.target_length || (p.L > 0 && !p.targets) || !p.frames || !p.out ||
      (p.Tmax > 0 && (!p.x || !p.norm || !q.bp)) || (p.L > 0 && (!q.start || !q.end)) || !q.trailing_blank ||
      (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))) ||
      !ctcx_transcript_block(p.L) || p.B * p.N > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kPathsInNative>(q, s);
  if (p.xfmt == kPathsInF16) return launch_all<float, kPathsInF16>(q, s);
  if (p.xfmt == kPathsInBF16) return launch_all<float, kPathsInBF16>(q, s);
  return launch_all<float, kPathsInNative>(q, s);
}
