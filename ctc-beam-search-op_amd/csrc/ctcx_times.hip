// ctcx_times.hip — token start/end frames and the trailing blank count of each
// path's best alignment (include/ctcext.h, "Token times"), from the rows the
// traceback leaves in the workspace.  A translation unit of its own: the decode
// objects neither see nor depend on it.
//
// One 256-thread workgroup per (item, path) row.  The traceback's walks are
// reversed, so "from the end" is index 0 upward: element i of the alignment
// walk is frame frames - 1 - i, element g of the decoded walk is token
// m - 1 - g.  A row is covered in tiles of kTimesTile elements, one per thread,
// with three scans per tile and a carry between tiles:
//   last     the index of the last non-blank element before i (exclusive
//            max-scan): the end of the previous run, whose label is the
//            "previous non-blank run's";
//   group    the number of group heads up to i (inclusive count): a group head
//            is the first element of a non-blank run and, with merge_repeated,
//            of a run whose label differs from the previous non-blank run's.
//            Group g belongs to token g of the reversed decoded walk;
//   K        the lowest group whose label is not its token's, or that has no
//            token (a minimum, kept in LDS across tiles): groups below K are
//            the matched prefix, the prefix-AND of the definition.
// The head of group g < K writes its token's end, and the head of group
// g <= K the start of token g - 1 (the last non-blank element before it); the
// last group's start is written from the carry after the last tile.  Nothing
// past the tile that finds K is read.  Every row element that is not a timed
// token is written -1 by a fill over the complement, so no element is written
// twice.
#include "ctcx_times.h"

namespace {

constexpr int kNT = kTimesTile;
constexpr int kWaves = kNT / 64;
constexpr int kNone = 0x7fffffff;

__global__ __launch_bounds__(kNT) void ctcx_token_times(CtcxTimesParams p) {
  __shared__ int s_last[2][kWaves], s_cnt[2][kWaves];   // per-wave totals, by tile parity
  __shared__ int s_K;
  const int64_t bp = blockIdx.x;
  const int64_t b = bp / p.P;
  const int pth = (int)(bp - b * p.P);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tmax = (int)p.Tmax;
  auto clampT = [&](int v) { return v < 0 ? 0 : v > Tmax ? Tmax : v; };
  const bool empty = p.status && p.status[b] != 0;
  const int frames = clampT(p.frames[b]);
  const int m = empty ? 0 : clampT(p.len[((int64_t)pth * 2 + 0) * p.B + b]);
  int L = empty ? 0 : clampT(p.len[((int64_t)pth * 2 + 1) * p.B + b]);
  if (L > frames) L = frames;   // (a walk is never longer than its item: frame numbers stay >= 0)
  const int32_t* const d_rev = p.seq + (bp * 2 + 0) * p.Tmax;
  const int32_t* const a_rev = p.seq + (bp * 2 + 1) * p.Tmax;
  int32_t* const start = p.start ? p.start + bp * p.Tmax : nullptr;
  int32_t* const end = p.end ? p.end + bp * p.Tmax : nullptr;
  const int blank = p.blank_label;
  const bool want = start != nullptr && m > 0;   // token rows to write (else: trailing_blank only)

  if (tid == 0) s_K = kNone;
  __syncthreads();
  int c_last = -1;   // carries (uniform): the last non-blank index so far, groups so far, the lowest bad group
  int c_cnt = 0;
  int K = kNone;
  for (int base = 0; base < L; base += kNT) {
    const int par = (base / kNT) & 1;
    const int i = base + tid;
    const bool in = i < L;
    const int v = in ? a_rev[i] : blank;
    const bool nb = in && v != blank;
    const bool head = nb && (i == 0 || a_rev[i - 1] != v);
    // last: inclusive max-scan of (nb ? i : -1) within the wave, then across waves
    int x = nb ? i : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d && y > x) x = y;
    }
    if (lane == 63) s_last[par][wave] = x;
    int lastx = __shfl_up(x, 1, 64);   // exclusive within the wave
    if (lane == 0) lastx = -1;
    __syncthreads();
    int last = c_last > lastx ? c_last : lastx;
    int t_last = c_last;
    for (int w = 0; w < kWaves; ++w) {
      const int y = s_last[par][w];
      if (w < wave && y > last) last = y;
      if (y > t_last) t_last = y;
    }
    // group heads; last < i, and a_rev[last] is a non-blank run's label
    const bool ghead = head && (!p.merge || last < 0 || a_rev[last] != v);
    int c = ghead ? 1 : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(c, d, 64);
      if (lane >= d) c += y;
    }
    if (lane == 63) s_cnt[par][wave] = c;
    __syncthreads();
    int g = c_cnt + c - 1, t_cnt = c_cnt;
    for (int w = 0; w < kWaves; ++w) {
      const int y = s_cnt[par][w];
      if (w < wave) g += y;
      t_cnt += y;
    }
    // (with no token rows asked for, group 0's position is all that is read: stop after it)
    if (ghead && (!want || g >= m || d_rev[g] != v)) atomicMin(&s_K, g);
    __syncthreads();
    K = s_K;
    if (ghead) {
      if (g == 0 && p.trailing_blank) p.trailing_blank[bp] = i;
      if (want) {
        if (g < K) end[m - 1 - g] = frames - 1 - i;
        if (g >= 1 && g <= K) start[m - g] = frames - 1 - last;
      }
    }
    c_last = t_last;
    c_cnt = t_cnt;
    if (K != kNone) break;
  }
  // the timed tokens: groups [0, nt), tokens [m - nt, m)
  const int nt = !want ? 0 : K != kNone ? K : c_cnt;
  if (tid == 0) {
    if (K == kNone && c_cnt > 0 && want) start[m - c_cnt] = frames - 1 - c_last;
    if (c_cnt == 0 && p.trailing_blank) p.trailing_blank[bp] = L;
  }
  if (start) {
    for (int q = tid; q < Tmax; q += kNT)
      if (q < m - nt || q >= m) {
        start[q] = -1;
        end[q] = -1;
      }
  }
}

}  // namespace

hipError_t ctcx_launch_token_times(const CtcxTimesParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (p.B * p.P > 0x7fffffffLL || p.Tmax < 0 || p.Tmax > 0x7fffffffLL || !p.seq || !p.len || !p.frames ||
      (p.start == nullptr) != (p.end == nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_token_times, dim3((unsigned)(p.B * p.P)), dim3(kNT), 0, s, p);
  return hipGetLastError();
}
