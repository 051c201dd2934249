// ctcx_stable.hip — the stable prefix of a stream (include/ctcext.h,
// ctcext_stream_stable): how many leading labels of the decoded output are the
// same in every hypothesis this push returns and any later push can return.
//
// Every beam entry alive after an item's newest frame n - 1 has a chain through
// the per-frame records rec[b][t][k]: record (t, k)'s link >> 1 is its source
// position at frame t - 1.  The chains of the live positions 0..m-1 (m: the
// committed CtcxStreamHdr.nb, the records the last commit wrote) merge some
// frames back; every later hypothesis descends from a live entry, so what lies
// on the shared part of the chain is final.
//
// One 256-thread workgroup per item:
//   convergence walk  the chains as the set of occupied positions of the
//       current frame (byte flags, two buffers; two chains on one position stay
//       together, so the set only shrinks).  One step counts the set with
//       ballots while it maps it through link >> 1, one lane per position, one
//       barrier; it stops when the set is one position, (f, k*), or at the
//       cached frontier, where by construction it is one.
//   count walk        from (f, k*) the single chain down to the cached
//       frontier, counting the labels ctcx_traceback's decoded walk emits.
//   frontier cache    {frames, pos, count, last_label} of the last answer per
//       item: every chain of this query passes through it, so neither walk
//       goes below it.
// The records of several frames at a time are staged in LDS with 16-byte
// loads (the next segment's loads in flight, in registers, during this one's
// steps), so a step waits on LDS, not on one dependent global load.  Static
// LDS: two 24-KB segment buffers and two 4-KB flag buffers, 56 KB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CTCX_STREAM_HOST
#include "ctcx_stable.h"

namespace {

using ctcx::rec_link_label;

constexpr int kNT = 256;
constexpr int kLoads = kStableBufBytes / 16 / kNT;   // 16-byte loads per thread per segment
static_assert(kLoads * 16 * kNT == kStableBufBytes, "whole loads");
constexpr int kMaxG = 1024;                          // frames per segment at most

// LDS: records staged, flags in LDS (ctcx_stable_in_lds).  Otherwise the
// records are read in place and the flags live in p.flags (any beam width).
template <bool LDS>
__global__ __launch_bounds__(kNT) void ctcx_stable(CtcxStableParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t buf[LDS ? 2 : 1][LDS ? kStableBufBytes / 4 : 4];
  __shared__ uint8_t lfl[LDS ? 2 : 1][LDS ? kStableLdsW : 4];
  __shared__ int cnt[3], kinfo[3][3];   // per step (rotating): the set's size; a set position, its link and label
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int W = p.W;
  const int rb = ctcx::rec_fmt_bytes(p.rec_fmt);
  const int rw = rb >> 2;   // words per record
  const CtcxStreamHdr hdr = *(const CtcxStreamHdr*)(p.state + b * p.stride);
  const int n = hdr.frames < 0 ? 0 : hdr.frames > p.Tmax ? (int)p.Tmax : hdr.frames;
  const int m = hdr.nb < 0 ? 0 : hdr.nb > W ? W : hdr.nb;
  CtcxStableCache c = p.cache[b];
  if (c.frames < 0 || c.frames > n || c.pos < 0 || c.pos >= W) c = CtcxStableCache{0, 0, 0, -1};
  if (n == 0 || m == 0) {
    if (tid == 0) {
      p.decoded_length[b] = 0;
      p.stable_frames[b] = 0;
      p.walked[b] = 0;
    }
    return;
  }
  const int fc = c.frames - 1;   // the cached frontier's frame (-1: none)
  const uint32_t* recw = (const uint32_t*)p.rec;
  const int64_t item_w = b * p.Tmax * (int64_t)W * rw;   // the item's first word

  uint8_t* fl[2];
  if constexpr (LDS) {
    fl[0] = lfl[0];
    fl[1] = lfl[1];
  } else {
    fl[0] = p.flags + b * 2 * (int64_t)W;
    fl[1] = fl[0] + W;
  }
  for (int q = tid; q < W; q += kNT) {
    fl[0][q] = q < m ? 1 : 0;
    fl[1][q] = 0;
  }
  if (tid < 3) cnt[tid] = 0;

  // segments of staged frames [lo, hi], words [a0, a1) of the record array
  // (absolute, a0 aligned down to 16 bytes); the lowest frame read is fc + 1
  const int lo_all = fc + 1;
  const int G = !LDS ? kMaxG : (kStableBufBytes - 16) / (W * rb) < kMaxG ? (kStableBufBytes - 16) / (W * rb) : kMaxG;
  auto seg = [&](int hi, int& lo, int64_t& a0, int64_t& a1) {
    lo = hi - G + 1 > lo_all ? hi - G + 1 : lo_all;
    a0 = (item_w + (int64_t)lo * W * rw) & ~(int64_t)3;
    a1 = item_w + (int64_t)(hi + 1) * W * rw;
  };
  uint4 ld[kLoads];
  auto load = [&](int64_t a0, int64_t a1) {   // into registers; the last piece word by word (never past a1)
    if constexpr (LDS) {
#pragma unroll
      for (int q = 0; q < kLoads; ++q) {
        const int64_t w = a0 + 4 * ((int64_t)q * kNT + tid);
        if (w + 4 <= a1) {
          ld[q] = *(const uint4*)(recw + w);
        } else if (w < a1) {
          ld[q].x = recw[w];
          ld[q].y = w + 1 < a1 ? recw[w + 1] : 0u;
          ld[q].z = w + 2 < a1 ? recw[w + 2] : 0u;
          ld[q].w = 0u;
        }
      }
    }
  };
  auto store = [&](int bi, int64_t a0, int64_t a1) {
    if constexpr (LDS) {
#pragma unroll
      for (int q = 0; q < kLoads; ++q) {
        const int64_t w = a0 + 4 * ((int64_t)q * kNT + tid);
        if (w < a1) *(uint4*)&buf[bi][4 * (q * kNT + tid)] = ld[q];
      }
    }
  };

  // block-uniform state of the walks
  bool conv = false;         // the set was one position at (f, ks)
  bool never = false;        // the chains reached frame 0 apart
  int f = -1, ks = 0;
  int cur = 0;               // flag buffer of the current frame's set
  int step = 0;              // convergence steps done (cnt / kinfo rotate on it)
  int walked = 0;
  // thread 0: the count walk
  int k = 0, nlab = 0, prev = -1, newest = -1;
  bool any = false;

  int hi = n - 1, lo = 0, lo1 = 0;
  int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  const bool have = hi >= lo_all;   // frames above the cached frontier
  if (have) {
    seg(hi, lo, a0, a1);
    load(a0, a1);
    store(0, a0, a1);
  }
  __syncthreads();   // flags, counters and the first segment written
  for (int s = 0; have; ++s) {
    const int bi = s & 1;
    const bool more = lo > lo_all && !never;
    if (more) {   // the next segment's loads in flight during this one's steps
      seg(lo - 1, lo1, b0, b1);
      load(b0, b1);
    }
    auto rec_at = [&](int t, int pos, uint32_t& link, int& lab) {
      const int64_t wr = item_w + ((int64_t)t * W + pos) * rw;
      if constexpr (LDS) rec_link_label(&buf[bi][wr - a0], p.rec_fmt, link, lab);
      else rec_link_label(recw + wr, p.rec_fmt, link, lab);
    };
    for (int t = hi; t >= lo && !never; --t) {
      if (!conv) {
        // one step, one barrier: the set of frame t is counted while it is
        // mapped through link >> 1 onto frame t - 1.  A count of one makes
        // (t, that position) the meeting point, and the mapping just done the
        // count walk's first step (its holder leaves the record in kinfo).
        const int ci = step % 3;
        uint8_t* const fa = fl[cur];
        uint8_t* const fb = fl[cur ^ 1];
        if (tid == 0) cnt[(step + 1) % 3] = 0;
        int mine = 0;
        for (int base = 0; base < W; base += kNT) {   // (uniform trip count: every lane takes part in the ballot)
          const int pos = base + tid;
          const bool on = pos < W && fa[pos] != 0;
          mine += __popcll(__ballot(on));
          if (on) {
            fa[pos] = 0;   // (this buffer is the step after next's target)
            uint32_t link;
            int lab;
            rec_at(t, pos, link, lab);
            const uint32_t src = link >> 1;
            if (src < (uint32_t)W) fb[src] = 1;
            kinfo[ci][0] = pos;   // (read only when one position is set)
            kinfo[ci][1] = (int)link;
            kinfo[ci][2] = lab;
          }
        }
        if ((tid & 63) == 0 && mine) atomicAdd(&cnt[ci], mine);
        __syncthreads();
        ++walked;
        ++step;
        cur ^= 1;
        const int c1 = cnt[ci];
        if (c1 == 1) {
          conv = true;
          f = t;
          ks = kinfo[ci][0];
          if (tid == 0) {
            const uint32_t link = (uint32_t)kinfo[ci][1];
            if (link & 1u) {   // (the newest label of the count walk: nothing to merge with yet)
              ++nlab;
              newest = prev = kinfo[ci][2];
              any = true;
            }
            const uint32_t src = link >> 1;
            k = src < (uint32_t)W ? (int)src : 0;
          }
        } else if (c1 == 0 || t == 0) {
          // frame 0's set is still several positions (fc == -1): the chains never meet
          // (a count of 0: records no chain of this stream writes; answer nothing)
          never = true;
        }
      } else if (tid == 0) {
        // the count walk: record (t, k) of the single chain, as ctcx_traceback's decoded walk
        uint32_t link;
        int lab;
        rec_at(t, k, link, lab);
        if (link & 1u) {
          if (!p.merge || lab != prev) ++nlab;
          if (!any) newest = lab;
          any = true;
          prev = lab;
        }
        const uint32_t src = link >> 1;
        k = src < (uint32_t)W ? (int)src : 0;
      }
    }
    if (more) store(bi ^ 1, b0, b1);
    __syncthreads();   // the next buffer written; this one free for the segment after
    if (!more) break;
    hi = lo - 1;
    lo = lo1;
    a0 = b0;
    a1 = b1;
  }
  if (tid != 0) return;
  int out_len = 0, out_frames = 0;
  if (never) {
    // no frame holds all chains on one position (only without a cached frontier)
  } else if (!conv || f == fc) {
    // the chains meet at the cached frontier, where by construction they are one
    out_len = c.count;
    out_frames = c.frames;
  } else {
    // (f, ks) above the frontier: the labels of frames (fc, f] on top of the
    // cached count; with merge_repeated the oldest of them merges into the
    // cached chain's newest label when the two are equal
    int total = c.count + nlab;
    if (p.merge && any && c.count > 0 && prev == c.last_label) --total;
    CtcxStableCache nc;
    nc.frames = f + 1;
    nc.pos = ks;
    nc.count = total;
    nc.last_label = any ? newest : (c.count > 0 ? c.last_label : -1);
    p.cache[b] = nc;
    out_len = total;
    out_frames = f + 1;
  }
  p.decoded_length[b] = out_len;
  p.stable_frames[b] = out_frames;
  p.walked[b] = walked;
}

}  // namespace

hipError_t ctcx_launch_stable(const CtcxStableParams& p, hipStream_t s) {
  if (p.B == 0) return hipSuccess;
  if (ctcx_stable_in_lds(p.W, p.rec_fmt)) {
    hipLaunchKernelGGL(ctcx_stable<true>, dim3((unsigned)p.B), dim3(kNT), 0, s, p);
  } else {
    if (!p.flags) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctcx_stable<false>, dim3((unsigned)p.B), dim3(kNT), 0, s, p);
  }
  return hipGetLastError();
}
