// ctcx_stream_dense.hip — the device side of the enqueue-only push of a stream
// (include/ctcext.h, ctcext_stream_push_dense): the two decisions the
// synchronous push takes on the host, taken on the device, so that a push is a
// fixed chain of launches over fixed addresses.
//
//   ctcx_stream_prologue   one thread per item, before the pre-pass.  Applies
//       reset[b] (the committed header and the stable-prefix cache entry go to
//       zero: the item's next frame runs Reset()), checks the chunk's length
//       against chunk_time and the stream's capacity, and writes the length the
//       kernels read (0 for an item that fails either check), cum[b] (the
//       traceback's lengths), this push's status bits and the accumulators
//       ctcext_stream_check reports from.
//   ctcx_stream_commit     one 256-thread workgroup per item, after the decode.
//       The decode read the committed buffer and wrote the other one.  Where
//       the item's hand-over held (ItemOut.pad == 0) its header, top arrays and
//       image are copied back over the committed buffer with 16-byte loads and
//       stores: the item is committed, and the buffers never swap, so the same
//       launch can run again (a captured graph).  Where it did not, the
//       committed state stays, cum[b] goes back to the committed frames, and
//       the item's results (ItemOut, top_pos, top_kind, log_prob) are put back
//       to what the committed header holds, so the traceback that follows walks
//       valid records.  It also writes the push's final status and frames.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CTCX_STREAM_HOST
#include "ctcx_stream_dense.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kNT = 256;

__global__ __launch_bounds__(kNT) void ctcx_stream_prologue(CtcxStreamPrologueParams p) {
  const int64_t b = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (b >= p.B) return;
  CtcxStreamHdr* const hdr = (CtcxStreamHdr*)(p.state + b * p.stride);
  if (p.reset && p.reset[b] != 0) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int q = 0; q < (int)(sizeof(CtcxStreamHdr) / 16); ++q) ((u32x4*)hdr)[q] = z;
    *(u32x4*)(p.cache + b) = z;
    if (p.skip) *(u32x4*)(p.skip + b) = z;
  }
  const int64_t recs = hdr->frames;
  const int64_t frames = p.skip ? (int64_t)p.skip[b].n : recs;
  int64_t v = p.chunk_length ? (int64_t)p.chunk_length[b] : p.chunk_time;
  if (v < 0) v = 0;
  int32_t st = 0;
  if (v > p.chunk_time) st |= ctcx::kItemLength;
  if (frames + v > p.max_frames) st |= kCtcxItemCapacity;
  const int32_t n = st ? 0 : (int32_t)v;
  p.sl[b] = n;
  p.cum[b] = (int32_t)recs + n;   // (a skipping stream's chunk plan writes it again, with the frames it keeps)
  p.pre[b] = st;
  if (st) {
    CtcxStreamAcc a = p.acc[b];
    if ((st & ctcx::kItemLength) && !(a.status & ctcx::kItemLength)) a.len_chunk = p.chunk_time;
    if ((st & kCtcxItemCapacity) && !(a.status & kCtcxItemCapacity))
      a.cap_total = (int32_t)(frames + v < 0x7fffffffLL ? frames + v : 0x7fffffffLL);
    a.status |= st;
    p.acc[b] = a;
  }
}

__global__ __launch_bounds__(kNT) void ctcx_stream_commit(CtcxStreamCommitParams p) {
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  char* const dst = p.committed + b * p.stride;
  const char* const src = p.written + b * p.stride;
  __shared__ int32_t s_bad;
  if (tid == 0) s_bad = p.item[b].pad & ctcx::kItemDeadMask;
  __syncthreads();
  const int32_t bad = s_bad;
  int32_t frames, n_leaves;
  if (bad == 0) {
    // four 16-byte loads in flight per thread, then their stores
    const size_t n16 = (size_t)p.copy_bytes >> 4;
    const u32x4* const s4 = (const u32x4*)src;
    u32x4* const d4 = (u32x4*)dst;
    size_t q = tid;
    for (; q + 3 * kNT < n16; q += 4 * kNT) {
      const u32x4 a0 = s4[q], a1 = s4[q + kNT], a2 = s4[q + 2 * kNT], a3 = s4[q + 3 * kNT];
      d4[q] = a0; d4[q + kNT] = a1; d4[q + 2 * kNT] = a2; d4[q + 3 * kNT] = a3;
    }
    for (; q < n16; q += kNT) d4[q] = s4[q];
    if (tid != 0) return;
    frames = ((const CtcxStreamHdr*)src)->frames;
    n_leaves = p.item[b].n_leaves;
  } else {
    // the item stays at its committed state; its results are that state's
    const CtcxStreamHdr* const h = (const CtcxStreamHdr*)dst;
    const int32_t* const hp = (const int32_t*)(dst + sizeof(CtcxStreamHdr));
    const int64_t* const hl = (const int64_t*)(hp + 2 * p.P);
    for (int q = tid; q < p.P; q += kNT) {
      p.top_pos[b * p.P + q] = hp[q];
      p.top_kind[b * p.P + q] = hp[p.P + q];
      if (p.f64) ((double*)p.log_prob)[b * p.P + q] = *(const double*)(hl + q);
      else ((float*)p.log_prob)[b * p.P + q] = *(const float*)(hl + q);
    }
    if (tid != 0) return;
    ctcx::ItemOut io;
    io.n_leaves = h->n_leaves; io.literal_steps = h->literal_steps; io.dup_frames = h->dup_frames;
    io.why_nonfinite = h->why_nonfinite; io.why_fill = h->why_fill; io.pad = bad; io.records = h->records;
    p.item[b] = io;
    frames = h->frames;
    n_leaves = h->n_leaves;
    p.cum[b] = frames;
  }
  // (ctcx_pack_dense's rule, which writes the same word where the push has outputs)
  int32_t st = p.pre[b];
  if (bad != 0) st |= ctcx::kItemHelperTimeout;
  if (p.few_leaves && !(st & (ctcx::kItemLength | ctcx::kItemTable)) && n_leaves < p.P) st |= ctcx::kItemFewLeaves;
  if (st & ~p.pre[b]) p.acc[b].status |= st;
  p.status_ws[b] = st;
  if (p.status) p.status[b] = st;
  if (p.frames) p.frames[b] = frames;
}

}  // namespace

hipError_t ctcx_launch_stream_prologue(const CtcxStreamPrologueParams& p, hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(ctcx_stream_prologue, dim3((unsigned)((p.B + kNT - 1) / kNT)), dim3(kNT), 0, s, p);
  return hipGetLastError();
}

hipError_t ctcx_launch_stream_commit(const CtcxStreamCommitParams& p, hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  if (p.B > 0x7fffffffLL || (p.copy_bytes & 15) || p.copy_bytes > p.stride || p.copy_bytes < (int64_t)sizeof(CtcxStreamHdr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_stream_commit, dim3((unsigned)p.B), dim3(kNT), 0, s, p);
  return hipGetLastError();
}
