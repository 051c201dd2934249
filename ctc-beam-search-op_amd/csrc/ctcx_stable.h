// ctcx_stable.h — shared declarations between the stable-prefix kernel
// (ctcx_stable.hip) and the C-ABI host layer (ctcext_capi.hip): the query
// "how much of a stream's decoded output is final" (include/ctcext.h,
// ctcext_stream_stable).  Include after ctcx_kernels.h with CTCX_STREAM_HOST
// (or CTCX_STREAM) defined: the kernel reads the committed CtcxStreamHdr.
#pragma once

#include "ctcx_kernels.h"

// Per item, the last answer: every live chain of that query passed through
// record (frames - 1, pos), and every chain of a later query descends from one
// of those, so it passes through it too.  frames == 0: no answer yet.
struct CtcxStableCache {
  int32_t frames;       // stable_frames of the last answer (f + 1)
  int32_t pos;          // k*: the position at frame f all chains sit on
  int32_t count;        // decoded_length of the last answer
  int32_t last_label;   // the newest label on the chain at or below frame f (count > 0; merge_repeated's carry)
};
static_assert(sizeof(CtcxStableCache) == 16, "CtcxStableCache layout");

struct CtcxStableParams {
  const char* state;        // the committed state buffer: item b's CtcxStreamHdr at state + b * stride
  int64_t stride;
  const void* rec;          // [B][Tmax][W] records of rec_fmt
  int64_t Tmax, B;
  int32_t W, rec_fmt, merge, pad;
  CtcxStableCache* cache;   // [B], read and updated
  int32_t* decoded_length;  // [B]
  int64_t* stable_frames;   // [B]
  int64_t* walked;          // [B] record frames the convergence walk read in this call
  uint8_t* flags;           // beams past the LDS variant's limits: [B][2][W] scratch (null otherwise)
};

namespace ctcx {
// link and label of one record of any format, from its first 32-bit word
// (the fields ctcx_traceback's decoded walk reads).
__host__ __device__ inline void rec_link_label(const uint32_t* w, int fmt, uint32_t& link, int& lab) {
  if (fmt == kRecFmt128) {
    link = w[0];
    lab = (int)w[1];
  } else if (fmt == kRecFmt32) {
    link = w[0] & 255u;
    lab = (int)((w[0] >> 8) & 63u);
  } else {
    const Rec r = (Rec)w[0] | ((Rec)w[1] << 32);
    link = rec_link(r);
    lab = rec_label(r);
  }
}
__host__ __device__ inline int rec_fmt_bytes(int fmt) { return fmt == kRecFmt128 ? 16 : fmt == kRecFmt32 ? 4 : 8; }
}  // namespace ctcx

// The LDS variant stages records and keeps the position flags in LDS; a beam
// too wide for either runs the variant that reads records in place and keeps
// its flags in p.flags.
constexpr int kStableBufBytes = 24 * 1024;   // one record segment buffer
constexpr int kStableLdsW = 4096;            // positions of one flag buffer
inline bool ctcx_stable_in_lds(int W, int rec_fmt) {
  return W <= kStableLdsW && (int64_t)W * ctcx::rec_fmt_bytes(rec_fmt) <= kStableBufBytes - 16;
}
hipError_t ctcx_launch_stable(const CtcxStableParams& p, hipStream_t s);
