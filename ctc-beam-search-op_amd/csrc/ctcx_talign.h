// ctcx_talign.h — shared declarations between the target-alignments kernel
// (ctcx_talign.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Target alignments".  The segments and the LDS tile are
// those of the target scores (ctcx_targets.h); the decode objects do not depend
// on this header.
#pragma once

#include "ctcx_targets.h"

// Frames per decision word: a lane makes three decision bits a frame (one for
// its blank state, two for its label state) and stores one 32-bit word per
// kTalignWordFrames frames.
constexpr int kTalignWordFrames = 10;
static_assert(3 * kTalignWordFrames <= 32, "a word holds the frames' decision bits");

// Words per thread of one workgroup, and the bytes of the decision workspace:
// bp[workgroup][frame / kTalignWordFrames][thread].  -1: no segment holds L, or
// a negative argument.
constexpr int64_t ctcx_talign_words(int64_t Tmax) { return (Tmax + kTalignWordFrames - 1) / kTalignWordFrames; }
constexpr int64_t ctcx_talign_bytes(int64_t B, int64_t N, int64_t L, int64_t Tmax) {
  const int G = ctcx_targets_segment(L);
  if (!G || B < 0 || N < 0 || Tmax < 0) return -1;
  const int64_t per = kTargetsThreads / G;
  return B * ((N + per - 1) / per) * ctcx_talign_words(Tmax) * kTargetsThreads * 4;
}

struct CtcxTalignParams {
  CtcxTargetsParams t;     // the targets and the logits, as the target scores read them; t.out is logp [B][N]
  uint32_t* bp;            // the decision words, ctcx_talign_bytes(B, N, L, Tmax) bytes
  int32_t* start;          // [B][N][L]
  int32_t* end;            // [B][N][L]
  int32_t* trailing_blank; // [B][N]
  void* logp_sum;          // [B][N][L] of the compute dtype, or null
  void* logp_min;          // [B][N][L] of the compute dtype, or null
  int32_t* alignment;      // [B][N][Tmax], or null
};

hipError_t ctcx_launch_target_align(const CtcxTalignParams& p, hipStream_t s);
