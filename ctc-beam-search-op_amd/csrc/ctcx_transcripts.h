// ctcx_transcripts.h — shared declarations between the transcript-alignments
// kernel (ctcx_transcripts.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Transcript alignments".  The parameters are those of the
// target alignments (ctcx_talign.h; `staged` is not read); the decode objects
// do not depend on this header.
#pragma once

#include "ctcx_talign.h"

// One workgroup of kTranscriptThreads threads per target; thread t holds the K
// label pairs [t K, t K + K).  The longest target is one slot short of what the
// widest K holds, because slot m is the final blank.
constexpr int kTranscriptThreads = 256;
constexpr int64_t kTranscriptMaxTarget = 2047, kTranscriptMaxTime = 13000;
// Frames of a forward block: wave w runs block p - w in phase p, one barrier per phase.
constexpr int kTranscriptBlockFrames = 20;

// Label pairs per thread for a call's max_target: the smallest of 1, 2, 4, 8 with 256 K > L; 0: none.
constexpr int ctcx_transcript_block(int64_t L) {
  return L < 0 || L > kTranscriptMaxTarget ? 0 : L < 256 ? 1 : L < 512 ? 2 : L < 1024 ? 4 : 8;
}
// Frames per decision word: a thread makes 3 K bits a frame.
constexpr int ctcx_transcript_word_frames_of(int K) { return 32 / (3 * K); }
static_assert(ctcx_transcript_word_frames_of(1) == 10 && ctcx_transcript_word_frames_of(2) == 5 &&
                  ctcx_transcript_word_frames_of(4) == 2 && ctcx_transcript_word_frames_of(8) == 1,
              "10, 5, 2 and 1 frames per word");
static_assert(kTranscriptBlockFrames % 10 == 0 && kTranscriptBlockFrames % 5 == 0 && kTranscriptBlockFrames % 2 == 0,
              "a block is a multiple of every frames-per-word");
constexpr int ctcx_transcript_word_frames(int64_t L) {
  return ctcx_transcript_block(L) ? ctcx_transcript_word_frames_of(ctcx_transcript_block(L)) : 0;
}
// Words per thread of one target, and the bytes of the decision workspace:
// bp[target][frame / frames_per_word][thread].  -1: no K holds L, or a negative argument.
constexpr int64_t ctcx_transcript_words(int64_t L, int64_t Tmax) {
  return (Tmax + ctcx_transcript_word_frames(L) - 1) / ctcx_transcript_word_frames(L);
}
constexpr int64_t ctcx_transcript_bytes(int64_t B, int64_t N, int64_t L, int64_t Tmax) {
  if (!ctcx_transcript_block(L) || B < 0 || N < 0 || Tmax < 0) return -1;
  return B * N * ctcx_transcript_words(L, Tmax) * kTranscriptThreads * 4;
}

// p.t.L picks K; p.bp holds ctcx_transcript_bytes(B, N, L, Tmax) bytes.
hipError_t ctcx_launch_transcript_align(const CtcxTalignParams& p, hipStream_t s);
