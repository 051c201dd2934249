// ctcx_times_row.cpp — ctcext_token_times_row (include/ctcext.h, "Token
// times"): the definition for one row, on the host, in label order.  Plain
// C++, no HIP: it is the yardstick the kernel (ctcx_times.hip) is held to, and
// shares no code with it.
#include <stdint.h>

#include <vector>

#include "../../include/ctcext.h"

extern "C" int ctcext_token_times_row(const int64_t* decoded, int64_t m, const int64_t* alignment, int64_t L,
                                      int64_t frames, int64_t blank_label, int32_t merge_repeated, int32_t* start,
                                      int32_t* end, int32_t* trailing_blank) {
  if (m < 0 || L < 0 || (m > 0 && !decoded) || (L > 0 && !alignment) || ((start == nullptr) != (end == nullptr)))
    return CTCEXT_INVALID_ARGUMENT;
  struct Run {
    int64_t label, first, last;
  };
  std::vector<Run> runs;
  const int64_t base = frames - L;
  for (int64_t i = 0; i < L;) {
    int64_t j = i;
    while (j + 1 < L && alignment[j + 1] == alignment[i]) ++j;
    if (alignment[i] != blank_label) runs.push_back(Run{alignment[i], base + i, base + j});
    i = j + 1;
  }
  if (trailing_blank) {
    int64_t t = 0;
    while (t < L && alignment[L - 1 - t] == blank_label) ++t;
    *trailing_blank = (int32_t)t;
  }
  if (!start) return CTCEXT_OK;
  for (int64_t q = 0; q < m; ++q) start[q] = end[q] = -1;
  int64_t j = m - 1;
  bool opened = false;
  for (size_t r = runs.size(); r-- > 0;) {
    const Run& u = runs[r];
    if (j < 0) break;
    if (opened && merge_repeated && u.label == decoded[j]) {   // an earlier run of the same merged token
      start[j] = (int32_t)u.first;
      continue;
    }
    if (opened) {
      --j;
      opened = false;
    }
    if (j < 0 || u.label != decoded[j]) break;   // first mismatch: every earlier token stays -1
    start[j] = (int32_t)u.first;
    end[j] = (int32_t)u.last;
    opened = true;
  }
  return CTCEXT_OK;
}
