// ctcx_scores_row.cpp — ctcext_token_scores_row (include/ctcext.h, "Token
// scores"): the definition for one row, on the host, token by token.  Plain
// C++, no HIP: it is the yardstick the kernel (ctcx_scores.hip) is held to, and
// shares no code with it.
#include <stdint.h>

#include <limits>

#include "../../include/ctcext.h"

namespace {

template <typename F>
void scores_row(const F* x, const F* norm, int64_t frames, int64_t C, const int64_t* ali, int64_t L,
                const int32_t* start, const int32_t* end, int64_t m, int64_t blank_index, int64_t blank_label,
                F* lsum, F* lmin) {
  const F nan = std::numeric_limits<F>::quiet_NaN();
  const int64_t base = frames - L;
  for (int64_t i = 0; i < m; ++i) {
    F acc = nan, mn = nan;
    const int64_t s = start[i], e = end[i];
    // (an untimed token is -1; anything else outside the walk is refused the same way)
    bool scored = s >= 0 && s >= base && s <= e && e < frames;
    for (int64_t f = s; scored && f <= e; ++f) {   // ascending frames, every frame of the span
      const int64_t v = ali[f - base];
      const int64_t c = v == blank_label ? blank_index : v;
      if (c < 0 || c >= C) {
        scored = false;
        break;
      }
      const F lp = x[f * C + c] - norm[f];   // one rounded subtraction
      if (f == s) {
        acc = mn = lp;
      } else {
        acc = acc + lp;         // one rounded add, this order (nothing here can contract)
        if (lp < mn) mn = lp;   // a NaN never replaces, a leading NaN stays
      }
    }
    if (!scored) acc = mn = nan;
    if (lsum) lsum[i] = acc;
    if (lmin) lmin[i] = mn;
  }
}

}  // namespace

extern "C" int ctcext_token_scores_row(const void* x, const void* norm, int32_t f64, int64_t frames,
                                       int64_t num_classes, const int64_t* alignment, int64_t L, const int32_t* start,
                                       const int32_t* end, int64_t m, int32_t blank_index, int64_t blank_label,
                                       void* logp_sum, void* logp_min) {
  if (frames < 0 || num_classes <= 0 || L < 0 || L > frames || m < 0 || blank_index < 0 ||
      blank_index >= num_classes || (frames > 0 && (!x || !norm)) || (L > 0 && !alignment) ||
      (m > 0 && (!start || !end)) || (!logp_sum && !logp_min))
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    scores_row<double>((const double*)x, (const double*)norm, frames, num_classes, alignment, L, start, end, m,
                       blank_index, blank_label, (double*)logp_sum, (double*)logp_min);
  else
    scores_row<float>((const float*)x, (const float*)norm, frames, num_classes, alignment, L, start, end, m,
                      blank_index, blank_label, (float*)logp_sum, (float*)logp_min);
  return CTCEXT_OK;
}
