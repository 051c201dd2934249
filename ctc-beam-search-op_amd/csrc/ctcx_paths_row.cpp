// ctcx_paths_row.cpp — ctcext_path_score_row (include/ctcext.h, "Path
// scores"): the definition for one row, on the host, state by state in long
// double.  Plain C++, no HIP: it is the yardstick the kernels (ctcx_paths.hip)
// are held to, and shares no code with them.
#include <math.h>
#include <stdint.h>

#include <limits>
#include <vector>

#include "../../include/ctcext.h"

namespace {

typedef long double L;

const L kNinf = -std::numeric_limits<L>::infinity();

// LSE of up to three terms; all -inf gives -inf, never NaN
L lse(L a, L b, L c) {
  L m = a > b ? a : b;
  if (c > m) m = c;
  if (m == kNinf) return kNinf;
  return m + logl(expl(a - m) + expl(b - m) + expl(c - m));
}

template <typename F>
F score_row(const F* x, const F* norm, int64_t frames, int64_t C, const int64_t* y, int64_t m, int64_t blank) {
  for (int64_t j = 0; j < m; ++j)
    if (y[j] < 0 || y[j] >= C) return std::numeric_limits<F>::quiet_NaN();
  if (frames == 0) return m == 0 ? (F)0 : -std::numeric_limits<F>::infinity();
  const int64_t S = 2 * m + 1;
  auto z = [&](int64_t s) { return s % 2 ? y[s / 2] : blank; };
  auto lp = [&](int64_t f, int64_t c) { return (L)(F)(x[f * C + c] - norm[f]); };   // one rounded subtraction in F
  std::vector<L> a(S, kNinf), n(S);
  a[0] = lp(0, blank);
  if (m > 0) a[1] = lp(0, y[0]);
  for (int64_t f = 1; f < frames; ++f) {
    for (int64_t s = 0; s < S; ++s) {
      const L one = s >= 1 ? a[s - 1] : kNinf;
      const L two = (s % 2 && s >= 3 && z(s) != z(s - 2)) ? a[s - 2] : kNinf;
      n[s] = lse(a[s], one, two) + lp(f, z(s));
    }
    a.swap(n);
  }
  return (F)lse(a[S - 1], S >= 2 ? a[S - 2] : kNinf, kNinf);
}

}  // namespace

extern "C" int ctcext_path_score_row(const void* x, const void* norm, int32_t f64, int64_t frames,
                                     int64_t num_classes, const int64_t* decoded, int64_t m, int32_t blank_index,
                                     int64_t blank_label, void* score) {
  if (frames < 0 || num_classes <= 0 || m < 0 || blank_index < 0 || blank_index >= num_classes ||
      (frames > 0 && (!x || !norm)) || (m > 0 && !decoded) || !score ||
      (blank_label >= 0 && blank_label < num_classes && blank_label != blank_index))   // (the blank_label rule)
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    *(double*)score = score_row<double>((const double*)x, (const double*)norm, frames, num_classes, decoded, m,
                                        blank_index);
  else
    *(float*)score = score_row<float>((const float*)x, (const float*)norm, frames, num_classes, decoded, m,
                                      blank_index);
  return CTCEXT_OK;
}
