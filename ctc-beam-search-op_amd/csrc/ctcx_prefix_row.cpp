// ctcx_prefix_row.cpp — ctcext_prefix_score_row (include/ctcext.h, "Prefix
// scores"): the definition for one prefix, on the host, state by state in long
// double.  Plain C++, no HIP: it is the yardstick the kernels (ctcx_prefix.hip)
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

// a running LSE over the frames: the terms are kept and summed against their maximum at the end
struct Sum {
  std::vector<L> terms;
  void add(L t) { terms.push_back(t); }
  L value() const {
    L m = kNinf, s = 0;
    for (L t : terms) m = t > m ? t : m;
    if (m == kNinf) return kNinf;
    for (L t : terms) s += expl(t - m);
    return m + logl(s);
  }
};

template <typename F>
void prefix_row(const F* x, const F* norm, int64_t frames, int64_t C, const int64_t* g, int64_t m, int64_t blank,
                F* ext) {
  for (int64_t j = 0; j < m; ++j)
    if (g[j] < 0 || g[j] >= C) {
      for (int64_t c = 0; c < C; ++c) ext[c] = std::numeric_limits<F>::quiet_NaN();
      return;
    }
  const F ninf = -std::numeric_limits<F>::infinity();
  if (frames == 0) {
    for (int64_t c = 0; c < C; ++c) ext[c] = c == blank && m == 0 ? (F)0 : ninf;
    return;
  }
  const int64_t S = 2 * m + 1;
  auto z = [&](int64_t s) { return s % 2 ? g[s / 2] : blank; };
  auto lp = [&](int64_t f, int64_t c) { return (L)(F)(x[f * C + c] - norm[f]); };   // one rounded subtraction in F
  std::vector<L> a(S, kNinf), n(S);
  std::vector<Sum> sum(C);
  a[0] = lp(0, blank);
  if (m > 0) a[1] = lp(0, g[0]);
  for (int64_t c = 0; c < C; ++c) sum[c].add(m == 0 ? lp(0, c) : kNinf);   // term_0
  for (int64_t f = 1; f < frames; ++f) {
    const L bl = a[S - 1], nb = m > 0 ? a[S - 2] : kNinf, both = lse(bl, nb, kNinf);   // the tails of frame f - 1
    for (int64_t c = 0; c < C; ++c) sum[c].add((m > 0 && c == g[m - 1] ? bl : both) + lp(f, c));
    for (int64_t s = 0; s < S; ++s) {
      const L one = s >= 1 ? a[s - 1] : kNinf;
      const L two = (s % 2 && s >= 3 && z(s) != z(s - 2)) ? a[s - 2] : kNinf;
      n[s] = lse(a[s], one, two) + lp(f, z(s));
    }
    a.swap(n);
  }
  for (int64_t c = 0; c < C; ++c) ext[c] = (F)sum[c].value();
  ext[blank] = (F)lse(a[S - 1], m > 0 ? a[S - 2] : kNinf, kNinf);   // the end score
}

}  // namespace

extern "C" int ctcext_prefix_score_row(const void* x, const void* norm, int32_t f64, int64_t frames,
                                       int64_t num_classes, const int64_t* prefix, int64_t m, int32_t blank_index,
                                       void* ext) {
  if (frames < 0 || num_classes <= 0 || m < 0 || blank_index < 0 || blank_index >= num_classes ||
      (frames > 0 && (!x || !norm)) || (m > 0 && !prefix) || !ext)
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    prefix_row<double>((const double*)x, (const double*)norm, frames, num_classes, prefix, m, blank_index, (double*)ext);
  else
    prefix_row<float>((const float*)x, (const float*)norm, frames, num_classes, prefix, m, blank_index, (float*)ext);
  return CTCEXT_OK;
}
