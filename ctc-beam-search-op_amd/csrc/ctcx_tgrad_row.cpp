// ctcx_tgrad_row.cpp — ctcext_target_grad_row (include/ctcext.h, "Target
// gradients"): the definition for one target, on the host, state by state in
// long double.  Plain C++, no HIP: it is the yardstick the kernel
// (ctcx_tgrad.hip) is held to, and shares no code with it.
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
void grad_row(const F* x, const F* norm, int64_t frames, int64_t C, const int64_t* y, int64_t m, int64_t blank, F* logp,
              F* g) {
  for (int64_t i = 0; i < frames * C; ++i) g[i] = (F)0;
  for (int64_t j = 0; j < m; ++j)
    if (y[j] < 0 || y[j] >= C) {
      *logp = std::numeric_limits<F>::quiet_NaN();
      return;
    }
  if (frames == 0) {
    *logp = m == 0 ? (F)0 : -std::numeric_limits<F>::infinity();
    return;
  }
  const int64_t S = 2 * m + 1;
  auto z = [&](int64_t s) { return s % 2 ? y[s / 2] : blank; };
  auto skip = [&](int64_t s) { return s < S && s % 2 && s >= 3 && z(s) != z(s - 2); };
  auto lp = [&](int64_t f, int64_t c) { return (L)(F)(x[f * C + c] - norm[f]); };   // one rounded subtraction in F
  std::vector<L> a(frames * S, kNinf), bt(frames * S, kNinf);
  a[0] = lp(0, blank);
  if (m > 0) a[1] = lp(0, y[0]);
  for (int64_t f = 1; f < frames; ++f)
    for (int64_t s = 0; s < S; ++s)
      a[f * S + s] = lse(a[(f - 1) * S + s], s >= 1 ? a[(f - 1) * S + s - 1] : kNinf,
                         skip(s) ? a[(f - 1) * S + s - 2] : kNinf) + lp(f, z(s));
  const L* const end = &a[(frames - 1) * S];
  const L total = lse(end[S - 1], m > 0 ? end[S - 2] : kNinf, kNinf);
  *logp = (F)total;
  if (!(fabsl(total) < std::numeric_limits<L>::infinity())) return;   // -inf or NaN: the row adds nothing
  bt[(frames - 1) * S + S - 1] = lp(frames - 1, blank);
  if (m > 0) bt[(frames - 1) * S + S - 2] = lp(frames - 1, y[m - 1]);
  for (int64_t f = frames - 2; f >= 0; --f)
    for (int64_t s = 0; s < S; ++s)
      bt[f * S + s] = lse(bt[(f + 1) * S + s], s + 1 < S ? bt[(f + 1) * S + s + 1] : kNinf,
                          skip(s + 2) ? bt[(f + 1) * S + s + 2] : kNinf) + lp(f, z(s));
  std::vector<L> occ(C);
  for (int64_t f = 0; f < frames; ++f) {
    for (int64_t c = 0; c < C; ++c) occ[c] = 0;
    for (int64_t s = 0; s < S; ++s) {
      const L ab = a[f * S + s] + bt[f * S + s];
      if (ab > kNinf) occ[z(s)] += expl(ab - lp(f, z(s)) - total);   // (alpha + beta of -inf adds exactly 0)
    }
    for (int64_t c = 0; c < C; ++c) g[f * C + c] = (F)(occ[c] - expl(lp(f, c)));
  }
}

}  // namespace

extern "C" int ctcext_target_grad_row(const void* x, const void* norm, int32_t f64, int64_t frames, int64_t num_classes,
                                      const int64_t* target, int64_t m, int32_t blank_index, void* logp, void* grad) {
  if (frames < 0 || num_classes <= 0 || m < 0 || blank_index < 0 || blank_index >= num_classes ||
      (frames > 0 && (!x || !norm || !grad)) || (m > 0 && !target) || !logp)
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    grad_row<double>((const double*)x, (const double*)norm, frames, num_classes, target, m, blank_index, (double*)logp,
                     (double*)grad);
  else
    grad_row<float>((const float*)x, (const float*)norm, frames, num_classes, target, m, blank_index, (float*)logp,
                    (float*)grad);
  return CTCEXT_OK;
}
