// ctcx_align_row.cpp — ctcext_path_alignment_row (include/ctcext.h, "Path
// alignments"): the definition for one row, on the host, state by state in the
// compute dtype.  Plain C++, no HIP: it is the yardstick the kernels
// (ctcx_align.hip) are held to, and shares no code with them.  Compiled without
// contraction; every value below is one rounded operation of F.
#include <math.h>
#include <stdint.h>

#include <limits>
#include <vector>

#include "../../include/ctcext.h"

namespace {

template <typename F>
void align_row(const F* x, const F* norm, int64_t frames, int64_t C, const int64_t* y, int64_t m, int64_t blank,
               int64_t blank_label, int64_t* alignment, int64_t* length, F* logp) {
  const F ninf = -std::numeric_limits<F>::infinity();
  *length = 0;
  for (int64_t j = 0; j < m; ++j)
    if (y[j] < 0 || y[j] >= C) {
      *logp = std::numeric_limits<F>::quiet_NaN();
      return;
    }
  if (frames == 0) {
    *logp = m == 0 ? (F)0 : ninf;
    return;
  }
  const int64_t S = 2 * m + 1;
  auto z = [&](int64_t s) { return s % 2 ? y[s / 2] : blank; };
  auto lp = [&](int64_t f, int64_t c) {
    volatile F d = x[f * C + c] - norm[f];   // one rounded subtraction in F
    return (F)d;
  };
  std::vector<F> v(S, ninf), n(S);
  std::vector<uint8_t> dec((size_t)(frames * S), 0);
  v[0] = lp(0, blank);
  if (m > 0) v[1] = lp(0, y[0]);
  for (int64_t f = 1; f < frames; ++f) {
    for (int64_t s = 0; s < S; ++s) {
      F best = v[s];
      uint8_t d = 0;
      if (s >= 1 && v[s - 1] > best) {
        best = v[s - 1];
        d = 1;
      }
      if (s % 2 && s >= 3 && z(s) != z(s - 2) && v[s - 2] > best) {
        best = v[s - 2];
        d = 2;
      }
      volatile F sum = best + lp(f, z(s));
      n[s] = sum;
      dec[(size_t)(f * S + s)] = d;
    }
    v.swap(n);
  }
  int64_t s = S - 1;
  if (m > 0 && v[S - 2] > v[S - 1]) s = S - 2;
  *logp = v[s];
  if (!(*logp > ninf)) return;   // -inf or NaN: unaligned
  for (int64_t f = frames - 1; f >= 0; --f) {
    alignment[f] = s % 2 ? y[s / 2] : blank_label;
    if (f > 0) s -= dec[(size_t)(f * S + s)];
  }
  *length = frames;
}

}  // namespace

extern "C" int ctcext_path_alignment_row(const void* x, const void* norm, int32_t f64, int64_t frames,
                                         int64_t num_classes, const int64_t* decoded, int64_t m, int32_t blank_index,
                                         int64_t blank_label, int64_t* alignment, int64_t* alignment_length,
                                         void* logp) {
  if (frames < 0 || num_classes <= 0 || m < 0 || blank_index < 0 || blank_index >= num_classes ||
      (frames > 0 && (!x || !norm || !alignment)) || (m > 0 && !decoded) || !alignment_length || !logp ||
      (blank_label >= 0 && blank_label < num_classes && blank_label != blank_index))   // (the blank_label rule)
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    align_row<double>((const double*)x, (const double*)norm, frames, num_classes, decoded, m, blank_index, blank_label,
                      alignment, alignment_length, (double*)logp);
  else
    align_row<float>((const float*)x, (const float*)norm, frames, num_classes, decoded, m, blank_index, blank_label,
                     alignment, alignment_length, (float*)logp);
  return CTCEXT_OK;
}
