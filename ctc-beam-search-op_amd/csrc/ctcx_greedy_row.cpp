// ctcx_greedy_row.cpp — ctcext_greedy_row (include/ctcext.h, "Greedy decode"):
// the definition for one item, on the host, frame by frame in the compute
// dtype.  Plain C++, no HIP: it is the yardstick the kernels (ctcx_greedy.hip)
// are held to, and shares no code with them.  Compiled without contraction;
// every value below is one rounded operation of F.
#include <stdint.h>

#include "../../include/ctcext.h"

namespace {

template <typename F>
void greedy_row(const F* x, const F* norm, int64_t frames, int64_t C, int64_t blank, int64_t blank_label, bool merge,
                int64_t* decoded, int64_t* decoded_length, int64_t* alignment, int64_t* alignment_length, F* logp) {
  int64_t nd = 0, prev_k = -1, prev_lab = -1;   // (-1: none yet; a class index is never negative)
  F total = (F)0;
  for (int64_t f = 0; f < frames; ++f) {
    const F* r = x + f * C;
    F m = r[0];
    int64_t k = 0;
    for (int64_t j = 1; j < C; ++j)
      if (r[j] > m) {   // strict: the lowest index wins a tie; false for a NaN
        m = r[j];
        k = j;
      }
    volatile F lp = m - norm[f];   // one rounded subtraction in F
    volatile F sum = total + lp;   // one rounded add in F
    total = f == 0 ? (F)lp : (F)sum;
    alignment[f] = k == blank ? blank_label : k;
    if (k != blank && k != prev_k) {
      if (!(merge && k == prev_lab)) decoded[nd++] = k;
      prev_lab = k;
    }
    prev_k = k;
  }
  *decoded_length = nd;
  *alignment_length = frames;
  *logp = total;
}

}  // namespace

extern "C" int ctcext_greedy_row(const void* x, const void* norm, int32_t f64, int64_t frames, int64_t num_classes,
                                 int32_t blank_index, int64_t blank_label, int32_t merge_repeated, int64_t* decoded,
                                 int64_t* decoded_length, int64_t* alignment, int64_t* alignment_length, void* logp) {
  if (frames < 0 || num_classes <= 0 || blank_index < 0 || blank_index >= num_classes ||
      (frames > 0 && (!x || !norm || !decoded || !alignment)) || !decoded_length || !alignment_length || !logp)
    return CTCEXT_INVALID_ARGUMENT;
  if (f64)
    greedy_row<double>((const double*)x, (const double*)norm, frames, num_classes, blank_index, blank_label,
                       merge_repeated != 0, decoded, decoded_length, alignment, alignment_length, (double*)logp);
  else
    greedy_row<float>((const float*)x, (const float*)norm, frames, num_classes, blank_index, blank_label,
                      merge_repeated != 0, decoded, decoded_length, alignment, alignment_length, (float*)logp);
  return CTCEXT_OK;
}
