// ctcx_skip_row.cpp — ctcext_skip_plan_row and ctcext_skip_expand_row
// (include/ctcext.h, "Blank-frame skipping"): the definition for one row, on
// the host, frame by frame.  Plain C++, no HIP: it is the yardstick the kernels
// (ctcx_skip.hip) are held to, and shares no code with them.
#include <stdint.h>

#include "../../include/ctcext.h"

template <typename T>
static int64_t plan_row(const T* lp, int64_t n, T thr, int32_t* kmap) {
  int64_t kept = 0;
  bool prev = false;   // the frame before t was blank-dominant
  for (int64_t t = 0; t < n; ++t) {
    const bool dom = lp[t] > thr;   // (false for NaN)
    if (!(t > 0 && dom && prev)) kmap[kept++] = (int32_t)t;
    prev = dom;
  }
  return kept;
}

extern "C" int ctcext_skip_plan_row(const void* logp_blank, int32_t f64, int64_t n, double thr, int32_t* kmap,
                                    int64_t* kept) {
  if (n < 0 || n > INT32_MAX || !kept || (n > 0 && (!logp_blank || !kmap)) || !(thr <= 0))
    return CTCEXT_INVALID_ARGUMENT;
  *kept = f64 ? plan_row((const double*)logp_blank, n, thr, kmap)
              : plan_row((const float*)logp_blank, n, (float)thr, kmap);
  return CTCEXT_OK;
}

// The chunked plan (ctcext.h, "Streaming: blank-frame skipping"): frames
// first_frame .. first_frame + n - 1 of an item, given the flag of the frame
// before them.  Frame by frame, like plan_row, on the absolute frame number.
template <typename T>
static int64_t plan_chunk_row(const T* lp, int64_t n, T thr, int64_t first, bool prev, int32_t* kmap, bool* last) {
  int64_t kept = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool dom = lp[i] > thr;   // (false for NaN)
    if (!(first + i > 0 && dom && prev)) kmap[kept++] = (int32_t)(first + i);
    prev = dom;
  }
  *last = prev;
  return kept;
}

extern "C" int ctcext_skip_plan_chunk_row(const void* logp_blank, int32_t f64, int64_t n, double thr,
                                          int64_t first_frame, int32_t prev_dom, int32_t* kmap, int64_t* kept,
                                          int32_t* last_dom) {
  if (n < 0 || first_frame < 0 || first_frame > INT32_MAX - n || !kept || !last_dom ||
      (n > 0 && (!logp_blank || !kmap)) || !(thr <= 0))
    return CTCEXT_INVALID_ARGUMENT;
  bool last = prev_dom != 0;
  *kept = f64 ? plan_chunk_row((const double*)logp_blank, n, thr, first_frame, last, kmap, &last)
              : plan_chunk_row((const float*)logp_blank, n, (float)thr, first_frame, last, kmap, &last);
  *last_dom = last ? 1 : 0;
  return CTCEXT_OK;
}

extern "C" int ctcext_skip_expand_row(const int64_t* ali_c, int64_t L, const int32_t* kmap, int64_t kept, int64_t n,
                                      int64_t blank_label, int64_t* row, int64_t* row_len) {
  if (L < 0 || kept < 0 || n < 0 || L > kept || kept > n || !row_len || (L > 0 && (!ali_c || !kmap || !row)))
    return CTCEXT_INVALID_ARGUMENT;
  *row_len = 0;
  if (L == 0) return CTCEXT_OK;
  const int32_t* k = kmap + (kept - L);   // the frames the row covers
  for (int64_t i = 0; i < L; ++i)
    if (k[i] < 0 || k[i] >= n || (i > 0 && k[i] <= k[i - 1])) return CTCEXT_INVALID_ARGUMENT;
  const int64_t first = k[0], len = n - first;
  for (int64_t i = 0; i < len; ++i) row[i] = blank_label;
  for (int64_t i = 0; i < L; ++i) row[k[i] - first] = ali_c[i];
  *row_len = len;
  return CTCEXT_OK;
}
