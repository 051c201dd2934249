// ctcx_regsort.h — libstdc++'s std::sort (ctcx_topn.h lit_sort: the same
// introsort, step for step) over an array of at most 128 elements that lives
// in two wave registers instead of LDS, for the frames whose Extract() is
// std::sort (a beam no push changed, or one that is not full yet).
//
// Elements are packed words (key << 16) | slot, where key is the number of
// elements whose total is strictly greater: for totals without NaN,
// tot[a] > tot[b] <=> key[a] < key[b], equal totals share a key, and every
// comparison of the sort becomes an integer compare on the key field.
//
// The introsort loop (median-of-3 into `first`, the unguarded partition,
// threshold 16, depth limit 2 floor(log2 n)) is replayed step for step: it
// decides where equal elements end up.  Its scans -- `while (gt(e[first],
// pivot)) ++first` and the `--last` scan -- compare every position with one
// value, so each is one compare per register and a find-first / find-last on
// the mask (the comparisons have no side effects, so their order inside a
// scan does not matter); every swap is the literal algorithm's.
//
// The final insertion sort is not replayed.  __insertion_sort and
// __unguarded_linear_insert move an element left only past elements it is
// strictly greater than, so they never reorder equal elements: their result
// is the stable sort of the array the loop left behind.  An element's final
// position is therefore the number of elements with a smaller key -- the key
// itself -- plus the number of equal keys at lower positions, which every
// lane counts for its own two positions at once (L::finish).
//
// The functions are generic over the lane array L (position p: lane p & 63 of
// register p >> 6; positions at and past n hold 0xFFFFFFFF):
//   unsigned get(int p), void set(int p, unsigned v)
//   uint64_t below(int reg, unsigned x)   lanes of register reg with e < x
//   uint64_t above(int reg, unsigned x)   lanes of register reg with e > x
//   unsigned aux_get(int i), void aux_set(int i, unsigned v)   a spare register's lanes
//   void finish(int n)                    the stable placement above, into the result
// The decode kernel instantiates them over VGPRs (readlane / writelane /
// ballot, uniform control flow), tests/test_cpu_reg_sort.py over a 2 x 64
// host array.
//
// The depth limit: lit_sort turns to make_heap + sort_heap on that sub-range.
// rs_sort does not; it returns false with nothing placed, and the caller,
// whose source array is untouched, runs lit_sort instead.
#pragma once

#include <stdint.h>

#ifndef CTCX_RS_FN
#if defined(__HIPCC__)
#define CTCX_RS_FN __host__ __device__ __forceinline__
#else
#define CTCX_RS_FN inline
#endif
#endif

namespace ctcx {

CTCX_RS_FN bool rs_gt(unsigned a, unsigned b) { return (a >> 16) < (b >> 16); }

// the first position p >= first with !gt(e[p], pv) (128: none)
template <class L>
CTCX_RS_FN int rs_scan_up(L& l, int first, unsigned pv) {
  const unsigned x = pv & 0xFFFF0000u;   // gt(e, pv) <=> e < x
  int k = first >> 6;
  uint64_t m = ~l.below(k, x) & (~0ull << (first & 63));
  if (m == 0 && k == 0) {
    k = 1;
    m = ~l.below(1, x);
  }
  return m ? 64 * k + __builtin_ctzll(m) : 128;
}

// the last position p <= last with !gt(pv, e[p]) (-1: none)
template <class L>
CTCX_RS_FN int rs_scan_down(L& l, int last, unsigned pv) {
  if (last < 0) return -1;
  const unsigned y = pv | 0xFFFFu;   // gt(pv, e) <=> e > y
  int k = last >> 6;
  uint64_t m = ~l.above(k, y) & (~0ull >> (63 - (last & 63)));
  if (m == 0 && k == 1) {
    k = 0;
    m = ~l.above(0, y);
  }
  return m ? 64 * k + 63 - __builtin_clzll(m) : -1;
}

template <class L>
CTCX_RS_FN void rs_move_median_to_first(L& l, int result, int a, int b, int c) {
  const unsigned ea = l.get(a), eb = l.get(b), ec = l.get(c);
  int pick;
  unsigned ep;
  if (rs_gt(ea, eb)) {
    if (rs_gt(eb, ec)) { pick = b; ep = eb; }
    else if (rs_gt(ea, ec)) { pick = c; ep = ec; }
    else { pick = a; ep = ea; }
  } else if (rs_gt(ea, ec)) { pick = a; ep = ea; }
  else if (rs_gt(eb, ec)) { pick = c; ep = ec; }
  else { pick = b; ep = eb; }
  const unsigned tmp = l.get(result);
  l.set(result, ep);
  l.set(pick, tmp);
}

// (the pivot's position is outside [first, last): its value does not change)
template <class L>
CTCX_RS_FN int rs_unguarded_partition(L& l, int first, int last, int pivot) {
  const unsigned pv = l.get(pivot);
  while (true) {
    first = rs_scan_up(l, first, pv);
    --last;
    last = rs_scan_down(l, last, pv);
    if (!(first < last)) return first;
    const unsigned ef = l.get(first), el = l.get(last);
    l.set(first, el);
    l.set(last, ef);
    ++first;
  }
}

// std::sort over positions [0, n), 1 <= n <= 128.  False: the depth limit
// was reached (nothing is placed).
template <class L>
CTCX_RS_FN bool rs_sort(L& l, int n) {
  const int lg = 31 - __builtin_clz((unsigned)n);
  // the stack of sub-ranges, one per lane of the spare register: first (bits
  // 0-7), last (8-15), depth (16-23); at most 2 lg + 1 <= 15 entries
  int sp = 0;
  if (n > 16) l.aux_set(sp++, (unsigned)n << 8 | (unsigned)(2 * lg) << 16);
  while (sp > 0) {
    const unsigned f = l.aux_get(--sp);
    int first = (int)(f & 0xFFu), last = (int)(f >> 8 & 0xFFu), depth = (int)(f >> 16 & 0xFFu);
    while (last - first > 16) {
      if (depth == 0) return false;
      --depth;
      const int mid = first + (last - first) / 2;
      rs_move_median_to_first(l, first, first + 1, mid, last - 1);
      const int cut = rs_unguarded_partition(l, first + 1, last, first);
      l.aux_set(sp++, (unsigned)cut | (unsigned)last << 8 | (unsigned)depth << 16);
      last = cut;
    }
  }
  l.finish(n);
  return true;
}

}  // namespace ctcx
