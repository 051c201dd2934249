// Stand-in for tensorflow/core/lib/gtl/top_n.h (TensorFlow 1.14 to 2.1, the
// releases the reference builds against): the members the reference decoder
// calls, written from TopN's published algorithm.  TensorFlow's source is not
// part of this project, so this file and BoundedTop of ../ctc_oracle.cpp are
// the same reading of it: a reference build pins everything in the decoder
// EXCEPT these rules.
//
//   * elements live in one vector; size() is min(elements, limit);
//   * UNORDERED: push appends.  peek_bottom scans for the least element (the
//     last of equals wins the scan), swaps it to the front -> BOTTOM_KNOWN;
//   * BOTTOM_KNOWN: push appends, then swaps the new element to the front
//     unless it is greater than the front;
//   * the push that makes limit + 1 elements runs make_heap and pop_heap ->
//     HEAP_SORTED, where the last slot is spare: a push greater than the front
//     is written there and pop_heap'ed in, any other is dropped;
//   * Extract: std::sort of the vector, or (HEAP_SORTED) sort_heap of all but
//     the spare slot.  The caller owns the result and calls Reset.
// Which of several equal elements ends up where is decided by libstdc++'s
// make_heap / pop_heap / sort_heap / sort, so those are called, not restated.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace tensorflow {
namespace gtl {

template <class T, class Cmp>
class TopN {
 public:
  typedef typename std::vector<T>::const_iterator UnsortedIterator;

  explicit TopN(size_t limit) : limit_(limit) {}

  size_t size() const { return std::min(elements_.size(), limit_); }
  bool empty() const { return size() == 0; }

  void push(const T& v) {
    if (limit_ == 0) return;
    if (state_ != HEAP_SORTED) {
      elements_.push_back(v);
      if (state_ == BOTTOM_KNOWN && !cmp_(elements_.back(), elements_.front())) {
        std::swap(elements_.front(), elements_.back());
      }
      if (elements_.size() == limit_ + 1) {
        std::make_heap(elements_.begin(), elements_.end(), cmp_);
        std::pop_heap(elements_.begin(), elements_.end(), cmp_);
        state_ = HEAP_SORTED;
      }
    } else if (cmp_(v, elements_.front())) {
      elements_.back() = v;
      std::pop_heap(elements_.begin(), elements_.end(), cmp_);
    }
  }

  const T& peek_bottom() {
    if (state_ == UNORDERED) {
      size_t least = 0;
      for (size_t i = 1; i < elements_.size(); ++i) {
        if (cmp_(elements_[least], elements_[i])) least = i;
      }
      if (least != 0) std::swap(elements_[0], elements_[least]);
      state_ = BOTTOM_KNOWN;
    }
    return elements_.front();
  }

  std::vector<T>* Extract() {
    std::vector<T>* out = new std::vector<T>;
    out->swap(elements_);
    if (state_ != HEAP_SORTED) {
      std::sort(out->begin(), out->end(), cmp_);
    } else {
      out->pop_back();
      std::sort_heap(out->begin(), out->end(), cmp_);
    }
    return out;
  }

  void Reset() {
    elements_.clear();
    state_ = UNORDERED;
  }

  UnsortedIterator unsorted_begin() const { return elements_.begin(); }
  UnsortedIterator unsorted_end() const { return elements_.begin() + size(); }

 private:
  enum State { UNORDERED, BOTTOM_KNOWN, HEAP_SORTED };
  State state_ = UNORDERED;
  std::vector<T> elements_;
  size_t limit_;
  Cmp cmp_;
};

}  // namespace gtl
}  // namespace tensorflow
