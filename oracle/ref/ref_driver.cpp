// ref_driver.cpp — C entry point around the REFERENCE decoder's own headers
// (TEST INFRASTRUCTURE ONLY; built into oracle/_ref/libctc_ref.so by the
// Makefile beside this file, loaded by oracle/reference.py).
//
// The include below is resolved inside the reference tree (-I, never copied);
// the tensorflow/ and third_party/ includes that tree names resolve to the
// stand-in headers of this directory.  This file does what the reference op's
// Compute does between validation and SparseTensor packing (kernels.cc:54-90):
// one decoder with BaseBeamScorer for the whole batch; per item Step for
// seq_len[b] frames, TopPaths, Reset; the first item whose TopPaths fails ends
// the call with that status.  The reference reports a path without alignment
// by printing a line to std::cout; the driver captures std::cout for the call
// and counts those lines.
//
// The scorer hook.  The reference's AddAlignmentCandidate takes BeamEntry<T>*
// (ctc_beam_entry.h), so its decoder compiles only with the default
// EmptyBeamState: a scorer cannot keep its value in the state object.  It can
// keep it beside it.  BeamEntry::state is a member of an entry that BeamRoot
// allocates on the heap, one unique_ptr each, never moves, and frees only when
// Reset() replaces the root; Reset() then calls InitializeState.  So between
// two InitializeState calls the address of a state object names one entry and
// no other, and TableScorer below keys a side table by it: ExpandState stores
// table[(from_label + 1) * C + to_label] under to_state's address (the root's
// label is -1: row 0 is the root's), GetStateExpansionScore adds what is
// stored there to previous_score, InitializeState clears the table.  The
// counters say whether the argument held during a call (no lookup without a
// stored value, no address re-expanded to another value) and that the decoder
// never calls the end hooks.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "ctc_ext_beam_search_decoder.h"

namespace {

// What Step needs of its argument: size(), operator()(int) and maxCoeff().
// maxCoeff is a plain '>' scan: Eigen's result for rows without NaN (callers
// keep NaN out; -inf, also a whole row of it, is fine).
template <class T>
struct RowView {
  const T* data;
  int n;
  int size() const { return n; }
  T operator()(int i) const { return data[i]; }
  T maxCoeff() const {
    T m = data[0];
    for (int i = 1; i < n; ++i) {
      if (data[i] > m) m = data[i];
    }
    return m;
  }
};

struct CoutCapture {
  std::ostringstream text;
  std::streambuf* saved;
  CoutCapture() : saved(std::cout.rdbuf(text.rdbuf())) {}
  ~CoutCapture() { std::cout.rdbuf(saved); }
};

int count_lines(const std::string& text, const std::string& line) {
  int n = 0;
  std::istringstream in(text);
  std::string got;
  while (std::getline(in, got)) n += (got == line);
  return n;
}

// hook_stats[] of ref_decode_scored
enum { kInit = 0, kExpand, kLookup, kLookupNoState, kReexpandDiffers, kEndHook, kHookStats };

template <class T>
class TableScorer : public tensorflow::ctc::BaseBeamScorer<T, tensorflow::ctc::ctc_beam_search::EmptyBeamState> {
 public:
  typedef tensorflow::ctc::ctc_beam_search::EmptyBeamState State;
  TableScorer(const T* table, int64_t C) : table_(table), C_(C) {
    for (int i = 0; i < kHookStats; ++i) n[i] = 0;
  }
  void InitializeState(State* root) const override {
    ++n[kInit];
    cached_.clear();
  }
  void ExpandState(const State& from_state, int from_label, State* to_state, int to_label) const override {
    ++n[kExpand];
    const T v = table_[(int64_t)(from_label + 1) * C_ + to_label];
    auto at = cached_.emplace((const void*)to_state, v);
    if (!at.second && std::memcmp(&at.first->second, &v, sizeof(T)) != 0) {
      ++n[kReexpandDiffers];
      at.first->second = v;
    }
  }
  T GetStateExpansionScore(const State& state, T previous_score) const override {
    ++n[kLookup];
    auto at = cached_.find((const void*)&state);
    if (at == cached_.end()) {
      ++n[kLookupNoState];
      return previous_score;
    }
    return previous_score + at->second;
  }
  void ExpandStateEnd(State* state) const override { ++n[kEndHook]; }
  T GetStateEndExpansionScore(const State& state) const override {
    ++n[kEndHook];
    return T(0);
  }
  mutable int64_t n[kHookStats];

 private:
  const T* table_;
  int64_t C_;
  mutable std::unordered_map<const void*, T> cached_;
};

// copies the counters out on every way out of run()
template <class T>
struct HookReport {
  const TableScorer<T>& scorer;
  int64_t* to;
  ~HookReport() {
    for (int i = 0; to && i < kHookStats; ++i) to[i] = scorer.n[i];
  }
};

}  // namespace

struct RefResult {
  int32_t ok;                // 0: TopPaths failed on item failed_item, see message
  int32_t failed_item;
  int32_t no_label_lines;    // "No label seq available" lines printed during the call
  char message[256];         // the reference Status' error_message()
  int64_t total_dec, total_ali;
  int64_t* dec_len;          // [B*P], b-major
  int64_t* ali_len;
  int32_t* dec_vals;         // concatenated in the same order
  int32_t* ali_vals;
  double* log_prob;          // [B*P]
};

template <class T>
static RefResult* run(const T* x, const int32_t* seq_len, int64_t B, int64_t C, int W, int P,
                      int merge, int blank_index, int blank_label, const T* table = nullptr,
                      int64_t* hook_stats = nullptr) {
  namespace ctc = tensorflow::ctc;
  RefResult* r = new RefResult();
  std::memset(r, 0, sizeof(*r));
  r->ok = 1;
  std::vector<std::vector<int>> dec_all, ali_all;
  std::vector<double> lp_all;
  CoutCapture capture;

  // table == nullptr: the reference op's own scorer, as before there was a table
  typename ctc::CTCExtBeamSearchDecoder<T>::DefaultBeamScorer base;
  TableScorer<T> scored(table, C);
  typename ctc::CTCExtBeamSearchDecoder<T>::DefaultBeamScorer* scorer = &base;
  if (table) scorer = &scored;
  HookReport<T> report{scored, table ? hook_stats : nullptr};
  ctc::CTCExtBeamSearchDecoder<T> decoder((int)C, blank_index, W, scorer, blank_label, 1, merge != 0);
  for (int64_t b = 0; b < B && r->ok; ++b) {
    for (int64_t t = 0; t < seq_len[b]; ++t) {
      RowView<T> row{x + (t * B + b) * C, (int)C};
      decoder.Step(row);
    }
    std::vector<std::vector<int>> paths, aligns;
    std::vector<T> log_probs;
    tensorflow::Status s = decoder.TopPaths(P, &paths, &aligns, &log_probs, merge != 0);
    if (!s.ok()) {
      r->ok = 0;
      r->failed_item = (int32_t)b;
      std::strncpy(r->message, s.error_message().c_str(), sizeof(r->message) - 1);
      break;
    }
    decoder.Reset();
    for (int p = 0; p < P; ++p) {
      dec_all.push_back(paths[p]);
      ali_all.push_back(aligns[p]);
      lp_all.push_back((double)log_probs[p]);
    }
  }
  r->no_label_lines = count_lines(capture.text.str(), "No label seq available");
  if (!r->ok) return r;

  const int64_t n = B * P;
  r->dec_len = new int64_t[n + 1];
  r->ali_len = new int64_t[n + 1];
  r->log_prob = new double[n + 1];
  for (int64_t i = 0; i < n; ++i) {
    r->dec_len[i] = (int64_t)dec_all[i].size();
    r->ali_len[i] = (int64_t)ali_all[i].size();
    r->total_dec += r->dec_len[i];
    r->total_ali += r->ali_len[i];
    r->log_prob[i] = lp_all[i];
  }
  r->dec_vals = new int32_t[r->total_dec + 1];
  r->ali_vals = new int32_t[r->total_ali + 1];
  int64_t od = 0, oa = 0;
  for (int64_t i = 0; i < n; ++i) {
    for (int v : dec_all[i]) r->dec_vals[od++] = v;
    for (int v : ali_all[i]) r->ali_vals[oa++] = v;
  }
  return r;
}

extern "C" {

// dtype 0 = float32, 1 = float64; x is [T, B, C] row-major, seq_len[b] <= T.
// The caller has validated shapes and blank_index as the op does.
RefResult* ref_decode(int dtype, const void* x, const int32_t* seq_len, int64_t B, int64_t C,
                      int W, int P, int merge, int blank_index, int blank_label) {
  if (dtype == 0) return run<float>((const float*)x, seq_len, B, C, W, P, merge, blank_index, blank_label);
  return run<double>((const double*)x, seq_len, B, C, W, P, merge, blank_index, blank_label);
}

// As ref_decode with TableScorer over table [C + 1, C] of the same dtype (row
// from_label + 1, row 0 the root's; see the head of this file).  hook_stats, if
// not null, receives six counts for the whole call: InitializeState calls,
// ExpandState calls, GetStateExpansionScore calls, those of them that found no
// stored value, ExpandState calls that found another value stored under the
// address, and calls of either end hook.
RefResult* ref_decode_scored(int dtype, const void* x, const int32_t* seq_len, int64_t B, int64_t C,
                             int W, int P, int merge, int blank_index, int blank_label,
                             const void* table, int64_t* hook_stats) {
  if (dtype == 0)
    return run<float>((const float*)x, seq_len, B, C, W, P, merge, blank_index, blank_label,
                      (const float*)table, hook_stats);
  return run<double>((const double*)x, seq_len, B, C, W, P, merge, blank_index, blank_label,
                     (const double*)table, hook_stats);
}

void ref_free(RefResult* r) {
  if (!r) return;
  delete[] r->dec_len;
  delete[] r->ali_len;
  delete[] r->dec_vals;
  delete[] r->ali_vals;
  delete[] r->log_prob;
  delete r;
}

}  // extern "C"
