"""The register-resident replay of std::sort (csrc/ctcx_regsort.h) that the
one-node float decode kernels run for a frame whose Extract() is std::sort,
instantiated on the host over a 2 x 64 "lane" array and compared with
libstdc++'s std::sort under the same comparator (tot[a] > tot[b] on slots).

The host array gives the header's lane primitives their literal meaning (a
mask per 64-lane register; the final placement by key and equal keys below,
which stands in for the two insertion sorts); the introsort loop -- scans on
masks, median-of-3, unguarded partition, threshold 16, depth limit -- is the
text the kernel compiles.  The full slot order
is compared, ties included, for every length 1..128 and the input families
below; keys are computed as in the kernel (the number of strictly greater
totals), so -inf totals and equal totals go through the same packing.

The depth limit: an input built by McIlroy's adversary against std::sort
itself (length 128) must make rs_sort give up, and the fall-back (the source
array sorted the literal way, here std::sort) must give std::sort's result.

The programme is built twice, plain and with -fsanitize=address,undefined.
"""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ctc-beam-search-op_amd", "csrc")

SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ctcx_regsort.h"

struct HostLanes {
  unsigned r[2][64], aux[64];
  unsigned get(int p) const { return r[p >> 6][p & 63]; }
  void set(int p, unsigned v) { r[p >> 6][p & 63] = v; }
  uint64_t below(int reg, unsigned x) const {
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)(r[reg][l] < x) << l;
    return m;
  }
  uint64_t above(int reg, unsigned x) const {
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)(r[reg][l] > x) << l;
    return m;
  }
  // every "lane" places its own two positions: the key, plus the equal keys below
  int out[128];
  void finish(int n) {
    for (int p = 0; p < n; ++p) {
      const unsigned key = get(p) >> 16;
      unsigned c = 0;
      for (int q = 0; q < p; ++q) c += (get(q) >> 16) == key;
      out[key + c] = (int)(get(p) & 0xFFFFu);
    }
  }
  unsigned aux_get(int i) const { return aux[i]; }
  void aux_set(int i, unsigned v) { aux[i] = v; }
};

static const float NINF = -std::numeric_limits<float>::infinity();
static long g_cases = 0, g_bad = 0, g_fallbacks = 0;

// totals by position; slots are a permutation of ids below 3 * 128
static bool run(const std::vector<float>& t, std::mt19937& g, const char* what) {
  const int n = (int)t.size();
  std::vector<int> ids(384);
  for (int i = 0; i < 384; ++i) ids[i] = i;
  std::shuffle(ids.begin(), ids.end(), g);
  std::vector<float> tot(384, 0.f);
  std::vector<int> e(n);
  for (int p = 0; p < n; ++p) { e[p] = ids[p]; tot[e[p]] = t[p]; }
  std::vector<int> want = e;
  std::sort(want.begin(), want.end(), [&](int a, int b) { return tot[a] > tot[b]; });
  static HostLanes l;
  for (int p = 0; p < 128; ++p) l.out[p] = -1;
  for (int p = 0; p < 128; ++p) {
    unsigned w = 0xFFFFFFFFu;
    if (p < n) {
      unsigned key = 0;
      for (int j = 0; j < n; ++j) key += tot[e[j]] > tot[e[p]];
      w = key << 16 | (unsigned)e[p];
    }
    l.set(p, w);
  }
  std::vector<int> got(n);
  bool fell = false;
  if (ctcx::rs_sort(l, n)) {
    for (int p = 0; p < n; ++p) got[p] = l.out[p];
  } else {   // the kernel's fall-back: the untouched source, the literal way
    fell = true;
    ++g_fallbacks;
    got = e;
    std::sort(got.begin(), got.end(), [&](int a, int b) { return tot[a] > tot[b]; });
  }
  ++g_cases;
  if (got != want) {
    if (g_bad < 8) std::printf("mismatch: %s n %d\n", what, n);
    ++g_bad;
  }
  return fell;
}

// McIlroy's adversary ("A killer adversary for quicksort", 1999) against
// std::sort: values are decided while the sort compares them
static std::vector<int> adv_val;
static int adv_solid, adv_cand, adv_gas;
static bool adv_lt(int x, int y) {
  if (adv_val[x] == adv_gas && adv_val[y] == adv_gas) adv_val[x == adv_cand ? x : y] = adv_solid++;
  if (adv_val[x] == adv_gas) adv_cand = x;
  else if (adv_val[y] == adv_gas) adv_cand = y;
  return adv_val[x] < adv_val[y];
}
static std::vector<float> killer(int n) {
  adv_val.assign(n, n);
  adv_gas = n;
  adv_solid = adv_cand = 0;
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), adv_lt);
  std::vector<float> t(n);
  // gt(a, b) = tot[a] > tot[b] must decide as adv_lt did: negate
  for (int i = 0; i < n; ++i) t[i] = -(float)adv_val[i];
  return t;
}

int main() {
  std::mt19937 g(7);
  std::normal_distribution<float> nd;
  for (int n = 1; n <= 128; ++n) {
    std::vector<float> t(n);
    // descending, and with the minimum swapped to the front (BOTTOM_KNOWN)
    for (int i = 0; i < n; ++i) t[i] = -(float)i * 0.25f;
    run(t, g, "descending");
    std::swap(t[0], t[n - 1]);
    run(t, g, "front-swap");
    // the same over sorted random draws
    for (int rep = 0; rep < 2; ++rep) {
      for (auto& x : t) x = nd(g);
      std::sort(t.begin(), t.end(), std::greater<float>());
      std::swap(t[0], t[n - 1]);
      run(t, g, "front-swap, random draws");
    }
    for (int rep = 0; rep < 6; ++rep) {
      for (auto& x : t) x = nd(g);
      run(t, g, "random");
    }
    for (auto& x : t) x = 1.5f;
    run(t, g, "all-equal");
    const int nds[3] = {2, 4, n / 2 > 0 ? n / 2 : 1};
    for (int q = 0; q < 3; ++q)
      for (int rep = 0; rep < 3; ++rep) {
        for (auto& x : t) x = 0.5f * (float)(g() % nds[q]);
        if (rep == 1) std::sort(t.begin(), t.end(), std::greater<float>());
        if (rep == 1) std::swap(t[0], t[n - 1]);
        run(t, g, "tie-heavy");
      }
    // twin pairs at ranks 0/1 and n-2/n-1: sorted, front-swapped, shuffled
    if (n >= 4)
      for (int rep = 0; rep < 4; ++rep) {
        for (int i = 0; i < n; ++i) t[i] = -(float)i;
        t[1] = t[0];
        t[n - 2] = t[n - 1];
        if (rep == 1) std::swap(t[0], t[n - 1]);
        if (rep >= 2) std::shuffle(t.begin(), t.end(), g);
        run(t, g, "twins");
      }
    // -inf totals: one, several (ties among them), all
    for (int rep = 0; rep < 4; ++rep) {
      for (auto& x : t) x = nd(g);
      const int k = rep == 0 ? 1 : rep == 3 ? n : 1 + (int)(g() % n);
      for (int i = 0; i < k; ++i) t[g() % n] = NINF;
      if (rep == 3) for (auto& x : t) x = NINF;
      if (rep == 2) { std::sort(t.begin(), t.end(), std::greater<float>()); std::swap(t[0], t[n - 1]); }
      run(t, g, "-inf");
    }
  }
  const long before = g_fallbacks;
  const bool fell = run(killer(128), g, "killer");
  std::printf("cases %ld bad %ld fallbacks %ld (before the killer: %ld) killer_fell %d\n", g_cases, g_bad,
              g_fallbacks, before, (int)fell);
  return g_bad || !fell ? 1 : 0;
}
"""


@pytest.mark.parametrize("san", [False, True])
def test_register_sort_matches_std_sort(tmp_path, san):
    src = tmp_path / "reg_sort_model.cpp"
    src.write_text(SRC)
    exe = tmp_path / "reg_sort_model"
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC] + flags + [str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 3000 and int(last[3]) == 0 and int(last[-1]) == 1, r.stdout
