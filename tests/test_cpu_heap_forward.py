"""The forwarding rule of the decode kernel's register-resident heap pops
(extract_fwd_f32 in csrc/ctcx_decode.hip), as a host model against libstdc++.

The kernel keeps every lane's child pair P_j = (node 2j+1, node 2j+2) in
registers across TopN operations instead of storing the moved nodes to LDS
and re-reading the pairs after each one (the pairs go back to LDS when the
call ends).  One operation sifts (v, s) from the root; the model below carries
the lane arrays and applies the kernel's rule, lane for lane (its `he` array
is the heap the stores would have produced, kept only to compare):

  * pickR_j = !(R_j > L_j), c_j the min child, gt_j = c_j > v;
  * lane j publishes v where gt_j (and lane 0 always), else c_j: what node j
    holds after the sift if the path reaches it;
  * lane j fetches the published pair of its min child's lane; where the min
    child is not a lane (lanes 32..63, lane 31 on the right) it fetches lane
    0's, v;
  * the stop is the first path node with gt or a min child that is not a
    lane; the path nodes at or above it that have no gt take their min child
    (up), and exactly those lanes put the fetched pair into P on the min
    child's side;
  * a pop takes e[len - 1] out of lane (len - 2) / 2's P and leaves the
    sentinel there.

After every operation the model's heap must equal std::pop_heap's (values and
slots: the layout, ties included) and P must equal the heap's child pairs in
every lane.  Pushes are TopN pushes on a full heap (push_back, pop_heap,
pop_back), pops are sort_heap's.
"""
import subprocess

SRC = r"""
#include <algorithm>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

struct E { float v; int s; };
struct Gt { bool operator()(const E& a, const E& b) const { return a.v > b.v; } };
static const float INF = std::numeric_limits<float>::infinity();

struct Model {
  E he[257];          // by position; [len, 256] hold sentinels (lanes read up to 128)
  E L[64], R[64];     // P: lane j's registered child pair
  void load(const std::vector<E>& e) {
    for (int p = 0; p < 257; ++p) he[p] = p < (int)e.size() ? e[p] : E{INF, -1};
    for (int j = 0; j < 64; ++j) { L[j] = he[2 * j + 1]; R[j] = he[2 * j + 2]; }
  }
  void sift(E x) {
    bool pr[64], gt[64], onp[64];
    E c[64], pub[64], got[64];
    for (int j = 0; j < 64; ++j) {
      pr[j] = !(R[j].v > L[j].v);
      c[j] = pr[j] ? R[j] : L[j];
      gt[j] = c[j].v > x.v;
      pub[j] = (gt[j] || j == 0) ? x : c[j];
    }
    for (int j = 0; j < 64; ++j) {
      const int src = j >= 32 ? 0 : (j == 31 ? (pr[j] ? 0 : 63) : 2 * j + 1 + (int)pr[j]);
      got[j] = pub[src];
    }
    onp[0] = true;
    for (int j = 1; j < 64; ++j) { const int p = (j - 1) / 2; onp[j] = onp[p] && 2 * p + 1 + (int)pr[p] == j; }
    int k = -1;
    for (int j = 0; j < 64 && k < 0; ++j)
      if (onp[j] && (gt[j] || j >= 32 || (j == 31 && pr[j]))) k = j;
    for (int j = 0; j < 64; ++j) {
      const bool live = onp[j] && j <= k, up = live && !gt[j];
      if (up) he[j] = c[j];
      if (j == k) he[gt[j] ? j : 2 * j + 1 + (int)pr[j]] = x;
    }
    for (int j = 0; j < 64; ++j) {
      const bool up = onp[j] && j <= k && !gt[j];
      if (up) (pr[j] ? R[j] : L[j]) = got[j];
    }
  }
  void pop(int len) {   // pop_heap(len) without parking the front (the kernel keeps it in a register)
    const int q = len - 1, l = (q - 1) / 2;
    E& ent = (q & 1) ? L[l] : R[l];
    const E x = ent;
    ent = E{INF, -1};
    he[q] = E{INF, -1};
    sift(x);
  }
  bool same(const std::vector<E>& e, int n) const {
    for (int p = 0; p < n; ++p) if (he[p].v != e[p].v || he[p].s != e[p].s) return false;
    for (int p = n; p <= 128; ++p) if (he[p].s != -1 || he[p].v != INF) return false;
    for (int j = 0; j < 64; ++j)
      if (L[j].v != he[2 * j + 1].v || L[j].s != he[2 * j + 1].s || R[j].v != he[2 * j + 2].v ||
          R[j].s != he[2 * j + 2].s) return false;
    return true;
  }
};

int main() {
  std::mt19937 g(5);
  long arrays = 0, ops = 0, bad = 0;
  static Model m;
  for (int rep = 0; rep < 160; ++rep)
    for (int len = 2; len <= 129; ++len) {
      const int nd = 4 + (int)(g() % 5);          // 4..8 distinct values: ties everywhere
      const int order = rep % 4;                  // random, ascending, descending, random
      std::vector<E> e(len);
      for (auto& x : e) x.v = 0.5f * (float)(g() % nd);
      if (order == 1) std::sort(e.begin(), e.end(), [](const E& a, const E& b) { return a.v < b.v; });
      if (order == 2) std::sort(e.begin(), e.end(), [](const E& a, const E& b) { return a.v > b.v; });
      for (int i = 0; i < len; ++i) e[i].s = i;
      std::make_heap(e.begin(), e.end(), Gt());
      m.load(e);
      ++arrays;
      bool ok = m.same(e, len);
      // TopN pushes on the full heap: the offer replaces the front (any value: the
      // sift does not need it above the front)
      const int npush = 8 + (int)(g() % 40);
      for (int r = 0; r < npush && ok; ++r) {
        const E x{0.5f * (float)(g() % (nd + 2)), 1000 + r};
        e.push_back(x);
        std::pop_heap(e.begin(), e.end(), Gt());
        e.pop_back();
        if (len >= 2 && len <= 128) { m.sift(x); ok = m.same(e, len); ++ops; }
        else { m.load(e); }   // (129: the one-node form pushes over at most 128)
      }
      // sort_heap
      for (int l = len; l > 1 && ok; --l) {
        std::pop_heap(e.begin(), e.begin() + l, Gt());
        m.pop(l);
        ok = m.same(e, l - 1);
        ++ops;
      }
      if (!ok) { if (bad < 5) std::printf("mismatch: rep %d len %d\n", rep, len); ++bad; }
    }
  std::printf("arrays %ld ops %ld bad %ld\n", arrays, ops, bad);
  return bad ? 1 : 0;
}
"""


def test_forwarded_pairs_match_libstdcxx(tmp_path):
    src = tmp_path / "heap_fwd_model.cpp"
    src.write_text(SRC)
    exe = tmp_path / "heap_fwd_model"
    subprocess.check_call(["g++", "-O2", "-std=c++17", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 20000 and int(last[5]) == 0, r.stdout
