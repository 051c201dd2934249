"""The stop test of the decode kernel's TopN push loop (heap_events_f32 in
csrc/ctcx_decode.hip), as a host model against the form it replaced and
against libstdc++.

One push sifts the offer (v, s) down from the root of a heap of W elements
(2 <= W <= 128), lane j owning node j and reading its child pair; positions at
and past W hold +inf sentinels.  Per lane: pickR_j = !(R_j > L_j), c_j the min
child, gt_j = c_j > v, BT_j = (pickR ^ req_j) & anc_j (zero iff every ancestor
of node j picks the child toward j: j is on the root's min-child path).  The
stop condition is cnd = gt | lanes 32..63 | (pickR & lane 31): v lands on the
node (gt) or in a min child that is not a lane.  Two node stores per lane
follow: the lanes of `up` take their min child, the stop lane writes v to
itself (gt) or to its min child.

Three forms of (up, stop), which must agree for every mask:

  * scalar (the loop before): onp = (BT == 0); the stop is the lowest lane of
    onp & cnd (path nodes are ancestors of one another, the shallowest is the
    lowest lane); live = onp at or below that lane; up = live & ~gt.
  * per lane: live_j = ((cnd_lo & anc_j) | BT_j) == 0, that is on the path
    with no proper ancestor meeting the stop condition (ancestors of a lane
    are below 32); up = live & ~gt; stop = live & cnd, a single lane, since
    every deeper path node meeting cnd has the stop as a proper ancestor.
  * the kernel's: live_j = ((gt_lo & anc_j) | BT_j) == 0.  cnd's lane-31 term
    is already in BT: the only lane below node 31 is lane 63, its left child,
    and BT_63 is non-zero when lane 31 picks right.  The stop is not formed as
    a mask: a live lane writes v to itself (gt), else to its min child where
    that is not a lane (left child: lanes 32..63; right child: lanes 31..63),
    else to its dummy slot; the lanes that write v anywhere real are the stop.

The masks come from real heaps (every W in 2..128; tie-heavy, all-equal where
pickR is all right, sorted and random values) and, for the mask identities
alone, from random and adversarial pickR / gt words that no heap need
produce.  For the real heaps the array after the stores must equal TopN's own
step on the same array: the offer written to the spare slot behind the heap
and std::pop_heap over W + 1 (libstdc++'s __adjust_heap down the min-child
path followed by its __push_heap of the offer), values and slots, ties
included.  std::pop_heap of the front followed by std::push_heap of the offer
holds the same elements under the same front, though libstdc++ may lay the
ties out differently there; that much is asserted of it too.
"""
import subprocess

SRC = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

struct E { float v; int s; };
struct Gt { bool operator()(const E& a, const E& b) const { return a.v > b.v; } };
static const float INF = std::numeric_limits<float>::infinity();
static uint32_t anc[64], req[64];

static void geometry() {
  for (unsigned j = 0; j < 64; ++j) {
    const unsigned J = j + 1;
    anc[j] = req[j] = 0;
    for (int k = 1; k <= 6; ++k) {
      const unsigned a = J >> k;
      if (!a) continue;
      anc[j] |= 1u << (a - 1);
      req[j] |= ((J >> (k - 1)) & 1u) << (a - 1);
    }
  }
}

struct Masks { uint64_t up, stop; };

static Masks scalar_form(uint64_t pickR, uint64_t gt) {
  uint64_t onp = 0;
  for (int j = 0; j < 64; ++j) if ((((uint32_t)pickR ^ req[j]) & anc[j]) == 0) onp |= 1ull << j;
  const uint64_t cnd = gt | 0xffffffff00000000ull | (pickR & 0x80000000ull);
  const uint64_t cm = onp & cnd;
  const int k = __builtin_ctzll(cm);             // never empty: every path ends in lanes 31..63
  const uint64_t live = onp & ~(k == 63 ? 0ull : (~1ull << k));
  return Masks{live & ~gt, 1ull << k};
}

static Masks lane_form(uint64_t pickR, uint64_t gt) {
  const uint64_t cnd = gt | 0xffffffff00000000ull | (pickR & 0x80000000ull);
  uint64_t live = 0;
  for (int j = 0; j < 64; ++j) {
    const uint32_t bt = ((uint32_t)pickR ^ req[j]) & anc[j];
    if ((((uint32_t)cnd & anc[j]) | bt) == 0) live |= 1ull << j;
  }
  return Masks{live & ~gt, live & cnd};
}

// the kernel's: where each lane writes v (-1: its dummy slot), by position
static Masks kernel_form(uint64_t pickR, uint64_t gt, int land[64]) {
  uint64_t live = 0, stop = 0;
  for (int j = 0; j < 64; ++j) {
    const uint32_t bt = ((uint32_t)pickR ^ req[j]) & anc[j];
    const bool lv = (((uint32_t)gt & anc[j]) | bt) == 0;
    if (lv) live |= 1ull << j;
    const bool pr = (pickR >> j) & 1ull, g = (gt >> j) & 1ull;
    const int alx = j >= 32 ? 2 * j + 1 : -1, arx = j >= 31 ? 2 * j + 2 : -1;
    int a = pr ? arx : alx;
    a = g ? j : a;
    land[j] = lv ? a : -1;
    if (land[j] >= 0) stop |= 1ull << j;
  }
  return Masks{live & ~gt, stop};
}

static long bad = 0, checked = 0;

static bool masks_agree(uint64_t pickR, uint64_t gt) {
  int land[64];
  const Masks a = scalar_form(pickR, gt), b = lane_form(pickR, gt), c = kernel_form(pickR, gt, land);
  ++checked;
  const bool ok = a.up == b.up && a.stop == b.stop && a.up == c.up && a.stop == c.stop &&
                  __builtin_popcountll(b.stop) == 1;
  if (!ok) { if (bad < 5) std::printf("masks differ: pickR %016llx gt %016llx\n", (unsigned long long)pickR, (unsigned long long)gt); ++bad; }
  return ok;
}

// one push on a real heap: the masks from the lanes' child pairs, the stores, against libstdc++
static void push_case(std::vector<E>& e, E x) {
  const int W = (int)e.size();
  E he[130];
  for (int p = 0; p < 130; ++p) he[p] = p < W ? e[p] : E{INF, -1};
  uint64_t pickR = 0, gt = 0;
  E c[64];
  for (int j = 0; j < 64; ++j) {
    const E L = he[2 * j + 1], R = he[2 * j + 2];
    const bool pr = !(R.v > L.v);
    c[j] = pr ? R : L;
    if (pr) pickR |= 1ull << j;
    if (c[j].v > x.v) gt |= 1ull << j;
  }
  if (!masks_agree(pickR, gt)) return;
  int land[64];
  const Masks m = kernel_form(pickR, gt, land);
  E out[130];
  for (int p = 0; p < 130; ++p) out[p] = he[p];
  for (int j = 0; j < 64; ++j) {
    if ((m.up >> j) & 1ull) out[j] = c[j];
    if (land[j] >= 0) out[land[j]] = x;
  }
  // TopN's step: the offer in the spare slot, pop_heap over W + 1
  std::vector<E> t = e;
  t.push_back(x);
  std::pop_heap(t.begin(), t.end(), Gt());
  t.pop_back();
  bool ok = true;
  for (int p = 0; p < W; ++p) ok = ok && out[p].v == t[p].v && out[p].s == t[p].s;
  for (int p = W; p < 130; ++p) ok = ok && out[p].s == -1 && out[p].v == INF;
  // pop_heap of the front, then push_heap of the offer: the same elements under the same front
  std::vector<E> u = e;
  std::pop_heap(u.begin(), u.end(), Gt());
  u.back() = x;
  std::push_heap(u.begin(), u.end(), Gt());
  ok = ok && u[0].v == out[0].v && std::is_heap(out, out + W, Gt());
  std::vector<E> a(out, out + W), b = u;
  auto lt = [](const E& p, const E& q) { return p.v < q.v || (p.v == q.v && p.s < q.s); };
  std::sort(a.begin(), a.end(), lt);
  std::sort(b.begin(), b.end(), lt);
  for (int p = 0; p < W; ++p) ok = ok && a[p].v == b[p].v && a[p].s == b[p].s;
  if (!ok) { if (bad < 5) std::printf("heap differs: W %d\n", W); ++bad; }
  e = t;
}

int main() {
  geometry();
  std::mt19937_64 g(26);
  long pushes = 0;
  for (int W = 2; W <= 128; ++W)
    for (int rep = 0; rep < 24; ++rep) {
      const int kind = rep % 6;   // 0, 1: ties; 2: all equal; 3: ascending; 4: descending; 5: tie-free
      const int nd = 3 + (int)(g() % 6);
      std::vector<E> e(W);
      std::normal_distribution<float> nrm;
      for (auto& x : e) x.v = kind == 2 ? 1.0f : (kind == 5 ? nrm(g) : 0.5f * (float)(g() % nd));
      if (kind == 3) std::sort(e.begin(), e.end(), [](const E& a, const E& b) { return a.v < b.v; });
      if (kind == 4) std::sort(e.begin(), e.end(), [](const E& a, const E& b) { return a.v > b.v; });
      for (int i = 0; i < W; ++i) e[i].s = i;
      std::make_heap(e.begin(), e.end(), Gt());
      for (int r = 0; r < 40; ++r) {
        // any offer: the sift does not need it above the front (all equal: the same value again, or above)
        E x{kind == 2 ? 1.0f + (float)(r % 2) : (kind == 5 ? nrm(g) + 0.02f * r : 0.5f * (float)(g() % (nd + 2))), 1000 + r};
        push_case(e, x);
        ++pushes;
      }
    }
  // mask identities alone: random and adversarial words
  const uint64_t fixed[] = {0ull, ~0ull, 0xffffffffull, 0xffffffff00000000ull, 0x80000000ull, 0x7fffffffull,
                            1ull, 0xaaaaaaaaaaaaaaaaull, 0x5555555555555555ull, 0xfffffffeull, 0x8000000000000000ull};
  for (uint64_t p : fixed)
    for (uint64_t q : fixed) masks_agree(p, q);
  for (int i = 0; i < 200000; ++i) {
    uint64_t p = g(), q = g();
    switch (i % 5) {
      case 1: q &= g() & g(); break;                 // sparse gt: long paths
      case 2: q = 0; break;                          // no gt at all: the path runs to a non-lane leaf
      case 3: p = ~0ull; q &= g() & g() & g(); break;// all ties: every lane picks right
      case 4: p |= 0x80000000ull; q &= ~0x80000000ull & g(); break;
      default: break;
    }
    masks_agree(p, q);
  }
  // the single path through lane 31 and lane 63, both ways
  for (int right = 0; right < 2; ++right) {
    uint64_t p = right ? 0x80000000ull : 0ull;       // lanes 0, 1, 3, 7, 15 pick left, lane 31 left or right
    masks_agree(p, 0ull);
    masks_agree(p, 1ull << 63);
    masks_agree(p, 1ull << 31);
  }
  std::printf("pushes %ld masks %ld bad %ld\n", pushes, checked, bad);
  return bad ? 1 : 0;
}
"""


def test_push_stop_forms_agree_and_match_libstdcxx(tmp_path):
    src = tmp_path / "push_stop_model.cpp"
    src.write_text(SRC)
    exe = tmp_path / "push_stop_model"
    subprocess.check_call(["g++", "-O2", "-std=c++17", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 100000 and int(last[3]) >= 300000 and int(last[5]) == 0, r.stdout
