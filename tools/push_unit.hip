// push_unit.hip — GPU unit test and timing of the decode kernel's TopN push
// loop (heap_events_f32, taken from the kernel source as it stands: the stop
// found per lane, CTCX_PUSH_COPIES push bodies per loop trip) against the loop
// it replaced (heap_events_ff1_f32 below: the stop found by a scalar
// first-set-bit chain, one body per trip; kept here as the baseline).
//   * after every call, bit for bit between the two loops: the heap image, the
//     front (fv, fs), nfree, nv, myslot, evr, bat, NC, RB, done, the return
//     value and k (where the call returns 1: k is not written otherwise);
//   * the same against a host replay of the loop's rule with TopN's own heap
//     step (the offer in the spare slot, std::pop_heap over limit + 1);
//   * cases: W of 2, 3, 33, 64, 65, 127 and 128, tie-heavy and tie-free
//     values, evicted branch entries (fs < nb) and re-offering lanes (LB: the
//     loop returns 1 mid-chunk and is entered again);
//   * cycles per push of both loops (s_memtime around a few thousand pushes,
//     no stamp inside), the wave alone on its CU and with a second wave on
//     another SIMD reading LDS (ds_read_b128) all the while.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DCTCX_PART=99 [-DCTCX_PUSH_COPIES=1|2|4] tools/push_unit.hip -o tools/push_unit.bin
// (CTCX_PART=99: no kernel instantiation and no dispatcher, the device functions only)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../ctc-beam-search-op_amd/csrc/ctcx_decode.hip"

using namespace ctcx;

// The loop before the per-lane stop test: one push per trip, the stop the
// lowest lane of the path nodes meeting the stop condition.
__device__ __forceinline__ int heap_events_ff1_f32(float s, int c, int sl, unsigned anc, unsigned req, unsigned aj,
                                                   unsigned al, unsigned ar, unsigned dum, int& myslot, int& evr,
                                                   float& bat, uint64_t& NC, uint64_t& RB, uint64_t& done,
                                                   uint64_t LB, float& fv, int& fs, int& nfree, int& nv, int nb,
                                                   int& k, int& cnt) {
  int st;
  const unsigned k31 = 0x80000000u;
  NC = uni64(NC); RB = uni64(RB); done = uni64(done); LB = uni64(LB);
  fv = uni(fv); fs = uni(fs); nfree = uni(nfree); nv = uni(nv); nb = uni(nb); cnt = uni(cnt);
  asm volatile(
      "s_mov_b32 %[st], 0\n\t"
      "s_mov_b32 s99, -1\n\t"                              // cnd's high word: lanes 32..63 always stop
      "s_not_b64 s[80:81], %[done]\n\t"                    // lanes still to come
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"          // s > front
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"         // m (SCC: m != 0)
      "s_cbranch_scc0 .Lrf_exit_%=\n\t"
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
      "s_cbranch_scc1 .Lrf_rare_%=\n\t"
      "ds_read_b128 v[232:235], %[al]\n"                   // its child pairs (L.v, L.s, R.v, R.s)
      ".Lrf_tail_%=:\n\t"
      "s_lshl_b64 s[80:81], -2, %[k]\n\t"                  // lanes after k
      "v_readlane_b32 s84, %[s], %[k]\n\t"                 // v = offer k's score
      "s_mov_b32 s85, %[fs]\n\t"                           // slot = the front's
      "s_cmp_lt_i32 %[fs], %[nb]\n\t"
      "s_cbranch_scc1 .Lrf_evb_%=\n"
      ".Lrf_slot_%=:\n\t"
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[my]\n\t"
      "s_mov_b32 m0, %[k]\n\t"
      "v_cndmask_b32_e64 %[my], %[my], -1, s[90:91]\n\t"
      "v_writelane_b32 %[my], s85, m0\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cmp_ngt_f32_e64 s[92:93], v234, v232\n\t"         // pickR = !(R > L)
      "v_mov_b64_e32 v[240:241], s[84:85]\n\t"
      "v_cndmask_b32_e64 v237, v232, v234, s[92:93]\n\t"   // cv
      "v_cndmask_b32_e64 v238, v233, v235, s[92:93]\n\t"   // cs
      "v_bitop3_b32 v239, s92, %[req], %[anc] bitop3:0x28\n\t"
      "v_cmp_lt_f32_e64 s[96:97], s84, v237\n\t"           // gt: min child > v
      "v_cndmask_b32_e64 v236, %[al], %[ar], s[92:93]\n\t"
      "v_readfirstlane_b32 s86, v237\n\t"
      "v_cmp_eq_u32_e64 s[94:95], 0, v239\n\t"             // onp
      "v_readfirstlane_b32 s87, v238\n\t"
      "v_cndmask_b32_e64 v236, v236, %[aj], s[96:97]\n\t"
      "s_and_b32 s98, s92, %[k31]\n\t"
      "s_bitcmp1_b32 s96, 0\n\t"
      "s_cselect_b32 %[fv], s84, s86\n\t"
      "s_cselect_b32 %[fs], s85, s87\n\t"
      "s_or_b32 s98, s98, s96\n\t"                         // cnd
      CTCX_BAT_A
      "v_cmp_lt_f32_e64 s[88:89], %[fv], %[s]\n\t"
      "s_and_b64 s[90:91], s[94:95], s[98:99]\n\t"         // cm
      "s_ff1_i32_b64 s86, s[90:91]\n\t"                    // the stop: the shallowest of them
      CTCX_BAT_B
      "s_lshl_b64 s[90:91], -2, s86\n\t"
      "s_andn2_b64 s[94:95], s[94:95], s[90:91]\n\t"       // live
      "s_andn2_b64 s[90:91], s[94:95], s[96:97]\n\t"       // up
      "s_lshl_b64 s[94:95], 1, s86\n\t"                    // the stop
      "v_cndmask_b32_e64 v239, %[dum], %[aj], s[90:91]\n\t"
      "v_cndmask_b32_e64 v236, %[dum], v236, s[94:95]\n\t"
      "ds_write2_b32 v239, v237, v238 offset1:1\n\t"
      "ds_write2_b32 v236, v240, v241 offset1:1\n\t"
      "ds_read_b128 v[232:235], %[al]\n\t"
      CTCX_BAT_C
      "s_and_b64 s[88:89], s[88:89], %[nc]\n\t"
      "s_or_b64 s[88:89], s[88:89], %[rb]\n\t"
      "s_and_b64 s[88:89], s[88:89], s[80:81]\n\t"
      "s_cbranch_scc0 .Lrf_exit_%=\n\t"
      "s_ff1_i32_b64 %[k], s[88:89]\n\t"
      "s_bitcmp1_b64 %[lb], %[k]\n\t"
      "s_cbranch_scc0 .Lrf_tail_%=\n\t"
      "s_branch .Lrf_rare_%=\n"
      ".Lrf_evb_%=:\n\t"
      "s_mov_b32 s85, %[nfree]\n\t"
      "s_add_u32 %[nfree], %[nfree], 1\n\t"
      "s_mov_b32 m0, %[nv]\n\t"
      "s_add_u32 %[nv], %[nv], 1\n\t"
      "v_writelane_b32 %[evr], %[fs], m0\n\t"
      "v_cmp_eq_u32_e64 s[90:91], %[fs], %[c]\n\t"
      "s_and_b64 s[90:91], s[90:91], %[lb]\n\t"
      "s_or_b64 %[rb], %[rb], s[90:91]\n\t"
      "s_branch .Lrf_slot_%=\n"
      ".Lrf_rare_%=:\n\t"
      "s_mov_b32 %[st], 1\n"
      ".Lrf_exit_%=:\n\t"
      "s_not_b64 %[done], s[80:81]\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [my] "+v"(myslot), [evr] "+v"(evr), [bat] "+v"(bat), [nc] "+s"(NC), [rb] "+s"(RB), [done] "+s"(done),
        [fv] "+s"(fv), [fs] "+s"(fs), [nfree] "+s"(nfree), [nv] "+s"(nv), [k] "=&s"(k), [st] "=&s"(st), [cnt] "+s"(cnt)
      : [s] "v"(s), [c] "v"(c), [sl] "v"(sl), [anc] "v"(anc), [req] "v"(req), [aj] "v"(aj), [al] "v"(al),
        [ar] "v"(ar), [dum] "v"(dum), [lb] "s"(LB), [nb] "s"(nb), [k31] "s"(k31)
      : "memory", "vcc", "m0", "s80", "s81", "s84", "s85", "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93",
        "s94", "s95", "s96", "s97", "s98", "s99", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",
        "v240", "v241", "v242", "v243");
  return st;
}

constexpr int kHdum = 130;   // he index of lane 0's dummy slot (positions 0..128, then the dummies)
constexpr float kInf = std::numeric_limits<float>::infinity();

// everything one call reads and writes: the heap by position (sentinels at
// and past the beam's width), the chunk as the scored-chunk loop hands it
// over (s, c, sl per lane; the NC / RB / LB / done lane masks), the uniform state
struct Call {
  float hv[129];
  int hs[129];
  float s[64];
  int c[64], sl[64];
  int my[64], evr[64];
  float bat[64];
  unsigned long long NC, RB, done, LB;
  float fv;
  int fs, nfree, nv, nb, k, st;
};

template <int VAR>
__device__ __forceinline__ int one_call(float s, int c, int sl, const HeapM& geo, unsigned aj, unsigned al,
                                        unsigned ar, unsigned dum, int& my, int& evr, float& bat, uint64_t& NC,
                                        uint64_t& RB, uint64_t& done, uint64_t LB, float& fv, int& fs, int& nfree,
                                        int& nv, int nb, int& k) {
  int cnt = 0;
  if constexpr (VAR == 0)
    return heap_events_ff1_f32(s, c, sl, geo.anc, geo.req, aj, al, ar, dum, my, evr, bat, NC, RB, done, LB, fv, fs,
                               nfree, nv, nb, k, cnt);
  else
    return heap_events_f32(s, c, sl, geo.anc, geo.req, aj, al, ar, dum, my, evr, bat, NC, RB, done, LB, fv, fs,
                           nfree, nv, nb, k, cnt);
}

// one wave, one call
template <int VAR>
__global__ void call_kernel(const Call* in, Call* out) {
  __shared__ __attribute__((aligned(16))) HE<float> lds[kHdum + 64];
  CTCX_LDS HE<float>* he = (CTCX_LDS HE<float>*)lds;
  const int lane = threadIdx.x;
  for (int i = lane; i <= 128; i += 64) he_st(he, i + 1, HE<float>{in->hv[i], in->hs[i]});
  __syncthreads();
  const HeapM geo = heap_m(kHdum);
  const unsigned heb = (unsigned)(uintptr_t)he;
  const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
  const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(kHdum + lane);
  int my = in->my[lane], evr = in->evr[lane];
  float bat = in->bat[lane];
  uint64_t NC = in->NC, RB = in->RB, done = in->done;
  float fv = in->fv;
  int fs = in->fs, nfree = in->nfree, nv = in->nv, k = -1;
  const int st = one_call<VAR>(in->s[lane], in->c[lane], in->sl[lane], geo, aj, al, ar, dum, my, evr, bat, NC, RB,
                               done, in->LB, fv, fs, nfree, nv, in->nb, k);
  __syncthreads();
  for (int i = lane; i <= 128; i += 64) { out->hv[i] = he[i + 1].v; out->hs[i] = he[i + 1].s; }
  out->my[lane] = my; out->evr[lane] = evr; out->bat[lane] = bat;
  if (lane == 0) {
    out->NC = NC; out->RB = RB; out->done = done;
    out->fv = fv; out->fs = fs; out->nfree = nfree; out->nv = nv; out->st = st;
    out->k = st ? k : -1;
  }
}

// timing: wave 0 runs `nchunk` chunks of offers (staged in LDS) through the
// loop on one heap; with `busy`, wave 1 (another SIMD of the CU) reads LDS with
// ds_read_b128 until wave 0 is through (a bounded number of reads at the most)
constexpr int kChunks = 64;
typedef float fx4 __attribute__((ext_vector_type(4)));
template <int VAR>
__global__ void time_kernel(const float* hv, const int* hs, const float* offers, int nchunk, int busy,
                            unsigned long long* cyc, float* out_hv, int* out_hs, int* out_my) {
  __shared__ __attribute__((aligned(16))) HE<float> lds[kHdum + 64];
  __shared__ float off[kChunks * 64];
  __shared__ __attribute__((aligned(16))) float junk[64 * 4];
  __shared__ int flag;
  CTCX_LDS HE<float>* he = (CTCX_LDS HE<float>*)lds;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave == 0) {
    for (int i = lane; i <= 128; i += 64) he_st(he, i + 1, HE<float>{hv[i], hs[i]});
    for (int i = lane; i < nchunk * 64; i += 64) off[i] = offers[i];
    for (int i = lane; i < 256; i += 64) junk[i] = 0.f;
    if (lane == 0) flag = 0;
  }
  __syncthreads();
  if (wave == 1) {
    if (busy) {
      float acc = 0.f;
      volatile int* f = &flag;
      const unsigned ja = (unsigned)(uintptr_t)(CTCX_LDS float*)junk + 16u * (unsigned)lane;
      for (int it = 0; it < (1 << 21) && *f == 0; ++it) {
        fx4 q;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(q) : "v"(ja) : "memory");
        acc += q.x + q.w;
      }
      if (acc == 12345.f) cyc[1] = 1;   // (keeps the reads)
    }
    return;
  }
  if (wave != 0) return;
  const HeapM geo = heap_m(kHdum);
  const unsigned heb = (unsigned)(uintptr_t)he;
  const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
  const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(kHdum + lane);
  float fv = uni(he_ld(he, 1).v);
  int fs = uni(he_ld(he, 1).s);
  int nfree = 100000, my = -1, evr = 0, k = -1;
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int ch = 0; ch < nchunk; ++ch) {
    const float s = off[ch * 64 + lane];
    float bat = fv;
    uint64_t NC = ~0ull, RB = 0ull, done = 0ull;
    int nv = 0;
    one_call<VAR>(s, -1, 0, geo, aj, al, ar, dum, my, evr, bat, NC, RB, done, 0ull, fv, fs, nfree, nv, 0, k);
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) *(volatile int*)&flag = 1;
  for (int i = lane; i <= 128; i += 64) { out_hv[i] = he[i + 1].v; out_hs[i] = he[i + 1].s; }
  out_my[lane] = my;
  if (lane == 0) cyc[0] = t1 - t0;
}

// ---------------------------------------------------------------------------
// host replay
struct El { float v; int s; };
struct Gt { bool operator()(const El& a, const El& b) const { return a.v > b.v; } };

static unsigned long long low(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

// the loop's rule on a Call, the heap step by TopN's own sequence over the
// beam's W elements; returns the pushes made
static int replay(Call& q, int W) {
  std::vector<El> e(W);
  for (int i = 0; i < W; ++i) e[i] = El{q.hv[i], q.hs[i]};
  int pushes = 0;
  q.st = 0;
  q.k = -1;
  for (;;) {
    unsigned long long m = 0;
    for (int j = 0; j < 64; ++j)
      if ((((q.NC >> j) & 1ull) && q.s[j] > q.fv) || ((q.RB >> j) & 1ull)) m |= 1ull << j;
    m &= ~q.done;
    if (!m) break;
    const int k = __builtin_ctzll(m);
    if ((q.LB >> k) & 1ull) { q.st = 1; q.k = k; break; }
    q.done = low(k + 1);
    int slot = q.fs;
    if (q.fs < q.nb) {
      slot = q.nfree++;
      q.evr[q.nv++] = q.fs;
      for (int j = 0; j < 64; ++j)
        if (q.c[j] == q.fs && ((q.LB >> j) & 1ull)) q.RB |= 1ull << j;
    }
    for (int j = 0; j < 64; ++j)
      if (q.my[j] == q.fs) q.my[j] = -1;
    q.my[k] = slot;
    e.push_back(El{q.s[k], slot});               // the spare slot
    std::pop_heap(e.begin(), e.end(), Gt());
    e.pop_back();
    q.fv = e[0].v;
    q.fs = e[0].s;
    for (int j = 0; j < 64; ++j)
      if (q.sl[j] > k) q.bat[j] = q.fv;
    ++pushes;
  }
  for (int i = 0; i < W; ++i) { q.hv[i] = e[i].v; q.hs[i] = e[i].s; }
  return pushes;
}

static int differ(const Call& a, const Call& b, int W) {
  int d = 0;
  for (int i = 0; i <= 128; ++i) {
    const bool sent = i >= W;
    d += a.hs[i] != b.hs[i] || std::memcmp(&a.hv[i], &b.hv[i], 4) != 0;
    if (sent) d += a.hs[i] != -1 || a.hv[i] != kInf;
  }
  for (int j = 0; j < 64; ++j) {
    d += a.my[j] != b.my[j];
    d += std::memcmp(&a.bat[j], &b.bat[j], 4) != 0;
  }
  for (int j = 0; j < a.nv && j < 64; ++j) d += a.evr[j] != b.evr[j];
  d += a.NC != b.NC || a.RB != b.RB || a.done != b.done;
  d += std::memcmp(&a.fv, &b.fv, 4) != 0 || a.fs != b.fs || a.nfree != b.nfree || a.nv != b.nv;
  d += a.st != b.st || a.k != b.k;
  return d;
}

int main() {
  std::mt19937 g(26);
  Call *din, *dout;
  (void)hipMalloc(&din, sizeof(Call));
  (void)hipMalloc(&dout, sizeof(Call));
  const int Ws[7] = {2, 3, 33, 64, 65, 127, 128};
  long cases = 0, calls = 0, pushes = 0, reentries = 0, evbs = 0, bad_ab = 0, bad_host = 0;
  for (int wi = 0; wi < 7; ++wi)
    for (int it = 0; it < 48; ++it) {
      const int W = Ws[wi];
      const int q = it % 3 == 2 ? 0 : 1 + (it % 3);   // 4 or 8 distinct values (ties everywhere), or normal draws
      const bool rare = it % 4 >= 2;                  // LB lanes: the loop returns 1 mid-chunk
      const bool evb = it % 2 == 1;                   // branch entries in the heap (slots below nb)
      std::normal_distribution<float> nd;
      auto val = [&](float lift) { return q ? (float)(g() % (q * 4)) / q + (float)(int)lift : nd(g) + lift; };
      Call c0;
      std::memset(&c0, 0, sizeof c0);
      c0.nb = evb ? W : 0;
      std::vector<El> e(W);
      // slots: a shuffle of 0..2W-1's first W (with evb, about half are below nb)
      std::vector<int> sl(2 * W);
      for (int i = 0; i < 2 * W; ++i) sl[i] = i;
      std::shuffle(sl.begin(), sl.end(), g);
      for (int i = 0; i < W; ++i) e[i] = El{val(0.f), sl[i]};
      if (it % 5 == 1) std::sort(e.begin(), e.end(), [](const El& a, const El& b) { return a.v < b.v; });
      std::make_heap(e.begin(), e.end(), Gt());
      for (int i = 0; i <= 128; ++i) { c0.hv[i] = i < W ? e[i].v : kInf; c0.hs[i] = i < W ? e[i].s : -1; }
      c0.fv = e[0].v; c0.fs = e[0].s; c0.nfree = 2 * W;
      const int cqn = it % 7 == 0 ? 1 + (int)(g() % 64) : 64;
      int turn = 0;
      unsigned long long liveM = 0, isb = 0;
      for (int j = 0; j < 64; ++j) {
        c0.s[j] = val(it % 6 == 0 ? 0.f : 1.f);       // mostly above the front
        if (j && g() % 5 == 0) turn = j;              // a branch turn starts at lane j
        c0.sl[j] = turn;
        const bool b = rare && g() % 6 == 0;
        c0.c[j] = b ? (int)(g() % (unsigned)(evb ? W : 2 * W)) : -1;
        if (j < cqn && g() % 16 != 0) liveM |= 1ull << j;
        if (b) isb |= 1ull << j;
        c0.my[j] = -1;
        c0.bat[j] = c0.sl[j] > 0 ? c0.fv : -kInf;
      }
      c0.NC = liveM & ~isb; c0.LB = liveM & isb;
      c0.RB = 0;
      for (int j = 0; j < 64; ++j)
        if (((c0.LB >> j) & 1ull) && g() % 4 == 0) c0.RB |= 1ull << j;
      ++cases;
      Call st[3] = {c0, c0, c0};   // the old loop, the new loop, the host replay
      for (int round = 0; round < 70; ++round) {
        Call o[2];
        for (int v = 0; v < 2; ++v) {
          (void)hipMemcpy(din, &st[v], sizeof(Call), hipMemcpyHostToDevice);
          if (v == 0) hipLaunchKernelGGL(call_kernel<0>, dim3(1), dim3(64), 0, 0, din, dout);
          else hipLaunchKernelGGL(call_kernel<1>, dim3(1), dim3(64), 0, 0, din, dout);
          o[v] = st[v];
          Call r;
          if (hipMemcpy(&r, dout, sizeof(Call), hipMemcpyDeviceToHost) != hipSuccess) {
            printf("push_unit: HIP error after a call; stopping\n");
            return 2;
          }
          std::memcpy(o[v].hv, r.hv, sizeof r.hv); std::memcpy(o[v].hs, r.hs, sizeof r.hs);
          std::memcpy(o[v].my, r.my, sizeof r.my); std::memcpy(o[v].evr, r.evr, sizeof r.evr);
          std::memcpy(o[v].bat, r.bat, sizeof r.bat);
          o[v].NC = r.NC; o[v].RB = r.RB; o[v].done = r.done; o[v].fv = r.fv; o[v].fs = r.fs;
          o[v].nfree = r.nfree; o[v].nv = r.nv; o[v].st = r.st; o[v].k = r.k;
        }
        const int nv0 = st[2].nv;
        const int np = replay(st[2], W);
        pushes += np;
        evbs += st[2].nv - nv0;
        ++calls;
        const int dab = differ(o[0], o[1], W), dh = differ(o[1], st[2], W);
        if (dab) { if (bad_ab < 8) printf("W %d case %d call %d: old/new differ in %d places\n", W, it, round, dab); ++bad_ab; }
        if (dh) { if (bad_host < 8) printf("W %d case %d call %d: new/host differ in %d places\n", W, it, round, dh); ++bad_host; }
        if (dab || dh || st[2].st == 0) break;
        // the caller's part of a re-offering lane k, reduced to a rejection:
        // lanes up to k are done and lane k leaves the masks
        ++reentries;
        for (int v = 0; v < 3; ++v) {
          Call& n = v < 2 ? o[v] : st[2];
          const int k = n.k;
          n.done = low(k + 1);
          n.NC &= ~(1ull << k); n.LB &= ~(1ull << k); n.RB &= ~(1ull << k);
          if (v < 2) st[v] = n;
        }
      }
    }
  printf("checks: %ld cases, %ld calls (%ld re-entered after a return of 1), %ld pushes, %ld evicted branch entries\n",
         cases, calls, reentries, pushes, evbs);
  printf("push_unit: %ld calls differ old/new, %ld differ new/host replay (CTCX_PUSH_COPIES=%d)\n", bad_ab, bad_host,
         CTCX_PUSH_COPIES);

  // timing: a full heap of 128, 64 chunks of 64 offers that rise fast enough
  // for nearly every one to be accepted
  float *dhv, *doff, *ohv;
  int *dhs, *ohs, *omy;
  unsigned long long* dc;
  (void)hipMalloc(&dhv, 4 * 129); (void)hipMalloc(&dhs, 4 * 129); (void)hipMalloc(&doff, 4 * 64 * kChunks);
  (void)hipMalloc(&ohv, 4 * 129); (void)hipMalloc(&ohs, 4 * 129); (void)hipMalloc(&omy, 4 * 64); (void)hipMalloc(&dc, 16);
  int bad_t = 0;
  for (int tie = 0; tie < 2; ++tie) {
    std::vector<El> e(128);
    std::normal_distribution<float> nd;
    for (int i = 0; i < 128; ++i) e[i] = El{tie ? (float)(g() % 8) * 0.5f : nd(g), i};
    std::make_heap(e.begin(), e.end(), Gt());
    float hv[129];
    int hs[129];
    for (int i = 0; i <= 128; ++i) { hv[i] = i < 128 ? e[i].v : kInf; hs[i] = i < 128 ? e[i].s : -1; }
    std::vector<float> off(64 * kChunks);
    for (int i = 0; i < 64 * kChunks; ++i) {
      const float lift = 0.004f * (float)i;
      off[i] = tie ? (float)(g() % 8) * 0.5f + (float)(int)lift : nd(g) + lift;
    }
    // the host's count of pushes and final heap
    long np = 0;
    {
      Call q;
      std::memset(&q, 0, sizeof q);
      std::memcpy(q.hv, hv, sizeof hv); std::memcpy(q.hs, hs, sizeof hs);
      q.fv = hv[0]; q.fs = hs[0]; q.nfree = 100000; q.nb = 0;
      for (int j = 0; j < 64; ++j) { q.c[j] = -1; q.my[j] = -1; }
      for (int ch = 0; ch < kChunks; ++ch) {
        std::memcpy(q.s, &off[ch * 64], 256);
        q.NC = ~0ull; q.RB = 0; q.LB = 0; q.done = 0; q.nv = 0;
        np += replay(q, 128);
      }
      (void)hipMemcpy(dhv, hv, 4 * 129, hipMemcpyHostToDevice);
      (void)hipMemcpy(dhs, hs, 4 * 129, hipMemcpyHostToDevice);
      (void)hipMemcpy(doff, off.data(), 4 * 64 * kChunks, hipMemcpyHostToDevice);
      for (int busy = 0; busy < 2; ++busy) {
        double best[2] = {1e30, 1e30}, sum[2] = {0, 0};
        const int reps = 9;
        for (int rep = 0; rep < reps; ++rep)
          for (int v = 0; v < 2; ++v) {
            if (v == 0) hipLaunchKernelGGL(time_kernel<0>, dim3(1), dim3(busy ? 128 : 64), 0, 0, dhv, dhs, doff, kChunks, busy, dc, ohv, ohs, omy);
            else hipLaunchKernelGGL(time_kernel<1>, dim3(1), dim3(busy ? 128 : 64), 0, 0, dhv, dhs, doff, kChunks, busy, dc, ohv, ohs, omy);
            unsigned long long c;
            float gv[129];
            int gs[129];
            if (hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost) != hipSuccess) {
              printf("push_unit: HIP error after a timing run; stopping\n");
              return 2;
            }
            (void)hipMemcpy(gv, ohv, 4 * 129, hipMemcpyDeviceToHost);
            (void)hipMemcpy(gs, ohs, 4 * 129, hipMemcpyDeviceToHost);
            int mism = 0;
            for (int i = 0; i < 128; ++i) mism += gs[i] != q.hs[i] || gv[i] != q.hv[i];
            if (mism) { if (bad_t < 8) printf("timing run (%s, loop %d): final heap differs from the host's in %d places\n", tie ? "ties" : "normal", v, mism); ++bad_t; }
            const double cp = (double)c / (double)np;
            best[v] = std::min(best[v], cp);
            sum[v] += cp;
          }
        printf("cycles per push, %s, %s (%ld pushes, %d runs: best / mean): old %.1f / %.1f, new %.1f / %.1f\n",
               tie ? "8 distinct values" : "normal draws",
               busy ? "a second wave reading LDS" : "alone on the CU", np, reps, best[0], sum[0] / reps, best[1], sum[1] / reps);
      }
    }
  }
  printf("push_unit: %d timing runs left a heap other than the host's\n", bad_t);
  return (bad_ab || bad_host || bad_t) ? 1 : 0;
}
