// heap_fwd_unit.hip — GPU unit test and timing of the decode kernel's
// sort_heap loop with the child pairs forwarded in registers
// (extract_fwd_f32) against the loop that re-reads them from LDS after every
// pop (extract_f32), both taken from the kernel source as they stand.
//   * layouts: slots popped and the heap left behind, for every pop count,
//     against libstdc++'s std::pop_heap on tie-heavy arrays;
//   * cycles per pop (s_memtime around a whole extract, segments as in
//     exact_step's Extract), old against new, same arrays.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DCTCX_PART=99 tools/heap_fwd_unit.hip -o tools/heap_fwd_unit.bin
// (CTCX_PART=99: no kernel instantiation and no dispatcher, the device functions only)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../ctc-beam-search-op_amd/csrc/ctcx_decode.hip"

using namespace ctcx;

struct El { float v; int s; };
struct Gt { bool operator()(const El& a, const El& b) const { return a.v > b.v; } };

constexpr int kHdum = 130;   // he index of lane 0's dummy slot (positions 0..128, then the dummies)

// one wave: a heap of len elements (host layout) with sentinels behind it,
// sort_heap pops down to `stop` elements in exact_step's segments, with
// extract_fwd_f32 (fwd) or extract_f32; out: the popped slots by position,
// the heap's remaining nodes and the cycles spent in the pops
__global__ void pop_kernel(const float* v, const int* s, int len, int stop, int fwd, int* out_srt, float* out_hv,
                           int* out_hs, unsigned long long* cyc) {
  __shared__ __attribute__((aligned(16))) HE<float> lds[kHdum + 64];
  CTCX_LDS HE<float>* he = (CTCX_LDS HE<float>*)lds;
  const int lane = threadIdx.x;
  for (int i = lane; i <= 128; i += 64)
    he_st(he, i + 1, i < len ? HE<float>{v[i], s[i]} : HE<float>{std::numeric_limits<float>::infinity(), -1});
  __syncthreads();
  const HeapM geo = heap_m(kHdum);
  const unsigned heb = (unsigned)(uintptr_t)he;
  const unsigned aj = heb + 8u * (unsigned)(lane + 1), al = heb + 8u * (unsigned)(2 * lane + 2);
  const unsigned ar = al + 8u, dum = heb + 8u * (unsigned)(kHdum + lane);
  int fs = uni(he_ld(he, 1).s);
  int srt0 = -7, srt1 = -7;
  auto seg = [&](int top, int lo, int base, int& srt) {
    const int hi = len < top ? len : top;
    const int l = lo > stop ? lo : stop;
    if (hi <= l) return;
    if (fwd) extract_fwd_f32(heb, uni(hi), uni(l), base, geo.anc, geo.req, aj, al, dum, srt, fs);
    else extract_f32(heb, uni(hi), uni(l), base, geo.anc, geo.req, aj, al, ar, dum, srt, fs);
  };
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  seg(128, 96, 64, srt1);
  seg(96, 64, 64, srt1);
  seg(64, 32, 0, srt0);
  seg(32, 2, 0, srt0);
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  __syncthreads();
  out_srt[lane] = srt0;
  out_srt[64 + lane] = srt1;
  for (int i = lane; i <= 128; i += 64) { out_hv[i] = he[i + 1].v; out_hs[i] = he[i + 1].s; }
  if (lane == 0) { cyc[0] = t1 - t0; out_srt[128] = fs; }
}

int main() {
  std::mt19937 g(11);
  float *dv, *ohv;
  int *ds, *osrt, *ohs;
  unsigned long long* dc;
  (void)hipMalloc(&dv, 4 * 129); (void)hipMalloc(&ds, 4 * 129); (void)hipMalloc(&osrt, 4 * 129);
  (void)hipMalloc(&ohv, 4 * 129); (void)hipMalloc(&ohs, 4 * 129); (void)hipMalloc(&dc, 8);
  int bad = 0, cases = 0;
  double cyc[2] = {0, 0};
  long pops = 0;
  for (int it = 0; it < 400; ++it) {
    // every length 3..128 comes up (it % 126), the rest random; stop anywhere below it
    const int len = it < 126 ? 3 + it : 3 + (int)(g() % 126);
    const int stop = it % 3 == 0 ? 2 : 2 + (int)(g() % (len - 2));
    const int q = it % 4 == 3 ? 0 : 1 + (int)(g() % 2);   // 4 or 8 distinct values (ties), or none (normal draws)
    std::vector<El> e(len);
    std::normal_distribution<float> nd;
    for (int i = 0; i < len; ++i) e[i] = El{q ? (float)(g() % (q * 4)) / q : nd(g), i};
    if (it % 5 == 1) std::sort(e.begin(), e.end(), [](const El& a, const El& b) { return a.v < b.v; });
    std::make_heap(e.begin(), e.end(), Gt());
    std::vector<float> hv(len);
    std::vector<int> hs(len);
    for (int i = 0; i < len; ++i) { hv[i] = e[i].v; hs[i] = e[i].s; }
    (void)hipMemcpy(dv, hv.data(), 4 * len, hipMemcpyHostToDevice);
    (void)hipMemcpy(ds, hs.data(), 4 * len, hipMemcpyHostToDevice);
    for (int l = len; l > stop; --l) std::pop_heap(e.begin(), e.begin() + l, Gt());
    for (int fwd = 0; fwd < 2; ++fwd) {
      hipLaunchKernelGGL(pop_kernel, dim3(1), dim3(64), 0, 0, dv, ds, len, stop, fwd, osrt, ohv, ohs, dc);
      int srt[129], gs[129];
      float gv[129];
      unsigned long long c;
      (void)hipMemcpy(srt, osrt, 4 * 129, hipMemcpyDeviceToHost);
      (void)hipMemcpy(gs, ohs, 4 * 129, hipMemcpyDeviceToHost);
      (void)hipMemcpy(gv, ohv, 4 * 129, hipMemcpyDeviceToHost);
      (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
      int mism = 0;
      for (int p = stop; p < len; ++p) mism += srt[p] != e[p].s;                       // the popped slots
      for (int p = 0; p < stop; ++p) mism += gs[p] != e[p].s || gv[p] != e[p].v;       // the heap left behind
      for (int p = stop; p <= 128; ++p) mism += gs[p] != -1 || !(gv[p] > 3.0e38f);     // sentinels behind it
      mism += srt[128] != e[0].s;                                                      // the front's slot
      ++cases;
      if (mism) {
        if (bad < 8) printf("case %d %s len %d stop %d q %d: %d mismatches\n", it, fwd ? "fwd" : "old", len, stop, q, mism);
        ++bad;
      }
      cyc[fwd] += (double)c;
      if (fwd == 0) pops += len - stop;
    }
  }
  // the decode's case: 128 elements popped to 2, normal draws, and the same with ties
  for (int tie = 0; tie < 2; ++tie) {
    double c2[2] = {0, 0};
    for (int rep = 0; rep < 16; ++rep) {
      std::vector<El> e(128);
      std::normal_distribution<float> nd;
      for (int i = 0; i < 128; ++i) e[i] = El{tie ? (float)(g() % 8) * 0.5f : nd(g), i};
      std::make_heap(e.begin(), e.end(), Gt());
      std::vector<float> hv(128);
      std::vector<int> hs(128);
      for (int i = 0; i < 128; ++i) { hv[i] = e[i].v; hs[i] = e[i].s; }
      (void)hipMemcpy(dv, hv.data(), 4 * 128, hipMemcpyHostToDevice);
      (void)hipMemcpy(ds, hs.data(), 4 * 128, hipMemcpyHostToDevice);
      for (int fwd = 0; fwd < 2; ++fwd) {
        hipLaunchKernelGGL(pop_kernel, dim3(1), dim3(64), 0, 0, dv, ds, 128, 2, fwd, osrt, ohv, ohs, dc);
        unsigned long long c;
        (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
        c2[fwd] += (double)c;
      }
    }
    printf("sort_heap 128 -> 2 (%s): %.1f cycles per pop re-reading the pairs, %.1f forwarding them\n",
           tie ? "8 distinct values" : "normal draws", c2[0] / (16 * 126), c2[1] / (16 * 126));
  }
  printf("all %d cases: %.1f cycles per pop re-reading, %.1f forwarding (%ld pops each)\n", cases / 2,
         cyc[0] / pops, cyc[1] / pops, pops);
  printf("heap_fwd_unit: %d/%d cases mismatched\n", bad, cases);
  return bad ? 1 : 0;
}
