// reg_sort_unit.hip — GPU unit test and timing of the decode kernel's
// register-resident std::sort (reg_sort_extract over ctcx_regsort.h) against
// lane 0's literal replay over LDS (lit_sort), both taken from the kernel
// source as they stand.
//   * one launch, one wave per case: the wave sorts its own array with both
//     forms; the host compares both slot orders with std::sort under the same
//     comparator (ties included) over every length 1..128 and the input
//     families of tests/test_cpu_reg_sort.py, and an adversarial input of
//     length 128 that reaches the depth limit (the register form must give up
//     there, and the literal form must give std::sort's result);
//   * cycles per sort (s_memtime around each form), n = 17, 64 and 128, on the
//     descending array with its minimum swapped to the front: those cases run
//     once more in a small launch of their own, one wave per CU.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DCTCX_PART=99 tools/reg_sort_unit.hip -o tools/reg_sort_unit.bin
// (CTCX_PART=99: no kernel instantiation and no dispatcher, the device functions only;
//  csrc/Makefile builds it with the library)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../ctc-beam-search-op_amd/csrc/ctcx_decode.hip"

using namespace ctcx;

constexpr int kSlots = 384;   // slot ids stay below 3 W
constexpr int kMaxN = 128;

#define HIP_OK(e)                                                                          \
  do {                                                                                     \
    const hipError_t err_ = (e);                                                           \
    if (err_ != hipSuccess) {                                                              \
      printf("reg_sort_unit: %s at line %d\n", hipGetErrorString(err_), __LINE__);         \
      return 2;                                                                            \
    }                                                                                      \
  } while (0)

// block b: case b.  tot: [case][kSlots] totals by slot; e: [case][kMaxN] slots by position
__global__ __launch_bounds__(64) void sort_kernel(const float* tot, const int* e, const int* ns, int ncases,
                                                  int* out_reg, int* out_lit, int* fell, unsigned long long* cyc) {
  __shared__ float et[kSlots];
  __shared__ __attribute__((aligned(16))) HE<float> lds[kMaxN + 2];
  __shared__ int srt[kMaxN];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= ncases) return;
  int n = ns[b];
  n = n < 1 ? 1 : n > kMaxN ? kMaxN : n;
  CTCX_LDS HE<float>* he = (CTCX_LDS HE<float>*)lds;
  for (int i = lane; i < kSlots; i += 64) et[i] = tot[(size_t)b * kSlots + i];
  for (int i = lane; i < kMaxN; i += 64) {
    int s = e[(size_t)b * kMaxN + i];
    s = s < 0 ? 0 : s >= kSlots ? kSlots - 1 : s;
    he_st(he, i + 1, HE<float>{tot[(size_t)b * kSlots + s], s});
    srt[i] = -1;
  }
  __syncthreads();
  Ctx<float> cx{};
  cx.et = (CTCX_LDS float*)et;
  cx.sorted = (CTCX_LDS int*)srt;
  n = uni(n);
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  const bool ok = reg_sort_extract<float>(cx, he, n);
  __syncthreads();
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  for (int i = lane; i < n; i += 64) out_reg[(size_t)b * kMaxN + i] = srt[i];
  __syncthreads();
  const uint64_t t2 = __builtin_amdgcn_s_memtime();
  if (lane == 0) {
    for (int q = 0; q < n; ++q) cx.sorted[q] = he[q + 1].s;
    lit_sort(cx.sorted, n, SlotGreater<float>{cx.et});
  }
  __syncthreads();
  const uint64_t t3 = __builtin_amdgcn_s_memtime();
  for (int i = lane; i < n; i += 64) out_lit[(size_t)b * kMaxN + i] = srt[i];
  if (lane == 0) {
    fell[b] = ok ? 0 : 1;
    cyc[2 * (size_t)b] = t1 - t0;
    cyc[2 * (size_t)b + 1] = t3 - t2;
  }
}

struct Cases {
  std::vector<float> tot;
  std::vector<int> e, ns;
  std::vector<const char*> what;
  std::mt19937 g{7};
  int add(const std::vector<float>& t, const char* w) {
    const int n = (int)t.size();
    std::vector<int> ids(kSlots);
    for (int i = 0; i < kSlots; ++i) ids[i] = i;
    std::shuffle(ids.begin(), ids.end(), g);
    const size_t c = ns.size();
    tot.resize((c + 1) * kSlots, 0.f);
    e.resize((c + 1) * kMaxN, 0);
    for (int p = 0; p < n; ++p) {
      e[c * kMaxN + p] = ids[p];
      tot[c * kSlots + ids[p]] = t[p];
    }
    ns.push_back(n);
    what.push_back(w);
    return (int)c;
  }
};

// McIlroy's adversary against std::sort: values decided while the sort compares them
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
  for (int i = 0; i < n; ++i) t[i] = -(float)adv_val[i];
  return t;
}

int main() {
  Cases cs;
  std::mt19937& g = cs.g;
  std::normal_distribution<float> nd;
  const float NINF = -std::numeric_limits<float>::infinity();
  for (int n = 1; n <= kMaxN; ++n) {
    std::vector<float> t(n);
    for (int i = 0; i < n; ++i) t[i] = -(float)i * 0.25f;
    cs.add(t, "descending");
    std::swap(t[0], t[n - 1]);
    cs.add(t, "front-swap");
    for (int rep = 0; rep < 3; ++rep) {
      for (auto& x : t) x = nd(g);
      cs.add(t, "random");
    }
    for (auto& x : t) x = 1.5f;
    cs.add(t, "all-equal");
    const int nds[3] = {2, 4, n / 2 > 0 ? n / 2 : 1};
    for (int q = 0; q < 3; ++q)
      for (int rep = 0; rep < 2; ++rep) {
        for (auto& x : t) x = 0.5f * (float)(g() % nds[q]);
        if (rep == 1) { std::sort(t.begin(), t.end(), std::greater<float>()); std::swap(t[0], t[n - 1]); }
        cs.add(t, "tie-heavy");
      }
    if (n >= 4)
      for (int rep = 0; rep < 3; ++rep) {
        for (int i = 0; i < n; ++i) t[i] = -(float)i;
        t[1] = t[0];
        t[n - 2] = t[n - 1];
        if (rep == 1) std::swap(t[0], t[n - 1]);
        if (rep == 2) std::shuffle(t.begin(), t.end(), g);
        cs.add(t, "twins");
      }
    for (int rep = 0; rep < 3; ++rep) {
      for (auto& x : t) x = nd(g);
      const int k = rep == 0 ? 1 : 1 + (int)(g() % n);
      for (int i = 0; i < k; ++i) t[g() % n] = NINF;
      if (rep == 2) { std::sort(t.begin(), t.end(), std::greater<float>()); std::swap(t[0], t[n - 1]); }
      cs.add(t, "-inf");
    }
    for (auto& x : t) x = NINF;
    cs.add(t, "all -inf");
  }
  const int kill = cs.add(killer(kMaxN), "killer");
  // timing: the descending array with its minimum in front, random draws
  const int tn[3] = {17, 64, 128};
  constexpr int kReps = 16;
  int tfirst[3];
  for (int q = 0; q < 3; ++q)
    for (int rep = 0; rep < kReps; ++rep) {
      std::vector<float> t(tn[q]);
      for (auto& x : t) x = nd(g);
      std::sort(t.begin(), t.end(), std::greater<float>());
      std::swap(t[0], t[tn[q] - 1]);
      const int c = cs.add(t, "timing");
      if (rep == 0) tfirst[q] = c;
    }
  const int nc = (int)cs.ns.size();

  float* dtot;
  int *de, *dns, *oreg, *olit, *dfell;
  unsigned long long* dcyc;
  HIP_OK(hipMalloc(&dtot, sizeof(float) * cs.tot.size()));
  HIP_OK(hipMalloc(&de, sizeof(int) * cs.e.size()));
  HIP_OK(hipMalloc(&dns, sizeof(int) * nc));
  HIP_OK(hipMalloc(&oreg, sizeof(int) * (size_t)nc * kMaxN));
  HIP_OK(hipMalloc(&olit, sizeof(int) * (size_t)nc * kMaxN));
  HIP_OK(hipMalloc(&dfell, sizeof(int) * nc));
  HIP_OK(hipMalloc(&dcyc, sizeof(unsigned long long) * 2 * nc));
  HIP_OK(hipMemcpy(dtot, cs.tot.data(), sizeof(float) * cs.tot.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(de, cs.e.data(), sizeof(int) * cs.e.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dns, cs.ns.data(), sizeof(int) * nc, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(oreg, 0xff, sizeof(int) * (size_t)nc * kMaxN));
  HIP_OK(hipMemset(olit, 0xff, sizeof(int) * (size_t)nc * kMaxN));
  hipLaunchKernelGGL(sort_kernel, dim3(nc), dim3(64), 0, 0, dtot, de, dns, nc, oreg, olit, dfell, dcyc);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<int> hreg((size_t)nc * kMaxN), hlit((size_t)nc * kMaxN), hfell(nc);
  std::vector<unsigned long long> hcyc(2 * (size_t)nc);
  HIP_OK(hipMemcpy(hreg.data(), oreg, sizeof(int) * hreg.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hlit.data(), olit, sizeof(int) * hlit.size(), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hfell.data(), dfell, sizeof(int) * nc, hipMemcpyDeviceToHost));
  // the timing cases once more on their own (the last 3 * kReps cases: at most
  // one wave per CU, so the cycles are the sort's and not a neighbour's)
  {
    const int c0 = tfirst[0], nt = nc - c0;
    hipLaunchKernelGGL(sort_kernel, dim3(nt), dim3(64), 0, 0, dtot + (size_t)c0 * kSlots, de + (size_t)c0 * kMaxN,
                       dns + c0, nt, oreg + (size_t)c0 * kMaxN, olit + (size_t)c0 * kMaxN, dfell + c0, dcyc + 2 * (size_t)c0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
  }
  HIP_OK(hipMemcpy(hcyc.data(), dcyc, sizeof(unsigned long long) * hcyc.size(), hipMemcpyDeviceToHost));

  int bad = 0, fells = 0;
  for (int c = 0; c < nc; ++c) {
    const int n = cs.ns[c];
    const float* tot = &cs.tot[(size_t)c * kSlots];
    std::vector<int> want(cs.e.begin() + (size_t)c * kMaxN, cs.e.begin() + (size_t)c * kMaxN + n);
    std::sort(want.begin(), want.end(), [&](int a, int b) { return tot[a] > tot[b]; });
    int mreg = 0, mlit = 0;
    for (int p = 0; p < n; ++p) {
      mlit += hlit[(size_t)c * kMaxN + p] != want[p];
      if (!hfell[c]) mreg += hreg[(size_t)c * kMaxN + p] != want[p];
      else mreg += hreg[(size_t)c * kMaxN + p] != -1;   // a sort that gives up stores nothing
    }
    fells += hfell[c];
    if (mreg || mlit) {
      if (bad < 8) printf("case %d (%s, n %d): %d register, %d literal mismatches\n", c, cs.what[c], n, mreg, mlit);
      ++bad;
    }
  }
  const bool kill_ok = hfell[kill] == 1 && fells == 1;
  printf("depth-limit input: register sort gave up %d (cases that gave up: %d, want 1)\n", hfell[kill], fells);
  for (int q = 0; q < 3; ++q) {
    double cr = 0, cl = 0;
    for (int rep = 0; rep < kReps; ++rep) {
      cr += (double)hcyc[2 * (size_t)(tfirst[q] + rep)];
      cl += (double)hcyc[2 * (size_t)(tfirst[q] + rep) + 1];
    }
    printf("n = %3d, minimum in front of a descending array: %.0f cycles per sort in registers, %.0f literal\n",
           tn[q], cr / kReps, cl / kReps);
  }
  printf("reg_sort_unit: %d/%d cases mismatched\n", bad, nc);
  return bad || !kill_ok ? 1 : 0;
}
