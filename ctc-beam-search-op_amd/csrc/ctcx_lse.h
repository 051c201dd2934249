// ctcx_lse.h — the device helpers the forward-recursion kernels share
// (ctcx_paths.hip, ctcx_targets.hip): the log-domain sums, the widening read of
// a logits row and the DPP move.  Device code only, internal linkage; it
// includes no header of the decode objects.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

template <typename T>
__device__ __forceinline__ T ninf() { return (T)(-__builtin_inff()); }

// element idx of the row at `row`, widened as the decode kernels' row stage
// widens it (fp16: the hardware convert; bf16: the bits, 16 to the left);
// Fmt is a kPathsIn* value (0 native, 1 fp16, 2 bf16)
template <typename T, int Fmt>
__device__ __forceinline__ T row_at(const void* row, uint32_t idx) {
  if constexpr (Fmt == 1)
    return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)row)[idx]);
  else if constexpr (Fmt == 2)
    return (T)__uint_as_float((unsigned)((const uint16_t*)row)[idx] << 16);
  else
    return ((const T*)row)[idx];
}
template <int Fmt, typename T>
__device__ __forceinline__ const void* row_ptr(const void* x, int64_t off) {
  if constexpr (Fmt == 0) return (const T*)x + off;
  else return (const uint16_t*)x + off;
}

__device__ __forceinline__ float ex(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }
__device__ __forceinline__ float lg(float s) { return __builtin_amdgcn_logf(s) * 0.69314718055994530942f; }
__device__ __forceinline__ double ex(double d) { return exp(d); }
__device__ __forceinline__ double lg(double s) { return log(s); }
__device__ __forceinline__ float mx2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double mx2(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float ab(float a) { return fabsf(a); }
__device__ __forceinline__ double ab(double a) { return fabs(a); }

// log(exp(a) + exp(b)); all -inf (or NaN beside -inf): a + b.  A NaN argument
// gives a NaN in both functions: the maximum drops it (fmax returns the other
// argument), but every argument also goes through a subtraction of its own
// (here a - b, below a - m, b - m, c - m), and the NaN comes back through that.
template <typename T>
__device__ __forceinline__ T lse2(T a, T b) {
  const T m = mx2(a, b);
  const T r = m + lg((T)1 + ex(-ab(a - b)));   // (min - max, as a free modifier)
  return m > ninf<T>() ? r : a + b;
}
template <typename T>
__device__ __forceinline__ T lse3(T a, T b, T c) {
  const T m = mx2(mx2(a, b), c);
  const T r = m + lg(ex(a - m) + ex(b - m) + ex(c - m));
  return m > ninf<T>() ? r : a + b + c;
}

template <int Ctrl>
__device__ __forceinline__ int dpp_keep(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, Ctrl, 0xf, 0xf, false);   // a lane without a source keeps `old`
}
// lane l receives lane l - 1's v, lane 0 -inf (wave_shr:1)
__device__ __forceinline__ float from_prev_lane(float v) {
  return __int_as_float(dpp_keep<0x138>(__float_as_int(ninf<float>()), __float_as_int(v)));
}
__device__ __forceinline__ double from_prev_lane(double v) {
  const double o = ninf<double>();
  return __hiloint2double(dpp_keep<0x138>(__double2hiint(o), __double2hiint(v)),
                          dpp_keep<0x138>(__double2loint(o), __double2loint(v)));
}
__device__ __forceinline__ float finite_or_ninf(float v) { return fabsf(v) < __builtin_inff() ? v : ninf<float>(); }

}  // namespace
