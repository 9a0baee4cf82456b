// wave_ops.h -- the cross-lane primitives of the gfx950 kernels, one name per operation (device
// code only; wave size 64).
//
//   gt_max, gt_maxf            arma-style maximum (NaN never wins)
//   wave_sum, wave_max         64-lane butterflies on __shfl_xor, every lane gets the result
//   dpp_d, dpp_f               DPP moves within a 16-lane row; control words kDppXor1, kDppXor2,
//                              kDppHalfMirror, kDppMirror (lane ^ 1, ^ 2, ^ 7, ^ 15)
//   swap16, swap32 (+ f)       v_permlane16_swap / v_permlane32_swap of a register pair
//   swz_d                      ds_swizzle of a double
//   red_op, row16_sum, row16_max_i32, wave_allreduce, wave_maxf
//                              reductions built from the moves, all on VALU (no LDS round trips)
// Block-level reductions stay with their kernels: their combine orders differ, and merging them
// would change bits.
#pragma once
#include <hip/hip_runtime.h>

namespace scde {

// arma-style max: NaN never wins (first-max semantics live in the argmax paths)
__device__ __forceinline__ double gt_max(double a, double b) { return (b > a) ? b : a; }
__device__ __forceinline__ float gt_maxf(float a, float b) { return (b > a) ? b : a; }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Cross-lane moves on VALU (no LDS path): gfx950 v_permlane{32,16}_swap exchange the
// upper half-wave / odd rows of one register with the lower half / even rows of another
// (each leaves the two halves' values side by side, so one op combines them on every lane);
// DPP row_mirror (lane ^ 15), row_half_mirror (lane ^ 7), quad_perm (lane ^ 2, ^ 1).
constexpr int kDppMirror = 0x140, kDppHalfMirror = 0x141, kDppXor2 = 0x4E, kDppXor1 = 0xB1;
template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ void swap32(double& a, double& b) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false,
                                                   false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false,
                                                   false);
  a = __hiloint2double((int)hi[0], (int)lo[0]);
  b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap16(double& a, double& b) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false,
                                                   false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false,
                                                   false);
  a = __hiloint2double((int)hi[0], (int)lo[0]);
  b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap32f(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16f(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
// a double from the lane ds_swizzle's bit-mode PATTERN names (and 0x1F, xor in bits 10-14: within
// 32 lanes; an LDS-crossbar op, no memory access)
template <int PATTERN>
__device__ __forceinline__ double swz_d(double x) {
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), PATTERN);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), PATTERN);
  return __hiloint2double(hi, lo);
}

template <bool MAX>
__device__ __forceinline__ double red_op(double a, double b) {
  return MAX ? gt_max(a, b) : a + b;
}

// Sum over the 16 lanes of each row (16-lane group), the same bits on every lane of the row:
// partners lane^1, lane^2 (quad_perm), lane^7 (row_half_mirror), lane^15 (row_mirror); each
// step adds a pair of equal partial sums in both orders, and IEEE addition commutes.
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_d<kDppXor1>(v);
  v += dpp_d<kDppXor2>(v);
  v += dpp_d<kDppHalfMirror>(v);
  v += dpp_d<kDppMirror>(v);
  return v;
}
// Maximum over each 16-lane row, on every lane of the row (the same DPP partners).
__device__ __forceinline__ int row16_max_i32(int v) {
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppXor1, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppXor2, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppHalfMirror, 0xf, 0xf, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppMirror, 0xf, 0xf, true));
  return v;
}
// Whole-wave sum or maximum: within each 16-lane row by DPP, then across rows with the permlane
// swaps.  Every lane ends with the same bits.
template <bool MAX>
__device__ __forceinline__ double wave_allreduce(double v) {
  v = red_op<MAX>(v, dpp_d<kDppXor1>(v));
  v = red_op<MAX>(v, dpp_d<kDppXor2>(v));
  v = red_op<MAX>(v, dpp_d<kDppHalfMirror>(v));
  v = red_op<MAX>(v, dpp_d<kDppMirror>(v));
  double w = v;
  swap16(v, w);
  v = red_op<MAX>(v, w);
  w = v;
  swap32(v, w);
  return red_op<MAX>(v, w);
}
__device__ __forceinline__ float wave_maxf(float v) {
  v = gt_maxf(v, dpp_f<kDppXor1>(v));
  v = gt_maxf(v, dpp_f<kDppXor2>(v));
  v = gt_maxf(v, dpp_f<kDppHalfMirror>(v));
  v = gt_maxf(v, dpp_f<kDppMirror>(v));
  float w = v;
  swap16f(v, w);
  v = gt_maxf(v, w);
  w = v;
  swap32f(v, w);
  return gt_maxf(v, w);
}

}  // namespace scde
