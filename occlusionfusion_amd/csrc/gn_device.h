// Gauss-Newton solver, device helpers that more than one of the gn*.hip files uses (every one __forceinline__ or a
// template; no kernel lives here): the reductions. Design: gn_internal.h.
#pragma once

#include "gn_internal.h"

namespace ofx {

// ---------------------------------------------------------------------------- reductions
template <int CTL>
__device__ __forceinline__ double dpp_mov(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// Sum over each aligned 16-lane row; every lane of the row ends with identical bits.
__device__ __forceinline__ double row16_sum(double x) {
  x += dpp_mov<0xB1>(x);    // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E>(x);    // quad_perm [2,3,0,1]
  x += dpp_mov<0x141>(x);   // row_half_mirror
  x += dpp_mov<0x140>(x);   // row_mirror
  return x;
}
__device__ __forceinline__ double read_lane(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}
// x from the lanes selected by a broadcast DPP control into the rows of row_mask (0 elsewhere)
template <int CTL, int ROWS>
__device__ __forceinline__ double dpp_bcast(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTL, ROWS, 0xF, false);
  return __hiloint2double(hi, lo);
}
// Full-wave sum, fixed order, uniform result. Call from wave-uniform control flow. After the 16-lane row sums r0..r3,
// row_bcast:15 adds row 0 into row 1 and row 2 into row 3, row_bcast:31 adds row 1 into row 3, whose lane 63 then
// holds (r3 + r2) + (r1 + r0) — bitwise the (r0 + r1) + (r2 + r3) of reading four lanes (f64 addition commutes
// exactly), in 2 DPP adds and one lane read instead of 4 lane reads, 2 moves back to VGPRs and 3 adds.
__device__ __forceinline__ double wave_sum(double x) {
  x = row16_sum(x);
  x += dpp_bcast<0x142, 0xA>(x);   // row_bcast:15 into rows 1, 3
  x += dpp_bcast<0x143, 0x8>(x);   // row_bcast:31 into row 3
  return read_lane(x, 63);
}
// four block sums at once: fixed-order wave sums, then the kBlk/64 wave results combined in wave order
__device__ __forceinline__ void block_sum4(double v[4]) {
  __shared__ double s4[kBlk / 64][4];
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) s4[w][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < kBlk / 64; ++q) a += s4[q][k];
    v[k] = a;
  }
}
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double s[kBlk];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if (threadIdx.x < (unsigned)o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  double r = s[0];
  __syncthreads();
  return r;
}

// Sum of p[i*stride + off], i < n, in a fixed order; every thread of the WG gets the same bits.
__device__ __forceinline__ double wg_sum_fixed(const double* __restrict__ p, int n, int stride, int off) {
  __shared__ double s_res;
  if (threadIdx.x < 64) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) acc += p[(int64_t)i * stride + off];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (threadIdx.x == 0) s_res = acc;
  }
  __syncthreads();
  double r = s_res;
  __syncthreads();
  return r;
}

}  // namespace ofx
