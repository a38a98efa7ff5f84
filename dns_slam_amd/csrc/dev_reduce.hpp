// Wave sum and maximum and workgroup scan of the mesh and evaluation kernels (mesh, mesh_cc, mesh_eval, mesh_raster,
// mesh_masks); brings ws_carve.hpp, the HIP-free workspace alignment and carver their launch wrappers lay workspaces out with.
#pragma once
#include "common.hpp"
#include "ws_carve.hpp"
namespace dns {
// The sum over the 64 lanes, in every lane; butterfly from 32 down to 1: in floating point this order decides the bits.
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
// The maximum over the 64 lanes, in every lane (order-independent).
template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T y = __shfl_xor(x, o);
    x = y > x ? y : x;
  }
  return x;
}
// Inclusive Hillis-Steele scan of one value per thread over a workgroup of exactly N threads, through s [N] in LDS: returns
// the sum of the values of threads 0 .. threadIdx.x.  T needs T{} = zero and +=.  Every thread of the workgroup calls it.
template <int N, class T>
__device__ __forceinline__ T block_scan_inclusive(T* s, T own) {
  const uint32_t t = threadIdx.x;
  s[t] = own;
  __syncthreads();
  for (uint32_t o = 1; o < N; o <<= 1) {
    const T a = t >= o ? s[t - o] : T{};
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  return s[t];
}
}  // namespace dns
