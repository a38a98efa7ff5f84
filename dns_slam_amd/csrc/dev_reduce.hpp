// Wave sum and maximum, workgroup scan and carry scan of the mesh and evaluation kernels (mesh, mesh_cc, mesh_holes, mesh_eval,
// mesh_raster, mesh_render, mesh_masks, tsdf, hull, vis_panels); brings ws_carve.hpp, the HIP-free workspace alignment and carver
// their launch wrappers lay workspaces out with, and SCAN_THREADS.
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
// Two counts that are summed and scanned together.
template <class T>
struct Counts2 {
  T a, b;
  __device__ Counts2& operator+=(const Counts2& o) { return a += o.a, b += o.b, *this; }
};
// The carry scan of a count -> scan -> emit pass, called by one workgroup of SCAN_THREADS with s [SCAN_THREADS] in LDS: thread t
// sums its contiguous run of the workgroup counts bcount [n_blocks][2], the run sums are scanned, and every entry of the run
// gets its exclusive prefix in bpre [n_blocks][2].  Returns the scan's value: in the last thread the two totals.
template <class T>
__device__ __forceinline__ Counts2<T> carry_scan(Counts2<T>* s, const uint32_t* bcount, T* bpre, uint32_t n_blocks) {
  const uint32_t per = (n_blocks + SCAN_THREADS - 1) / SCAN_THREADS;
  const uint32_t b0 = (uint32_t)min((uint64_t)threadIdx.x * per, (uint64_t)n_blocks), b1 = min(b0 + per, n_blocks);
  Counts2<T> own{0, 0};
  for (uint32_t b = b0; b < b1; ++b) own.a += bcount[2 * b], own.b += bcount[2 * b + 1];
  const Counts2<T> incl = block_scan_inclusive<SCAN_THREADS>(s, own);
  T pa = incl.a - own.a, pb = incl.b - own.b;
  for (uint32_t b = b0; b < b1; ++b) {
    bpre[2 * b] = pa, bpre[2 * b + 1] = pb;
    pa += bcount[2 * b], pb += bcount[2 * b + 1];
  }
  return incl;
}
}  // namespace dns
