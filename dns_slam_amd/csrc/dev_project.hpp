// "Does pose k see point p": the pose tile and the pinhole projection of kf_project_kernel (mesh.hip), kf_pair_kernel
// (mesh_feature.hip), frustum_seen_kernel (mesh_eval.hip), views_see_any_kernel (mesh_raster.hip) and the point-mask kernels
// (mesh_masks.hip).  Their agreement is part of
// the result (labels and codes pick the same keyframes; views_see_any is frustum_seen per pose), so the expressions exist here
// and nowhere else.  Each kernel keeps its own loop over the tiles, its tile size and its exits.
// project(): cam = w2c @ [p, 1], x *= -1, K @ cam, z = cam.z + eps, (u, v) = uv / z, in fp32.  Two conventions:
//   meshing     (get_2d_feature / point_masks, reference slams/meshing.py:319-335 and 210-220): eps = 1e-8;
//               inside iff u < W, u > 0, v < H, v > 0, z < 0; the pixel read is round-half-even(u, v) clamped to the image;
//               point_masks' forecast frustum: the same with the image widened by 1000 px on every side.
//   evaluation  (check_proj, reference eval_3d.py:78-87 / cull_mesh.py:53-74): eps = 1e-5;
//               inside iff 0 <= -z, u < W, u > 0, v < H, v > 0.
// Every translation unit that includes this header must be compiled with -ffp-contract=off (Makefile): one rounding per
// operation, in the order written, is what makes the four kernels -- and the restatements in tests/ -- the same bits.
#pragma once
#include "common.hpp"
namespace dns {
constexpr float PROJ_EPS_MESHING = 1e-8f, PROJ_EPS_EVAL = 1e-5f;
struct Projected { float u, v, z, czw; };                          // czw: the camera-space z before eps
// point p of pts [P,3]; the origin for a thread without a point
__device__ __forceinline__ float3 load_point3(const float* __restrict__ pts, uint32_t p, bool live) {
  float3 q = make_float3(0.f, 0.f, 0.f);
  if (live) q.x = pts[3 * (size_t)p], q.y = pts[3 * (size_t)p + 1], q.z = pts[3 * (size_t)p + 2];
  return q;
}
// Rows 0-2 of the poses lo .. lo + n - 1 of w2c [K,4,4] into s_w [12 * TILE]; the caller's __syncthreads() before and after.
template <int BLOCK>
__device__ __forceinline__ void stage_poses(float* s_w, const float* __restrict__ w2c, uint32_t lo, int n) {
  for (int x = threadIdx.x; x < n * 12; x += BLOCK) s_w[x] = w2c[(size_t)(lo + x / 12) * 16 + x % 12];
}
__device__ __forceinline__ Projected project(const float* m, float3 p, float fx, float fy, float cx, float cy, float eps) {
  const float cxw = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];               // m: one staged pose (12 floats)
  const float cyw = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
  const float czw = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
  Projected q;
  q.czw = czw;
  q.z = czw + eps;
  q.u = (fx * -cxw + cx * czw) / q.z;
  q.v = (fy * cyw + cy * czw) / q.z;
  return q;
}
__device__ __forceinline__ bool inside_meshing(const Projected& q, float fW, float fH) {
  return q.u < fW && q.u > 0.f && q.v < fH && q.v > 0.f && q.z < 0.f;
}
__device__ __forceinline__ bool inside_eval(const Projected& q, float fW, float fH) {
  return 0.f <= -q.z && q.u < fW && q.u > 0.f && q.v < fH && q.v > 0.f;
}
// meshing, point_masks' forecast frustum (reference slams/meshing.py:190-193, 224-227): the image widened by 1000 px on every side
__device__ __forceinline__ bool inside_forecast(const Projected& q, float fW, float fH) {
  return q.u < fW + 1000.f && q.u > -1000.f && q.v < fH + 1000.f && q.v > -1000.f && q.z < 0.f;
}
// meshing: the pixel a point reads, along one axis of `size` pixels
__device__ __forceinline__ int round_pixel(float u, int size) { return min(max((int)rintf(u), 0), size - 1); }
}  // namespace dns
