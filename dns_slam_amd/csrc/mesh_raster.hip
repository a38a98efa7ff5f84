// Depth L1 (the reference's eval_3d.py:120-210, calc_2d_metric): a triangle mesh to depth images, the mean absolute difference
// of two depth stacks, and the per-pose frustum test of the view sampler.
//
// dns_rasterize_depth: depth [V,H,W] of a mesh seen from V poses, by homogeneous rasterisation: no triangle is ever clipped.
// Compiled with -ffp-contract=off; every operation below is one fp32 rounding, in the order written.
//   camera space    v = ((r0 x + r1 y) + r2 z) + t per row of w2c
//   pixel ray       d = ((j - cx) / fx, (i - cy) / fy, 1) for pixel (row i, column j)
//   edge functions  for the edges (0,1), (1,2), (2,0) of the face: with the edge's two vertices ordered by vertex INDEX, a < b,
//                   c = v_a x v_b (c.x = a.y b.z - a.z b.y, c.y = a.z b.x - a.x b.z, c.z = a.x b.y - a.y b.x), negated when
//                   the winding runs from b to a; E = (d.x c.x + d.y c.y) + c.z.  Two triangles that share an edge evaluate
//                   the same fp32 number there (up to the sign), so no pixel centre falls between them.
//   coverage        all three E >= 0 or all three E <= 0 (both faces are drawn, the test is inclusive)
//   depth           e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 (components as for c), num = (n.x v0.x + n.y v0.y) + n.z v0.z,
//                   den = (n.x d.x + n.y d.y) + n.z, t = num / den; accepted when z_near <= t <= z_far, which also rejects
//                   the mirror image of a triangle that reaches behind the camera (t < 0) and den = 0
//   result          the minimum of t over the accepting triangles: the bit pattern of a positive float orders as an unsigned
//                   integer, the image starts at +inf and is merged with atomicMin; a last pass turns +inf into 0.  A minimum
//                   does not depend on the order: the image is the same bits for every call and both methods.
// A triangle with a non-finite vertex (world or camera space) is skipped and flagged; one with n = 0 is skipped.
//
// The set-up, the per-pixel expressions, the kernels rs_init, rs_setup and rs_large (rs_draw_init, rs_draw_setup, rs_draw_large
// with the depth sink, timed as rs_*_kernel) and the host walk over them are dev_raster.hpp's, shared with mesh_render.hip.
//   rs_init:    the image set to +inf, the list counters and the status words cleared.
//   rs_setup:   thread = (triangle, view).  Camera space, normal, edge vectors; culled when wholly nearer than z_near, beyond
//               z_far or outside one of the four side planes of the image (tested as half-spaces of camera space, with a pixel
//               of slack, so valid for triangles that cross z = 0).  With all three vertices at or beyond z_near the pixel
//               box of the projected vertices, one pixel of slack each side, clamped to the image; otherwise the whole
//               image.  A box of at most RS_SMALL x RS_SMALL pixels is rasterised by the thread; every other triangle is
//               appended to the list.  With DNS_RASTER_SIMPLE the thread rasterises every box itself (the timing baseline).
//   rs_large:   a fixed grid; reads the list's count from device memory; one workgroup per entry repeats the set-up (the same
//               expressions, so the same bits) and walks the box 256 pixels at a time.
//   rs_finish:  +inf -> 0, the list counts summed into status[1].
// The list holds the worst case: the host cuts (triangles x views) into launches of at most `cap` pairs (RS_LIST_CAP, or the
// caller's smaller list_cap) and the list has `cap` entries, so no pair is ever dropped and no thread falls back to a long loop.
//
// dns_depth_l1: err[v] = sum |a - b| / (H W) over all pixels in float64: DNS_DEPTH_L1_PARTS workgroups per view, each a strided
// sum, a butterfly over the wave and the waves in order; then one thread per view adds the parts in order.  No atomics.
//
// dns_views_see_any: frustum_seen_kernel (mesh_eval.hip) with the roles turned round, one flag per pose (dev_project.hpp).
#include <algorithm>
#include "common.hpp"
#include "dev_project.hpp"
#include "dev_raster.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

__global__ __launch_bounds__(RS_BLOCK) void rs_finish_kernel(uint32_t* __restrict__ depth, size_t n_words, const uint32_t* __restrict__ counters,
                                                             uint32_t n_counters, uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  for (size_t i = t0; i < n_words; i += stride)
    if (depth[i] == RsDepthSink::EMPTY) depth[i] = 0u;
  if (t0 == 0) status[1] = rs_list_total(counters, n_counters);
}

// ---- depth L1 --------------------------------------------------------------------------------------------------------------
constexpr int L1_BLOCK = 256;

__global__ __launch_bounds__(L1_BLOCK) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, uint64_t n_pix,
                                                              double* __restrict__ partial) {
  __shared__ double s_w[L1_BLOCK / WAVE];
  const uint32_t view = blockIdx.x / DNS_DEPTH_L1_PARTS, part = blockIdx.x % DNS_DEPTH_L1_PARTS;
  const float* __restrict__ pa = a + (size_t)view * n_pix;
  const float* __restrict__ pb = b + (size_t)view * n_pix;
  double s = 0.0;
  for (uint64_t p = (uint64_t)part * L1_BLOCK + threadIdx.x; p < n_pix; p += (uint64_t)DNS_DEPTH_L1_PARTS * L1_BLOCK)
    s += fabs((double)pa[p] - (double)pb[p]);
  s = wave_sum(s);
  if (threadIdx.x % WAVE == 0) s_w[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = s_w[0];
    for (int k = 1; k < L1_BLOCK / WAVE; ++k) v += s_w[k];
    partial[blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(L1_BLOCK) void l1_final_kernel(const double* __restrict__ partial, uint32_t V, uint64_t n_pix,
                                                            double* __restrict__ err) {
  const uint32_t v = blockIdx.x * L1_BLOCK + threadIdx.x;
  if (v >= V) return;
  double s = 0.0;
  for (uint32_t k = 0; k < DNS_DEPTH_L1_PARTS; ++k) s += partial[(size_t)v * DNS_DEPTH_L1_PARTS + k];
  err[v] = s / (double)n_pix;
}

// ---- per-pose frustum test ------------------------------------------------------------------------------------------------
constexpr int VS_BLOCK = 256, VS_TILE = 128;                     // poses per LDS tile (12 floats each)

__global__ __launch_bounds__(VS_BLOCK) void vs_clear_kernel(uint8_t* __restrict__ sees, uint32_t K) {
  const uint32_t k = blockIdx.x * VS_BLOCK + threadIdx.x;
  if (k < K) sees[k] = 0;
}

__global__ __launch_bounds__(VS_BLOCK) void views_see_any_kernel(const float* __restrict__ pts, uint32_t N, const float* __restrict__ w2c,
                                                                 uint32_t K, float fW, float fH, float fx, float fy, float cx, float cy,
                                                                 uint8_t* __restrict__ sees) {
  __shared__ float s_w[VS_TILE * 12];
  __shared__ uint32_t s_hit[VS_TILE];
  const uint32_t p = blockIdx.x * VS_BLOCK + threadIdx.x;
  const bool live = p < N;
  const float3 pt = load_point3(pts, p, live);
  for (uint32_t lo = 0; lo < K; lo += VS_TILE) {
    const int n = (int)min((uint32_t)VS_TILE, K - lo);
    __syncthreads();
    stage_poses<VS_BLOCK>(s_w, w2c, lo, n);
    if (threadIdx.x < VS_TILE) s_hit[threadIdx.x] = 0u;
    __syncthreads();
    if (live) {
      for (int kk = 0; kk < n; ++kk)                              // the evaluation convention; every writer stores the same value
        if (inside_eval(project(s_w + kk * 12, pt, fx, fy, cx, cy, PROJ_EPS_EVAL), fW, fH)) s_hit[kk] = 1u;
    }
    __syncthreads();
    if ((int)threadIdx.x < n && s_hit[threadIdx.x]) sees[lo + threadIdx.x] = 1;     // likewise across workgroups
  }
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_rasterize_ws_bytes(uint32_t F, uint32_t V, uint32_t H, uint32_t W) {
  if (F >= (1u << 31) || H == 0 || W == 0 || H > 32768u || W > 32768u) return 0;
  RsWs w;
  return rs_layout(nullptr, 0, F, V, &w);
}

extern "C" int dns_rasterize_depth(const float* verts, uint32_t P, const int32_t* faces, uint32_t F, const float* w2c, uint32_t V,
                                   uint32_t H, uint32_t W, const float* intr, float z_near, float z_far, uint32_t flags,
                                   uint32_t list_cap, void* ws, float* depth, uint32_t* status, void* stream) {
  DNS_REQUIRE((flags & ~(DNS_RASTER_SIMPLE | DNS_RASTER_STATS)) == 0u, "dns_rasterize_depth: unknown flags %#x", flags);
  RsCam cam;
  RsCut cut;
  if (const int e = rs_check("dns_rasterize_depth", P, F, V, H, W, intr, z_near, z_far, list_cap, &cam, &cut)) return e;
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(w2c && ws && depth && status, "dns_rasterize_depth: NULL argument");
  DNS_REQUIRE(F == 0 || (verts && faces), "dns_rasterize_depth: F > 0 needs verts and faces");
  hipStream_t st = (hipStream_t)stream;
  RsWs w;
  rs_layout(ws, 0, F, V, &w);
  uint32_t* img = (uint32_t*)depth;
  const size_t n_words = (size_t)V * H * W;
  rs_draw<RsDepthSink>(verts, P, faces, F, w2c, V, cam, flags, cut, w, img, status, st);
  DNS_LAUNCH(rs_finish_kernel, dim3(rs_fill_grid(n_words)), dim3(RS_BLOCK), 0, st, img, n_words, (const uint32_t*)w.counters,
             (uint32_t)cut.n_launch, status);
  return check_launch("dns_rasterize_depth");
}

extern "C" int dns_depth_l1(const float* a, const float* b, uint32_t V, uint32_t H, uint32_t W, double* partial, double* err,
                            void* stream) {
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(a && b && partial && err, "dns_depth_l1: NULL argument");
  DNS_REQUIRE(H > 0 && W > 0 && H <= 32768u && W <= 32768u, "dns_depth_l1: image %u x %u", H, W);
  DNS_REQUIRE(V <= (1u << 24), "dns_depth_l1: %u views (at most 2^24)", V);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n_pix = (uint64_t)H * W;
  DNS_LAUNCH(l1_partial_kernel, dim3(V * DNS_DEPTH_L1_PARTS), dim3(L1_BLOCK), 0, st, a, b, n_pix, partial);
  DNS_LAUNCH(l1_final_kernel, dim3((V + L1_BLOCK - 1) / L1_BLOCK), dim3(L1_BLOCK), 0, st, (const double*)partial, V, n_pix, err);
  return check_launch("dns_depth_l1");
}

extern "C" int dns_views_see_any(const float* pts, uint32_t N, const float* w2c, uint32_t K, int H, int W, const float* intr,
                                 uint8_t* sees, void* stream) {
  if (K == 0) return DNS_OK;
  DNS_REQUIRE(w2c && sees && intr, "dns_views_see_any: NULL argument");
  DNS_REQUIRE(N == 0 || pts, "dns_views_see_any: N > 0 needs pts");
  DNS_REQUIRE(N < (1u << 31), "dns_views_see_any: %u points (must be < 2^31)", N);
  DNS_REQUIRE(H > 0 && W > 0, "dns_views_see_any: image %d x %d", H, W);
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(vs_clear_kernel, dim3((K + VS_BLOCK - 1) / VS_BLOCK), dim3(VS_BLOCK), 0, st, sees, K);
  if (N)
    DNS_LAUNCH(views_see_any_kernel, dim3((N + VS_BLOCK - 1) / VS_BLOCK), dim3(VS_BLOCK), 0, st, pts, N, w2c, K, (float)W, (float)H,
               intr[0], intr[1], intr[2], intr[3], sees);
  return check_launch("dns_views_see_any");
}
