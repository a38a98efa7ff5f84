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
// The set-up and the per-pixel expressions are dev_raster.hpp's, shared with the colour rasteriser (mesh_render.hip).
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

constexpr uint32_t RS_INF = 0x7f800000u;

// Pixel (row i, column j) of the image img [H,W]; 0 <= i < H and 0 <= j < W by the caller's box.
__device__ __forceinline__ void rs_pixel(const RsTri& t, const RsCam& cam, int i, int j, uint32_t* __restrict__ img) {
  float d;
  if (rs_depth(t, cam, i, j, d)) {
    uint32_t* p = img + (size_t)i * (size_t)cam.W + (size_t)j;
    const uint32_t bits = __float_as_uint(d);
    if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, bits);
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rs_init_kernel(uint32_t* __restrict__ depth, size_t n_words, uint32_t* __restrict__ counters,
                                                           uint32_t n_counters, uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  for (size_t i = t0; i < n_words; i += stride) depth[i] = RS_INF;
  for (size_t i = t0; i < n_counters; i += stride) counters[i] = 0u;
  if (t0 < 4) status[t0] = 0u;
}

__global__ __launch_bounds__(RS_BLOCK) void rs_setup_kernel(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                            uint32_t f_lo, uint32_t f_hi, const float* __restrict__ w2c, uint32_t v_lo,
                                                            RsCam cam, uint32_t flags, uint64_t* __restrict__ list, uint32_t cap,
                                                            uint32_t* __restrict__ counter, uint32_t* __restrict__ depth,
                                                            uint32_t* __restrict__ status) {
  const uint32_t f = f_lo + blockIdx.x * RS_BLOCK + threadIdx.x, view = v_lo + blockIdx.y;
  if (f >= f_hi) return;
  RsTri t;
  if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status)) return;
  uint32_t* img = depth + (size_t)view * (size_t)cam.H * (size_t)cam.W;
  const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
  if (flags & DNS_RASTER_SIMPLE) {
    for (int i = t.y0; i <= t.y1; ++i)
      for (int j = t.x0; j <= t.x1; ++j) rs_pixel(t, cam, i, j, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else if (bw <= RS_SMALL && bh <= RS_SMALL) {
    for (int a = 0; a < RS_SMALL; ++a)
      for (int b = 0; b < RS_SMALL; ++b)
        if (a < bh && b < bw) rs_pixel(t, cam, t.y0 + a, t.x0 + b, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else {
    const uint32_t pos = atomicAdd(counter, 1u);
    if (pos < cap) list[pos] = ((uint64_t)view << 32) | (uint64_t)f;      // cap >= the pairs of this launch: always
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rs_large_kernel(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                            uint32_t F, const float* __restrict__ w2c, uint32_t V, RsCam cam,
                                                            const uint64_t* __restrict__ list, uint32_t cap,
                                                            const uint32_t* __restrict__ counter, uint32_t* __restrict__ depth,
                                                            uint32_t* __restrict__ status) {
  const uint32_t n = min(*counter, cap);
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint64_t ent = list[e];
    const uint32_t f = (uint32_t)ent, view = (uint32_t)(ent >> 32);
    if (f >= F || view >= V) continue;
    RsTri t;
    if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status)) continue;
    uint32_t* img = depth + (size_t)view * (size_t)cam.H * (size_t)cam.W;
    const uint32_t bw = (uint32_t)(t.x1 - t.x0 + 1), area = bw * (uint32_t)(t.y1 - t.y0 + 1);
    for (uint32_t p = threadIdx.x; p < area; p += RS_BLOCK) rs_pixel(t, cam, t.y0 + (int)(p / bw), t.x0 + (int)(p % bw), img);
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rs_finish_kernel(uint32_t* __restrict__ depth, size_t n_words, const uint32_t* __restrict__ counters,
                                                             uint32_t n_counters, uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  for (size_t i = t0; i < n_words; i += stride)
    if (depth[i] == RS_INF) depth[i] = 0u;
  if (t0 == 0) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < n_counters; ++k) s += counters[k];
    status[1] = s;
  }
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
  DNS_REQUIRE(F < (1u << 31) && P < (1u << 31), "dns_rasterize_depth: %u vertices, %u faces (must be < 2^31)", P, F);
  DNS_REQUIRE(H > 0 && W > 0 && H <= 32768u && W <= 32768u, "dns_rasterize_depth: image %u x %u", H, W);
  DNS_REQUIRE((flags & ~(DNS_RASTER_SIMPLE | DNS_RASTER_STATS)) == 0u, "dns_rasterize_depth: unknown flags %#x", flags);
  DNS_REQUIRE(z_near > 0.f && z_far >= z_near && z_far <= 3.0e38f, "dns_rasterize_depth: z_near %g, z_far %g (need 0 < z_near <= z_far, finite)",
              (double)z_near, (double)z_far);
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(intr && w2c && ws && depth && status, "dns_rasterize_depth: NULL argument");
  DNS_REQUIRE(F == 0 || (verts && faces), "dns_rasterize_depth: F > 0 needs verts and faces");
  DNS_REQUIRE(intr[0] - intr[0] == 0.f && intr[1] - intr[1] == 0.f && intr[0] != 0.f && intr[1] != 0.f && intr[2] - intr[2] == 0.f &&
                  intr[3] - intr[3] == 0.f, "dns_rasterize_depth: intrinsics must be finite, fx and fy non-zero");
  const auto [cap, r, g, n_launch] = rs_cut(F, V, list_cap);
  DNS_REQUIRE(n_launch <= RS_MAX_LAUNCHES, "dns_rasterize_depth: list_cap %u cuts %u faces x %u views into %llu launches (at most %u)",
              list_cap, F, V, (unsigned long long)n_launch, RS_MAX_LAUNCHES);
  hipStream_t st = (hipStream_t)stream;
  RsWs w;
  rs_layout(ws, 0, F, V, &w);
  uint32_t* img = (uint32_t*)depth;
  const size_t n_words = (size_t)V * H * W;
  const RsCam cam = {intr[0], intr[1], intr[2], intr[3], z_near, z_far, (int)H, (int)W};
  const uint32_t fill_grid = (uint32_t)std::min<size_t>(8192, (n_words + RS_BLOCK - 1) / RS_BLOCK);
  DNS_LAUNCH(rs_init_kernel, dim3(std::max(fill_grid, (uint32_t)((n_launch + RS_BLOCK - 1) / RS_BLOCK))), dim3(RS_BLOCK), 0, st, img,
             n_words, w.counters, (uint32_t)n_launch, status);
  uint32_t k = 0;
  for (uint32_t v_lo = 0; F && v_lo < V; v_lo += g) {
    const uint32_t nv = std::min(g, V - v_lo);
    for (uint32_t f_lo = 0; f_lo < F; f_lo += r, ++k) {
      const uint32_t f_hi = std::min(F, f_lo + r);
      DNS_LAUNCH(rs_setup_kernel, dim3((f_hi - f_lo + RS_BLOCK - 1) / RS_BLOCK, nv), dim3(RS_BLOCK), 0, st, verts, P, faces, f_lo, f_hi,
                 w2c, v_lo, cam, flags, w.list, cap, w.counters + k, img, status);
      if (!(flags & DNS_RASTER_SIMPLE))
        DNS_LAUNCH(rs_large_kernel, dim3(RS_LARGE_GRID), dim3(RS_BLOCK), 0, st, verts, P, faces, F, w2c, V, cam, (const uint64_t*)w.list,
                   cap, (const uint32_t*)(w.counters + k), img, status);
    }
  }
  DNS_LAUNCH(rs_finish_kernel, dim3(fill_grid), dim3(RS_BLOCK), 0, st, img, n_words, (const uint32_t*)w.counters, (uint32_t)n_launch, status);
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
