// The headless visualiser's rasteriser (the reference draws with open3d's window system, utils/viz.py:45-177): a triangle mesh
// with vertex colours and a point cloud to colour, depth and index images, V views at a time.
//
// dns_render_mesh.  Compiled with -ffp-contract=off; the triangle set-up, coverage and depth are dev_raster.hpp's, the
// expressions of dns_rasterize_depth (mesh_raster.hip), so the depth image is that function's, bit for bit.
//   visibility  one 64-bit key per pixel, (depth bits << 32) | id, merged with a 64-bit atomicMin behind a relaxed load and an
//               early-out.  id = the face index (< 2^31) for a triangle, 0x80000000 | point index for a point: the nearest
//               surface wins, at equal depth the lower face index, and a triangle beats a point.  A minimum does not depend on
//               the order: the images are the same bits for every call, launch split and method.
//   culling     per (face, view) by the sign of the set-up's num = n . v0: num < 0 is front-facing (the winding's normal points
//               at the camera).  DNS_RENDER_CULL_BACK drops num > 0, DNS_RENDER_CULL_FRONT drops num < 0, both drop num = 0.
//   points      camera space p = rs_camera (the triangles' transform); accepted when finite and z_near <= p.z <= z_far;
//               u = fx (p.x / p.z) + cx, w = fy (p.y / p.z) + cy; columns ceil(u - s/2) .. + s - 1 and rows ceil(w - s/2) ..
//               + s - 1 (the pixel centres in [u - s/2, u + s/2)), clipped to the image; key depth p.z.
//   shading     one thread per pixel reads the key.  Background: the background colour, depth 0, index -1.  Point: its colour,
//               index -2 - point.  Face: the set-up again (the same expressions), rs_sample at the pixel, weights
//               w0 = E[1] / S, w1 = E[2] / S, w2 = E[0] / S with S = (E[0] + E[1]) + E[2] (perspective-correct: the three
//               edge vectors sum to n, so den = n . d is the sum of the edge functions; the sum of the ROUNDED edge functions
//               is what keeps the weights a partition of one where a small, distant triangle leaves E few digits), colour =
//               (w0 c0 + w1 c1) + w2 c2 per channel; with DNS_RENDER_HEADLIGHT times ambient + (1 - ambient) (|den| /
//               (sqrt((n.x n.x + n.y n.y) + n.z n.z) * sqrt((d.x d.x + d.y d.y) + 1))): flat, two-sided.  Depth = the key's
//               depth bits.
//
//   rm_init:    keys set to all ones, the list counters and the status words cleared.
//   rm_setup:   thread = (triangle, view); as rs_setup_kernel: boxes up to RS_SMALL by the thread, the others to the list.
//   rm_large:   one workgroup per list entry, the box 256 pixels at a time.
//   rm_points:  thread = (point, view), its square of at most 16 x 16 pixels.
//   rm_shade:   thread = pixel; the list counts summed into status[1].
// Vector stores only; no atomics other than the key merge, the list cursor, the status word and the STATS count.
#include <algorithm>
#include "common.hpp"
#include "dev_raster.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

constexpr uint64_t RM_EMPTY = ~0ull;
constexpr uint32_t RM_POINT = 0x80000000u;

__device__ __forceinline__ void rm_merge(uint64_t* __restrict__ p, float d, uint32_t id) {
  const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)id;
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin((unsigned long long*)p, (unsigned long long)key);
}

// Pixel (row i, column j) of the key image img [H,W]; 0 <= i < H and 0 <= j < W by the caller's box.
__device__ __forceinline__ void rm_pixel(const RsTri& t, const RsCam& cam, int i, int j, uint32_t f, uint64_t* __restrict__ img) {
  float d;
  if (rs_depth(t, cam, i, j, d)) rm_merge(img + (size_t)i * (size_t)cam.W + (size_t)j, d, f);
}

__device__ __forceinline__ bool rm_culled(const RsTri& t, uint32_t flags) {
  if (flags & DNS_RENDER_CULL_BACK) return !(t.num < 0.f);
  if (flags & DNS_RENDER_CULL_FRONT) return !(t.num > 0.f);
  return false;
}

__global__ __launch_bounds__(RS_BLOCK) void rm_init_kernel(uint64_t* __restrict__ keys, size_t n_pix, uint32_t* __restrict__ counters,
                                                           uint32_t n_counters, uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  for (size_t i = t0; i < n_pix; i += stride) keys[i] = RM_EMPTY;
  for (size_t i = t0; i < n_counters; i += stride) counters[i] = 0u;
  if (t0 < 4) status[t0] = 0u;
}

__global__ __launch_bounds__(RS_BLOCK) void rm_setup_kernel(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                            uint32_t f_lo, uint32_t f_hi, const float* __restrict__ w2c, uint32_t v_lo,
                                                            RsCam cam, uint32_t flags, uint64_t* __restrict__ list, uint32_t cap,
                                                            uint32_t* __restrict__ counter, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ status) {
  const uint32_t f = f_lo + blockIdx.x * RS_BLOCK + threadIdx.x, view = v_lo + blockIdx.y;
  if (f >= f_hi) return;
  RsTri t;
  if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status) || rm_culled(t, flags)) return;
  uint64_t* img = keys + (size_t)view * (size_t)cam.H * (size_t)cam.W;
  const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
  if (flags & DNS_RASTER_SIMPLE) {
    for (int i = t.y0; i <= t.y1; ++i)
      for (int j = t.x0; j <= t.x1; ++j) rm_pixel(t, cam, i, j, f, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else if (bw <= RS_SMALL && bh <= RS_SMALL) {
    for (int a = 0; a < RS_SMALL; ++a)
      for (int b = 0; b < RS_SMALL; ++b)
        if (a < bh && b < bw) rm_pixel(t, cam, t.y0 + a, t.x0 + b, f, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else {
    const uint32_t pos = atomicAdd(counter, 1u);
    if (pos < cap) list[pos] = ((uint64_t)view << 32) | (uint64_t)f;      // cap >= the pairs of this launch: always
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rm_large_kernel(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                            uint32_t F, const float* __restrict__ w2c, uint32_t V, RsCam cam,
                                                            const uint64_t* __restrict__ list, uint32_t cap,
                                                            const uint32_t* __restrict__ counter, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ status) {
  const uint32_t n = min(*counter, cap);
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint64_t ent = list[e];
    const uint32_t f = (uint32_t)ent, view = (uint32_t)(ent >> 32);
    if (f >= F || view >= V) continue;
    RsTri t;
    if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status)) continue;       // culled pairs never reach the list
    uint64_t* img = keys + (size_t)view * (size_t)cam.H * (size_t)cam.W;
    const uint32_t bw = (uint32_t)(t.x1 - t.x0 + 1), area = bw * (uint32_t)(t.y1 - t.y0 + 1);
    for (uint32_t p = threadIdx.x; p < area; p += RS_BLOCK) rm_pixel(t, cam, t.y0 + (int)(p / bw), t.x0 + (int)(p % bw), f, img);
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rm_points_kernel(const float* __restrict__ pts, uint32_t N, const float* __restrict__ w2c,
                                                             uint32_t v_lo, RsCam cam, int size, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x, view = v_lo + blockIdx.y;
  if (p >= N) return;
  const float* __restrict__ m = w2c + (size_t)view * 16;
  const float x = pts[3 * (size_t)p], y = pts[3 * (size_t)p + 1], z = pts[3 * (size_t)p + 2];
  const float px = rs_camera(m, 0, x, y, z), py = rs_camera(m, 1, x, y, z), pz = rs_camera(m, 2, x, y, z);
  if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(px) && isfinite(py) && isfinite(pz))) {
    atomicOr(&status[0], DNS_RENDER_NONFINITE_POINT);
    return;
  }
  if (!(pz >= cam.z_near && pz <= cam.z_far)) return;
  const float half = (float)size * 0.5f;
  const float u = cam.fx * (px / pz) + cam.cx, w = cam.fy * (py / pz) + cam.cy;
  const float fj = ceilf(u - half), fi = ceilf(w - half);
  // compared as floats first: a quotient may be huge or, overflowed, infinite (then every comparison is false)
  if (!(fj <= (float)(cam.W - 1) && fj + (float)(size - 1) >= 0.f && fi <= (float)(cam.H - 1) && fi + (float)(size - 1) >= 0.f)) return;
  const int j0 = (int)fj, i0 = (int)fi;                          // within [-15, W - 1] and [-15, H - 1]
  const int ja = max(j0, 0), jb = min(j0 + size - 1, cam.W - 1), ia = max(i0, 0), ib = min(i0 + size - 1, cam.H - 1);
  uint64_t* img = keys + (size_t)view * (size_t)cam.H * (size_t)cam.W;
  for (int i = ia; i <= ib; ++i)
    for (int j = ja; j <= jb; ++j) rm_merge(img + (size_t)i * (size_t)cam.W + (size_t)j, pz, RM_POINT | p);
}

struct RmShade {
  float ambient, bg[3];
};

__global__ __launch_bounds__(RS_BLOCK) void rm_shade_kernel(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                            uint32_t F, const float* __restrict__ colors,
                                                            const float* __restrict__ point_colors, uint32_t N,
                                                            const float* __restrict__ w2c, RsCam cam, uint32_t flags, RmShade sh,
                                                            const uint64_t* __restrict__ keys, size_t n_pix,
                                                            const uint32_t* __restrict__ counters, uint32_t n_counters,
                                                            float* __restrict__ color, float* __restrict__ depth,
                                                            int32_t* __restrict__ index, uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  const size_t hw = (size_t)cam.H * (size_t)cam.W;
  for (size_t q = t0; q < n_pix; q += stride) {
    const uint64_t key = keys[q];
    const uint32_t id = (uint32_t)key;
    float rgb[3] = {sh.bg[0], sh.bg[1], sh.bg[2]}, d = 0.f;
    int32_t idx = -1;
    if (key != RM_EMPTY) {
      if (id & RM_POINT) {
        const uint32_t p = id & ~RM_POINT;
        if (p < N) {
          d = __uint_as_float((uint32_t)(key >> 32));
          idx = -2 - (int32_t)p;
          rgb[0] = point_colors[3 * (size_t)p], rgb[1] = point_colors[3 * (size_t)p + 1], rgb[2] = point_colors[3 * (size_t)p + 2];
        }
      } else if (id < F) {
        const size_t view = q / hw, r = q % hw;
        RsTri t;
        if (rs_setup(verts, P, faces, id, w2c + view * 16, cam, t, status)) {      // true: this face drew the pixel
          RsSample s;
          rs_sample(t, cam, (int)(r / (size_t)cam.W), (int)(r % (size_t)cam.W), s);
          const float den = rs_den(t, s);
          d = __uint_as_float((uint32_t)(key >> 32));
          idx = (int32_t)id;
          const float S = (s.E[0] + s.E[1]) + s.E[2];            // = den up to rounding; 0: all three E are 0, seen edge-on
          const float w0 = S != 0.f ? s.E[1] / S : 1.f, w1 = S != 0.f ? s.E[2] / S : 0.f, w2 = S != 0.f ? s.E[0] / S : 0.f;
          const size_t a = 3 * (size_t)(uint32_t)faces[3 * (size_t)id], b = 3 * (size_t)(uint32_t)faces[3 * (size_t)id + 1],
                       c = 3 * (size_t)(uint32_t)faces[3 * (size_t)id + 2];
          float light = 1.f;
          if (flags & DNS_RENDER_HEADLIGHT) {
            const float nn = (t.n[0] * t.n[0] + t.n[1] * t.n[1]) + t.n[2] * t.n[2], dd = (s.dx * s.dx + s.dy * s.dy) + 1.f;
            light = sh.ambient + (1.f - sh.ambient) * (fabsf(den) / (sqrtf(nn) * sqrtf(dd)));
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            rgb[k] = (w0 * colors[a + k] + w1 * colors[b + k]) + w2 * colors[c + k];
            if (flags & DNS_RENDER_HEADLIGHT) rgb[k] = rgb[k] * light;
          }
        }
      }
    }
    color[3 * q] = rgb[0], color[3 * q + 1] = rgb[1], color[3 * q + 2] = rgb[2];
    depth[q] = d;
    index[q] = idx;
  }
  if (t0 == 0) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < n_counters; ++k) s += counters[k];
    status[1] = s;
  }
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_render_mesh_ws_bytes(uint32_t F, uint32_t V, uint32_t H, uint32_t W) {
  if (F >= (1u << 31) || H == 0 || W == 0 || H > 32768u || W > 32768u) return 0;
  RsWs w;
  return rs_layout(nullptr, (uint64_t)V * H * W, F, V, &w);
}

extern "C" int dns_render_mesh(const float* verts, uint32_t P, const int32_t* faces, uint32_t F, const float* colors,
                               const float* points, const float* point_colors, uint32_t N, uint32_t point_size, const float* w2c,
                               uint32_t V, uint32_t H, uint32_t W, const float* intr, float z_near, float z_far, uint32_t flags,
                               float ambient, const float* background, uint32_t list_cap, void* ws, float* color, float* depth,
                               int32_t* index, uint32_t* status, void* stream) {
  DNS_REQUIRE(F < (1u << 31) && P < (1u << 31) && N < (1u << 31), "dns_render_mesh: %u vertices, %u faces, %u points (must be < 2^31)", P,
              F, N);
  DNS_REQUIRE(H > 0 && W > 0 && H <= 32768u && W <= 32768u, "dns_render_mesh: image %u x %u", H, W);
  const uint32_t known = DNS_RASTER_SIMPLE | DNS_RASTER_STATS | DNS_RENDER_CULL_BACK | DNS_RENDER_CULL_FRONT | DNS_RENDER_HEADLIGHT;
  DNS_REQUIRE((flags & ~known) == 0u, "dns_render_mesh: unknown flags %#x", flags);
  DNS_REQUIRE(!((flags & DNS_RENDER_CULL_BACK) && (flags & DNS_RENDER_CULL_FRONT)), "dns_render_mesh: both culling flags are set");
  DNS_REQUIRE(z_near > 0.f && z_far >= z_near && z_far <= 3.0e38f, "dns_render_mesh: z_near %g, z_far %g (need 0 < z_near <= z_far, finite)",
              (double)z_near, (double)z_far);
  DNS_REQUIRE(point_size >= 1 && point_size <= 16, "dns_render_mesh: point_size %u (must be 1..16)", point_size);
  DNS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "dns_render_mesh: ambient %g (must be in [0, 1])", (double)ambient);
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(intr && w2c && ws && color && depth && index && status && background, "dns_render_mesh: NULL argument");
  DNS_REQUIRE(F == 0 || (verts && faces && colors), "dns_render_mesh: F > 0 needs verts, faces and colors");
  DNS_REQUIRE(N == 0 || (points && point_colors), "dns_render_mesh: N > 0 needs points and point_colors");
  DNS_REQUIRE(intr[0] - intr[0] == 0.f && intr[1] - intr[1] == 0.f && intr[0] != 0.f && intr[1] != 0.f && intr[2] - intr[2] == 0.f &&
                  intr[3] - intr[3] == 0.f, "dns_render_mesh: intrinsics must be finite, fx and fy non-zero");
  const auto [cap, r, g, n_launch] = rs_cut(F, V, list_cap);
  DNS_REQUIRE(n_launch <= RS_MAX_LAUNCHES, "dns_render_mesh: list_cap %u cuts %u faces x %u views into %llu launches (at most %u)",
              list_cap, F, V, (unsigned long long)n_launch, RS_MAX_LAUNCHES);
  hipStream_t st = (hipStream_t)stream;
  const size_t n_pix = (size_t)V * H * W;
  RsWs w;
  rs_layout(ws, n_pix, F, V, &w);
  const RsCam cam = {intr[0], intr[1], intr[2], intr[3], z_near, z_far, (int)H, (int)W};
  const uint32_t fill_grid = (uint32_t)std::min<size_t>(8192, (n_pix + RS_BLOCK - 1) / RS_BLOCK);
  DNS_LAUNCH(rm_init_kernel, dim3(std::max(fill_grid, (uint32_t)((n_launch + RS_BLOCK - 1) / RS_BLOCK))), dim3(RS_BLOCK), 0, st, w.keys,
             n_pix, w.counters, (uint32_t)n_launch, status);
  uint32_t k = 0;
  for (uint32_t v_lo = 0; F && v_lo < V; v_lo += g) {
    const uint32_t nv = std::min(g, V - v_lo);
    for (uint32_t f_lo = 0; f_lo < F; f_lo += r, ++k) {
      const uint32_t f_hi = std::min(F, f_lo + r);
      DNS_LAUNCH(rm_setup_kernel, dim3((f_hi - f_lo + RS_BLOCK - 1) / RS_BLOCK, nv), dim3(RS_BLOCK), 0, st, verts, P, faces, f_lo, f_hi,
                 w2c, v_lo, cam, flags, w.list, cap, w.counters + k, w.keys, status);
      if (!(flags & DNS_RASTER_SIMPLE))
        DNS_LAUNCH(rm_large_kernel, dim3(RS_LARGE_GRID), dim3(RS_BLOCK), 0, st, verts, P, faces, F, w2c, V, cam, (const uint64_t*)w.list,
                   cap, (const uint32_t*)(w.counters + k), w.keys, status);
    }
  }
  for (uint32_t v_lo = 0; N && v_lo < V; v_lo += 65535u)
    DNS_LAUNCH(rm_points_kernel, dim3((N + RS_BLOCK - 1) / RS_BLOCK, std::min(65535u, V - v_lo)), dim3(RS_BLOCK), 0, st, points, N, w2c,
               v_lo, cam, (int)point_size, w.keys, status);
  const RmShade sh = {ambient, {background[0], background[1], background[2]}};
  DNS_LAUNCH(rm_shade_kernel, dim3(fill_grid), dim3(RS_BLOCK), 0, st, verts, P, faces, F, colors, point_colors, N, w2c, cam, flags, sh,
             (const uint64_t*)w.keys, n_pix, (const uint32_t*)w.counters, (uint32_t)n_launch, color, depth, index, status);
  return check_launch("dns_render_mesh");
}
