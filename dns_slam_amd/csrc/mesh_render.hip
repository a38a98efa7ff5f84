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
// rm_init, rm_setup and rm_large are dev_raster.hpp's draw kernels with the key sink (id = the face index; timed as rm_*_kernel):
//   rm_init:    keys set to all ones, the list counters and the status words cleared.
//   rm_setup:   thread = (triangle, view): boxes up to RS_SMALL by the thread, the others to the list.
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

constexpr uint64_t RM_EMPTY = RsKeySink::EMPTY;
constexpr uint32_t RM_POINT = 0x80000000u;

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
    for (int j = ja; j <= jb; ++j) RsKeySink::merge(img + (size_t)i * (size_t)cam.W + (size_t)j, pz, RM_POINT | p);
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
  if (t0 == 0) status[1] = rs_list_total(counters, n_counters);
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
  const uint32_t known = DNS_RASTER_SIMPLE | DNS_RASTER_STATS | DNS_RENDER_CULL_BACK | DNS_RENDER_CULL_FRONT | DNS_RENDER_HEADLIGHT;
  DNS_REQUIRE((flags & ~known) == 0u, "dns_render_mesh: unknown flags %#x", flags);
  DNS_REQUIRE(!((flags & DNS_RENDER_CULL_BACK) && (flags & DNS_RENDER_CULL_FRONT)), "dns_render_mesh: both culling flags are set");
  DNS_REQUIRE(point_size >= 1 && point_size <= 16, "dns_render_mesh: point_size %u (must be 1..16)", point_size);
  DNS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "dns_render_mesh: ambient %g (must be in [0, 1])", (double)ambient);
  RsCam cam;
  RsCut cut;
  if (const int e = rs_check("dns_render_mesh", P, F, V, H, W, intr, z_near, z_far, list_cap, &cam, &cut)) return e;
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(w2c && ws && color && depth && index && status && background, "dns_render_mesh: NULL argument");
  DNS_REQUIRE(F == 0 || (verts && faces && colors), "dns_render_mesh: F > 0 needs verts, faces and colors");
  DNS_REQUIRE(N == 0 || (points && point_colors), "dns_render_mesh: N > 0 needs points and point_colors");
  hipStream_t st = (hipStream_t)stream;
  const size_t n_pix = (size_t)V * H * W;
  RsWs w;
  rs_layout(ws, n_pix, F, V, &w);
  rs_draw<RsKeySink>(verts, P, faces, F, w2c, V, cam, flags, cut, w, w.keys, status, st);
  for (uint32_t v_lo = 0; N && v_lo < V; v_lo += 65535u)
    DNS_LAUNCH(rm_points_kernel, dim3((N + RS_BLOCK - 1) / RS_BLOCK, std::min(65535u, V - v_lo)), dim3(RS_BLOCK), 0, st, points, N, w2c,
               v_lo, cam, (int)point_size, w.keys, status);
  const RmShade sh = {ambient, {background[0], background[1], background[2]}};
  DNS_LAUNCH(rm_shade_kernel, dim3(rs_fill_grid(n_pix)), dim3(RS_BLOCK), 0, st, verts, P, faces, F, colors, point_colors, N, w2c, cam, flags, sh,
             (const uint64_t*)w.keys, n_pix, (const uint32_t*)w.counters, (uint32_t)cut.n_launch, color, depth, index, status);
  return check_launch("dns_render_mesh");
}
