// The triangle set-up and the per-pixel expressions of the homogeneous rasteriser, spelt once for the depth rasteriser
// (mesh_raster.hip: dns_rasterize_depth) and the colour rasteriser (mesh_render.hip: dns_render_mesh).  The rule is written
// out at the top of mesh_raster.hip and in include/dns_hip.h; tests/raster_ref.py restates it.  Both units are compiled with
// -ffp-contract=off (Makefile): every operation below is one fp32 rounding in the order written, so the two kernels compute
// the same bits for the same (triangle, view, pixel) -- the depth image of dns_render_mesh is dns_rasterize_depth's.
// At the end, the host side the two launch wrappers share: the workspace parts they have in common and the cut into launches.
#pragma once
#include <algorithm>
#include "common.hpp"
#include "ws_carve.hpp"
namespace dns {

constexpr int RS_BLOCK = 256;
constexpr int RS_SMALL = 8;                                      // side of the largest box a set-up thread draws itself
constexpr uint32_t RS_LIST_CAP = 1u << 24;                       // (triangle, view) pairs per launch = list entries (128 MiB)
constexpr uint32_t RS_MAX_LAUNCHES = 65536;                      // list counters in the workspace
constexpr uint32_t RS_LARGE_GRID = 2048;

struct RsCam {
  float fx, fy, cx, cy, z_near, z_far;
  int H, W;
};

struct RsTri {
  float c[3][3];                                                 // signed edge vectors
  float n[3], num;
  int x0, x1, y0, y1;                                            // pixel box, inclusive
};

__device__ __forceinline__ void rs_cross(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// Row r of the pose m (16 floats) applied to the world point (x, y, z).
__device__ __forceinline__ float rs_camera(const float* __restrict__ m, int r, float x, float y, float z) {
  return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// The set-up of triangle f under the pose m (16 floats): false when there is nothing to draw.
__device__ __forceinline__ bool rs_setup(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces, uint32_t f,
                                         const float* __restrict__ m, const RsCam& cam, RsTri& t, uint32_t* __restrict__ status) {
  const uint32_t id[3] = {(uint32_t)faces[3 * (size_t)f], (uint32_t)faces[3 * (size_t)f + 1], (uint32_t)faces[3 * (size_t)f + 2]};
  if (id[0] >= P || id[1] >= P || id[2] >= P) {                   // never dereferenced; the ops wrapper refuses such a mesh
    atomicOr(&status[0], DNS_RASTER_BAD_INDEX);
    return false;
  }
  float v[3][3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = verts[3 * (size_t)id[k]], y = verts[3 * (size_t)id[k] + 1], z = verts[3 * (size_t)id[k] + 2];
    finite = finite && isfinite(x) && isfinite(y) && isfinite(z);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      v[k][r] = rs_camera(m, r, x, y, z);
      finite = finite && isfinite(v[k][r]);
    }
  }
  if (!finite) {
    atomicOr(&status[0], DNS_RASTER_NONFINITE);
    return false;
  }
  const float e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
  const float e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
  rs_cross(e1, e2, t.n);
  if (t.n[0] == 0.f && t.n[1] == 0.f && t.n[2] == 0.f) return false;
  t.num = (t.n[0] * v[0][0] + t.n[1] * v[0][1]) + t.n[2] * v[0][2];
  const float zmin = fminf(fminf(v[0][2], v[1][2]), v[2][2]), zmax = fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]);
  if (zmax < cam.z_near || zmin > cam.z_far) return false;
  // side planes with a pixel of slack: u = fx x / z + cx < -1 (left) or > W (right) for z > 0 are the half-spaces
  // fx x + (cx + 1) z < 0 and fx x + (cx - W) z > 0; a triangle wholly inside one has no visible point in the image
  const float fW = (float)cam.W, fH = (float)cam.H;
  bool left = true, right = true, top = true, bottom = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ax = cam.fx * v[k][0], ay = cam.fy * v[k][1], z = v[k][2];
    left = left && ax + (cam.cx + 1.f) * z < 0.f;
    right = right && ax + (cam.cx - fW) * z > 0.f;
    top = top && ay + (cam.cy + 1.f) * z < 0.f;
    bottom = bottom && ay + (cam.cy - fH) * z > 0.f;
  }
  if (left || right || top || bottom) return false;
  if (zmin >= cam.z_near) {
    float ulo = __builtin_inff(), uhi = -__builtin_inff(), vlo = ulo, vhi = uhi;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float u = cam.fx * (v[k][0] / v[k][2]) + cam.cx, w = cam.fy * (v[k][1] / v[k][2]) + cam.cy;
      ulo = fminf(ulo, u), uhi = fmaxf(uhi, u), vlo = fminf(vlo, w), vhi = fmaxf(vhi, w);
    }
    // clamped as floats first (a quotient may be huge or, overflowed, infinite); NaN cannot occur: the vertices are finite, z > 0
    t.x0 = (int)fminf(fmaxf(floorf(ulo) - 1.f, 0.f), fW);
    t.x1 = (int)fminf(fmaxf(ceilf(uhi) + 1.f, -1.f), fW - 1.f);
    t.y0 = (int)fminf(fmaxf(floorf(vlo) - 1.f, 0.f), fH);
    t.y1 = (int)fminf(fmaxf(ceilf(vhi) + 1.f, -1.f), fH - 1.f);
    if (t.x0 > t.x1 || t.y0 > t.y1) return false;
  } else {
    t.x0 = 0, t.x1 = cam.W - 1, t.y0 = 0, t.y1 = cam.H - 1;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = k, b = (k + 1) % 3;
    const bool swap = id[a] > id[b];                              // equal indices: n = 0, not reached
    rs_cross(v[swap ? b : a], v[swap ? a : b], t.c[k]);
    if (swap) t.c[k][0] = -t.c[k][0], t.c[k][1] = -t.c[k][1], t.c[k][2] = -t.c[k][2];
  }
  return true;
}

// Triangle t at pixel (row i, column j): the ray and the three edge functions; rs_den adds n . d.
struct RsSample {
  float dx, dy, E[3];
};

__device__ __forceinline__ void rs_sample(const RsTri& t, const RsCam& cam, int i, int j, RsSample& s) {
  s.dx = ((float)j - cam.cx) / cam.fx, s.dy = ((float)i - cam.cy) / cam.fy;
  s.E[0] = (s.dx * t.c[0][0] + s.dy * t.c[0][1]) + t.c[0][2];
  s.E[1] = (s.dx * t.c[1][0] + s.dy * t.c[1][1]) + t.c[1][2];
  s.E[2] = (s.dx * t.c[2][0] + s.dy * t.c[2][1]) + t.c[2][2];
}

__device__ __forceinline__ float rs_den(const RsTri& t, const RsSample& s) { return (t.n[0] * s.dx + t.n[1] * s.dy) + t.n[2]; }

// Coverage and depth of triangle t at the pixel: true when the pixel centre is covered and z_near <= d <= z_far (false for
// NaN; d > 0: its bits order as the value).
__device__ __forceinline__ bool rs_depth(const RsTri& t, const RsCam& cam, int i, int j, float& d) {
  RsSample s;
  rs_sample(t, cam, i, j, s);
  if (!((s.E[0] >= 0.f && s.E[1] >= 0.f && s.E[2] >= 0.f) || (s.E[0] <= 0.f && s.E[1] <= 0.f && s.E[2] <= 0.f))) return false;
  d = t.num / rs_den(t, s);
  return d >= cam.z_near && d <= cam.z_far;
}

inline uint64_t rs_list_entries(uint32_t F, uint32_t V, uint32_t cap) {
  return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)F * V, cap));
}

// The workspace of both rasterisers (host side; the kernels take its members).
struct RsWs {
  uint64_t* keys;                                                // [n_keys] dns_render_mesh: one per pixel and view
  uint32_t* counters;                                            // [RS_MAX_LAUNCHES] entries of each launch's list
  uint64_t* list;                                                // [rs_list_entries] (triangle, view) pairs
};

// Its parts into *w; returns its bytes (ws NULL: the size only).  n_keys 0 (dns_rasterize_depth): the counters come first.
inline size_t rs_layout(void* ws, uint64_t n_keys, uint32_t F, uint32_t V, RsWs* w) {
  WsCarve c(ws);
  w->keys = c.take<uint64_t>(n_keys);
  w->counters = c.take<uint32_t>(RS_MAX_LAUNCHES);
  w->list = c.take<uint64_t>(rs_list_entries(F, V, RS_LIST_CAP));
  return c.end256();
}

// F faces x V views cut into n_launch launches of r triangles x g views, r g <= cap (list_cap 0: RS_LIST_CAP).
struct RsCut {
  uint32_t cap, r, g;
  uint64_t n_launch;
};

inline RsCut rs_cut(uint32_t F, uint32_t V, uint32_t list_cap) {
  const uint32_t cap = list_cap ? std::min(list_cap, RS_LIST_CAP) : RS_LIST_CAP;
  const uint32_t r = std::max(1u, std::min(F, cap));
  const uint32_t g = std::min(std::min(V, 65535u), std::max(1u, cap / r));
  return {cap, r, g, F ? (uint64_t)((F + r - 1) / r) * ((V + g - 1) / g) : 0};
}

}  // namespace dns
