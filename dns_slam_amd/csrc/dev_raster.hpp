// The homogeneous rasteriser, spelt once for the depth rasteriser (mesh_raster.hip: dns_rasterize_depth) and the colour rasteriser
// (mesh_render.hip: dns_render_mesh): the triangle set-up and the per-pixel expressions, the draw path built on them (the bodies of
// the init, set-up and large-box kernels, written against a pixel sink -- the merge of (depth, face) into a pixel is the one place
// where the two units differ) and, at the end, the host side: the workspace, the cut into launches, the shared checks and the
// walk that launches a unit's kernels.  The rule is written out at the top of mesh_raster.hip and in include/dns_hip.h;
// tests/raster_ref.py restates it.  Every translation unit that includes this file is compiled with -ffp-contract=off (Makefile):
// every operation below is one fp32 rounding in the order written, so the two units compute the same bits for the same
// (triangle, view, pixel) -- the depth image of dns_render_mesh is dns_rasterize_depth's.  tools/raster_host_check.cpp drives the
// draw path on the host under ASan and UBSan (no barriers, no cross-lane operations: plain loops over blocks and threads).
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

// ---- the draw path --------------------------------------------------------------------------------------------------------
// A pixel sink: the word of its image, the word of a pixel nothing covers, the merge of (depth d > 0, face id) into a pixel,
// whether it culls (a compile-time property: the depth instantiation holds no cull test, its wrapper refuses the flags) and the
// names dns_kernel_timing reports its three draw kernels under.
struct RsDepthSink {                                             // the minimum of the depth bits
  using Word = uint32_t;
  static constexpr Word EMPTY = 0x7f800000u;                     // +inf
  static constexpr bool CULLS = false;
  static constexpr const char *INIT = "rs_init_kernel", *SETUP = "rs_setup_kernel", *LARGE = "rs_large_kernel";
  static __device__ __forceinline__ void merge(Word* p, float d, uint32_t) {
    const uint32_t bits = __float_as_uint(d);
    if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, bits);
  }
};

struct RsKeySink {                                               // the minimum of (depth bits << 32) | id
  using Word = uint64_t;
  static constexpr Word EMPTY = ~0ull;
  static constexpr bool CULLS = true;
  static constexpr const char *INIT = "rm_init_kernel", *SETUP = "rm_setup_kernel", *LARGE = "rm_large_kernel";
  static __device__ __forceinline__ void merge(Word* __restrict__ p, float d, uint32_t id) {
    const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)id;
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin((unsigned long long*)p, (unsigned long long)key);
  }
  static __device__ __forceinline__ bool culled(const RsTri& t, uint32_t flags) {
    if (flags & DNS_RENDER_CULL_BACK) return !(t.num < 0.f);
    if (flags & DNS_RENDER_CULL_FRONT) return !(t.num > 0.f);
    return false;
  }
};

// Pixel (row i, column j) of the image img [H,W] under face f; 0 <= i < H and 0 <= j < W by the caller's box.
template <class Sink>
__device__ __forceinline__ void rs_pixel(const RsTri& t, const RsCam& cam, int i, int j, uint32_t f,
                                         typename Sink::Word* __restrict__ img) {
  float d;
  if (rs_depth(t, cam, i, j, d)) Sink::merge(img + (size_t)i * (size_t)cam.W + (size_t)j, d, f);
}

// Init: the image set to the sink's empty word, the list counters and the status words cleared.
template <class Sink>
__global__ __launch_bounds__(RS_BLOCK) void rs_draw_init(typename Sink::Word* __restrict__ img, size_t n_words,
                                                         uint32_t* __restrict__ counters, uint32_t n_counters,
                                                         uint32_t* __restrict__ status) {
  const size_t t0 = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * RS_BLOCK;
  for (size_t i = t0; i < n_words; i += stride) img[i] = Sink::EMPTY;
  for (size_t i = t0; i < n_counters; i += stride) counters[i] = 0u;
  if (t0 < 4) status[t0] = 0u;
}

// Set-up: thread = (triangle f_lo + x, view v_lo + blockIdx.y); draws a small box itself, appends every other to the list.
template <class Sink>
__global__ __launch_bounds__(RS_BLOCK) void rs_draw_setup(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                          uint32_t f_lo, uint32_t f_hi, const float* __restrict__ w2c, uint32_t v_lo,
                                                          RsCam cam, uint32_t flags, uint64_t* __restrict__ list, uint32_t cap,
                                                          uint32_t* __restrict__ counter, typename Sink::Word* __restrict__ image,
                                                          uint32_t* __restrict__ status) {
  const uint32_t f = f_lo + blockIdx.x * RS_BLOCK + threadIdx.x, view = v_lo + blockIdx.y;
  if (f >= f_hi) return;
  RsTri t;
  if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status)) return;
  if constexpr (Sink::CULLS)
    if (Sink::culled(t, flags)) return;
  typename Sink::Word* img = image + (size_t)view * (size_t)cam.H * (size_t)cam.W;
  const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
  if (flags & DNS_RASTER_SIMPLE) {
    for (int i = t.y0; i <= t.y1; ++i)
      for (int j = t.x0; j <= t.x1; ++j) rs_pixel<Sink>(t, cam, i, j, f, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else if (bw <= RS_SMALL && bh <= RS_SMALL) {
    for (int a = 0; a < RS_SMALL; ++a)
      for (int b = 0; b < RS_SMALL; ++b)
        if (a < bh && b < bw) rs_pixel<Sink>(t, cam, t.y0 + a, t.x0 + b, f, img);
    if (flags & DNS_RASTER_STATS) atomicAdd(&status[2], 1u);
  } else {
    const uint32_t pos = atomicAdd(counter, 1u);
    if (pos < cap) list[pos] = ((uint64_t)view << 32) | (uint64_t)f;      // cap >= the pairs of this launch: always
  }
}

// Large boxes: a fixed grid; one workgroup per list entry repeats the set-up (the same expressions, so the same bits; culled pairs
// never reach the list) and walks the box RS_BLOCK pixels at a time.
template <class Sink>
__global__ __launch_bounds__(RS_BLOCK) void rs_draw_large(const float* __restrict__ verts, uint32_t P, const int32_t* __restrict__ faces,
                                                          uint32_t F, const float* __restrict__ w2c, uint32_t V, RsCam cam,
                                                          const uint64_t* __restrict__ list, uint32_t cap,
                                                          const uint32_t* __restrict__ counter, typename Sink::Word* __restrict__ image,
                                                          uint32_t* __restrict__ status) {
  const uint32_t n = min(*counter, cap);
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint64_t ent = list[e];
    const uint32_t f = (uint32_t)ent, view = (uint32_t)(ent >> 32);
    if (f >= F || view >= V) continue;
    RsTri t;
    if (!rs_setup(verts, P, faces, f, w2c + (size_t)view * 16, cam, t, status)) continue;
    typename Sink::Word* img = image + (size_t)view * (size_t)cam.H * (size_t)cam.W;
    const uint32_t bw = (uint32_t)(t.x1 - t.x0 + 1), area = bw * (uint32_t)(t.y1 - t.y0 + 1);
    for (uint32_t p = threadIdx.x; p < area; p += RS_BLOCK) rs_pixel<Sink>(t, cam, t.y0 + (int)(p / bw), t.x0 + (int)(p % bw), f, img);
  }
}

// (triangle, view) pairs drawn through the list: the sum of the n launches' counters, for status[1].
__device__ __forceinline__ uint32_t rs_list_total(const uint32_t* __restrict__ counters, uint32_t n) {
  uint32_t s = 0;
  for (uint32_t k = 0; k < n; ++k) s += counters[k];
  return s;
}

// ---- the host side ----------------------------------------------------------------------------------------------------------
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

// The checks both launch wrappers make, under the caller's name; DNS_OK with V == 0 before anything is read through intr.
// -> the camera and the cut of rs_draw.
inline int rs_check(const char* who, uint32_t P, uint32_t F, uint32_t V, uint32_t H, uint32_t W, const float* intr, float z_near,
                    float z_far, uint32_t list_cap, RsCam* cam, RsCut* cut) {
  DNS_REQUIRE(F < (1u << 31) && P < (1u << 31), "%s: %u vertices, %u faces (must be < 2^31)", who, P, F);
  DNS_REQUIRE(H > 0 && W > 0 && H <= 32768u && W <= 32768u, "%s: image %u x %u", who, H, W);
  DNS_REQUIRE(z_near > 0.f && z_far >= z_near && z_far <= 3.0e38f, "%s: z_near %g, z_far %g (need 0 < z_near <= z_far, finite)", who,
              (double)z_near, (double)z_far);
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(intr, "%s: NULL argument", who);
  DNS_REQUIRE(intr[0] - intr[0] == 0.f && intr[1] - intr[1] == 0.f && intr[0] != 0.f && intr[1] != 0.f && intr[2] - intr[2] == 0.f &&
                  intr[3] - intr[3] == 0.f, "%s: intrinsics must be finite, fx and fy non-zero", who);
  *cut = rs_cut(F, V, list_cap);
  DNS_REQUIRE(cut->n_launch <= RS_MAX_LAUNCHES, "%s: list_cap %u cuts %u faces x %u views into %llu launches (at most %u)", who, list_cap,
              F, V, (unsigned long long)cut->n_launch, RS_MAX_LAUNCHES);
  *cam = {intr[0], intr[1], intr[2], intr[3], z_near, z_far, (int)H, (int)W};
  return DNS_OK;
}

// Workgroups of the kernels that stride over the n_words pixels of all views (init, and each unit's last pass).
inline uint32_t rs_fill_grid(size_t n_words) { return (uint32_t)std::min<size_t>(8192, (n_words + RS_BLOCK - 1) / RS_BLOCK); }

// The draw of F faces x V views into img [V,H,W]: the init launch, then per launch of the cut the set-up kernel and, without
// DNS_RASTER_SIMPLE, the large-box kernel, launch k with the list counter w.counters[k].
template <class Sink>
inline void rs_draw(const float* verts, uint32_t P, const int32_t* faces, uint32_t F, const float* w2c, uint32_t V, const RsCam& cam,
                    uint32_t flags, const RsCut& cut, const RsWs& w, typename Sink::Word* img, uint32_t* status, hipStream_t st) {
  const size_t n_words = (size_t)V * (size_t)cam.H * (size_t)cam.W;
  DNS_LAUNCH_AS(Sink::INIT, rs_draw_init<Sink>, dim3(std::max(rs_fill_grid(n_words), (uint32_t)((cut.n_launch + RS_BLOCK - 1) / RS_BLOCK))),
                dim3(RS_BLOCK), 0, st, img, n_words, w.counters, (uint32_t)cut.n_launch, status);
  uint32_t k = 0;
  for (uint32_t v_lo = 0; F && v_lo < V; v_lo += cut.g) {
    const uint32_t nv = std::min(cut.g, V - v_lo);
    for (uint32_t f_lo = 0; f_lo < F; f_lo += cut.r, ++k) {
      const uint32_t f_hi = std::min(F, f_lo + cut.r);
      DNS_LAUNCH_AS(Sink::SETUP, rs_draw_setup<Sink>, dim3((f_hi - f_lo + RS_BLOCK - 1) / RS_BLOCK, nv), dim3(RS_BLOCK), 0, st, verts, P, faces, f_lo,
                    f_hi, w2c, v_lo, cam, flags, w.list, cut.cap, w.counters + k, img, status);
      if (!(flags & DNS_RASTER_SIMPLE))
        DNS_LAUNCH_AS(Sink::LARGE, rs_draw_large<Sink>, dim3(RS_LARGE_GRID), dim3(RS_BLOCK), 0, st, verts, P, faces, F, w2c, V, cam,
                      (const uint64_t*)w.list, cut.cap, (const uint32_t*)(w.counters + k), img, status);
    }
  }
}

}  // namespace dns
