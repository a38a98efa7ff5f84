// The arithmetic of the point encoding, in one place: hash / dense row index, cell and fraction of a point on a level, the trilinear
// corner weights, the level gather with its Jacobian, the OneBlob kernel integrals (forward and backward of one axis) and the
// fp64 normalisation of a point.  Included by the encoder kernels (encode.hip), the table-gradient scatter (scatter.hip), which
// recomputes the cell, fraction and weights of every point and must land in the rows the forward read, and the fused tracker
// iteration (track_fused.inc, phases 1 and 7).  encode.hip and scatter.hip are compiled with -ffp-contract=off (value-exact arithmetic
// shared with oracle/tcnn_ref.py), the tracker's units are not: the functions whose results a contraction would change carry
// the same setting as a function-level pragma, so they give the same bits in every translation unit.
// Row arguments are a template parameter (RowP): the tracker passes explicit LDS address-space pointers (track_fused.inc, lds_fp).
#pragma once
#include "common.hpp"
#include "dev_rn.hpp"

namespace dns {

struct Bound6 {
  double b0[3];
  double inv_unused[3];
  double b1[3];
};

__device__ __forceinline__ uint32_t grid_row(uint32_t gx, uint32_t gy, uint32_t gz, uint32_t res,
                                             uint32_t size, uint32_t hashed) {
  uint32_t idx;
  if (hashed) {
    idx = gx ^ (gy * 2654435761u) ^ (gz * 805459861u);
    // hashed levels are exactly 2^T rows
    return idx & (size - 1u);
  }
  idx = gx + gy * res + gz * res * res;
  if (idx >= size) idx %= size;
  return idx;
}

// Cell and fraction of a point on a level.  The contract shared with oracle/tcnn_ref.py: pos = x * scale + 0.5 is two IEEE roundings
// (never contracted), the cell is (uint32)(int)floorf(pos).  The results are per axis; the order the axes are visited in only
// steers hipcc's SLP vectoriser.  From z down (the default) encode_fwd_kernel keeps 72 registers, from x up it packs (x1, x0) the
// wrong way round and needs 74 -- one occupancy step.  The fused tracker asks for X_FIRST: see grid_level.
template <bool X_FIRST = false>
__device__ __forceinline__ void grid_cell(const float x[3], float s, uint32_t g[3], float f[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int a = X_FIRST ? i : 2 - i;
    const float pos = DNS_FADD(DNS_FMUL(x[a], s), 0.5f);         // (dev_rn.hpp)
    const float fl = floorf(pos);
    g[a] = (uint32_t)(int)fl;
    f[a] = pos - fl;
  }
}

// trilinear weight of corner c (bit 0: x + 1, bit 1: y + 1, bit 2: z + 1)
__device__ __forceinline__ float corner_weight(const float f[3], uint32_t c) {
#pragma clang fp contract(off)
  return ((c & 1u) ? f[0] : 1.0f - f[0]) * ((c & 2u) ? f[1] : 1.0f - f[1]) * ((c & 4u) ? f[2] : 1.0f - f[2]);
}

// ... of the two corners of x-pair c (x, x + 1 at the same y, z; bit 0: y + 1, bit 1: z + 1), the (y, z) product formed once: the
// table scatter's form (its own rounding order, x * (y * z))
__device__ __forceinline__ void pair_weights(const float f[3], uint32_t c, float& w0, float& w1) {
#pragma clang fp contract(off)
  const float wyz = ((c & 1u) ? f[1] : 1.0f - f[1]) * ((c & 2u) ? f[2] : 1.0f - f[2]);
  w0 = (1.0f - f[0]) * wyz;
  w1 = f[0] * wyz;
}

// One level of the hash grid for one point: the 8-corner gather and its trilinear interpolation -> row[2 l], row[2 l + 1] (also
// returned).  dydx (may be null): d(feature) / d(normalised coordinate), both features, per axis -- what tcnn's kernel_grid keeps
// as dy_dx when the input needs a gradient (the poses do, through pts): the backward then needs no second gather of the 8 corners.
// Layout [level][axis][point] float2: a wave's 64 points are 512 contiguous bytes per store.
// JAC: the Jacobian is always kept (no null test); X_FIRST: grid_cell's axis order.  Both are the fused tracker's: its units are
// compiled WITH contraction, and which multiply-adds of the phases around this call fuse follows the vectoriser's packing of the
// whole kernel.  With <true, true> that kernel has the floating-point instruction mix, and run_fused the bits, that it had with
// a private copy of this function; with the null test, the z-first cell or both its count of fused multiply-adds changes (and,
// measured with both, the pose by an ulp).
template <bool JAC = false, bool X_FIRST = false, typename RowP>
__device__ __forceinline__ float2 grid_level(const float2* __restrict__ table, const GridLevels& lv, uint32_t l, const float (&x)[3],
                                             RowP row, float2* __restrict__ dydx, uint32_t P, uint32_t p) {
#pragma clang fp contract(off)
  const float s = lv.scale[l];
  const uint32_t res = lv.resolution[l], size = lv.size[l], hashed = lv.hashed[l];
  const float2* __restrict__ t = table + lv.offset[l];
  float f[3];
  uint32_t g[3];
  grid_cell<X_FIRST>(x, s, g, f);
  float2 v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = t[grid_row(g[0] + (c & 1), g[1] + ((c >> 1) & 1), g[2] + ((c >> 2) & 1), res, size, hashed)];
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float w = corner_weight(f, (uint32_t)c);
    a0 += w * v[c].x;
    a1 += w * v[c].y;
  }
  row[2 * l] = a0;
  row[2 * l + 1] = a1;
  if (JAC || dydx) {
    const float wx0 = 1.0f - f[0], wx1 = f[0], wy0 = 1.0f - f[1], wy1 = f[1], wz0 = 1.0f - f[2], wz1 = f[2];
    float2 jx, jy, jz;
    jx.x = s * (wy0 * wz0 * (v[1].x - v[0].x) + wy1 * wz0 * (v[3].x - v[2].x) + wy0 * wz1 * (v[5].x - v[4].x) + wy1 * wz1 * (v[7].x - v[6].x));
    jx.y = s * (wy0 * wz0 * (v[1].y - v[0].y) + wy1 * wz0 * (v[3].y - v[2].y) + wy0 * wz1 * (v[5].y - v[4].y) + wy1 * wz1 * (v[7].y - v[6].y));
    jy.x = s * (wx0 * wz0 * (v[2].x - v[0].x) + wx1 * wz0 * (v[3].x - v[1].x) + wx0 * wz1 * (v[6].x - v[4].x) + wx1 * wz1 * (v[7].x - v[5].x));
    jy.y = s * (wx0 * wz0 * (v[2].y - v[0].y) + wx1 * wz0 * (v[3].y - v[1].y) + wx0 * wz1 * (v[6].y - v[4].y) + wx1 * wz1 * (v[7].y - v[5].y));
    jz.x = s * (wx0 * wy0 * (v[4].x - v[0].x) + wx1 * wy0 * (v[5].x - v[1].x) + wx0 * wy1 * (v[6].x - v[2].x) + wx1 * wy1 * (v[7].x - v[3].x));
    jz.y = s * (wx0 * wy0 * (v[4].y - v[0].y) + wx1 * wy0 * (v[5].y - v[1].y) + wx0 * wy1 * (v[6].y - v[2].y) + wx1 * wy1 * (v[7].y - v[3].y));
    dydx[((size_t)l * 3 + 0) * P + p] = jx;
    dydx[((size_t)l * 3 + 1) * P + p] = jy;
    dydx[((size_t)l * 3 + 2) * P + p] = jz;
  }
  return make_float2(a0, a1);
}

// A non-finite coordinate must not leave as a finite row or gradient: fminf / fmaxf drop a NaN, so the clamp alone turned a NaN
// or +-Inf distance (r = NaN either way: Inf - Inf) into 0 and every such axis into the finite row (0, ..., 0, 1); the pdf's
// support test did the same to +-Inf.  The distance is what is tested, not r: r is also NaN at FINITE distances beyond ~4.3e9
// bins (u4 overflows), where the clamp's 0 is harmless (all three images saturate alike) and stays as it was -- for every
// finite coordinate the bits are unchanged.
__device__ __forceinline__ float quartic_cdf(float v, float n) {
#pragma clang fp contract(off)
  const float u = v * n;
  const float u2 = u * u;
  const float u4 = u2 * u2;
  const float r = (15.0f / 16.0f) * u * (1.0f - (2.0f / 3.0f) * u2 + (1.0f / 5.0f) * u4) + 0.5f;
  if (!(fabsf(v) < INFINITY)) return v - v;               // NaN
  return fminf(fmaxf(r, 0.0f), 1.0f);
}

__device__ __forceinline__ float quartic_pdf(float v, float n) {
#pragma clang fp contract(off)
  const float u = v * n;
  const float u2 = u * u;
  if (!(fabsf(v) < INFINITY)) return v - v;               // NaN (see quartic_cdf)
  if (u2 > 1.0f) return 0.0f;
  const float t = 1.0f - u2;
  return (15.0f / 16.0f) * n * t * t;
}

// G(b) of tcnn's kernel_one_blob at bin edge b (PDF: its derivative with respect to the distance): the kernel centred at x and
// its two periodic images; edge n_bins is edge 0 one period on (+1 for the cdf).  Expression order as in the full loops.
template <bool PDF>
__device__ __forceinline__ float oneblob_edge(uint32_t b, uint32_t n_bins, float n, float xa) {
#pragma clang fp contract(off)
  const uint32_t bb = b < n_bins ? b : 0u;
  const float d = (float)bb / n - xa;
  float g = PDF ? quartic_pdf(d, n) + quartic_pdf(d - 1.0f, n) + quartic_pdf(d + 1.0f, n)
                : quartic_cdf(d, n) + quartic_cdf(d - 1.0f, n) + quartic_cdf(d + 1.0f, n);
  if (!PDF && b >= n_bins) g += 1.0f;
  return g;
}

// The quartic kernel has radius 1/n: away from x (and its images x -+ 1) the cdf terms are EXACTLY 0 or 1 (clamped) and the
// pdf terms exactly 0, so a bin's value G(b+1) - G(b) is exactly zero unless one of its edges lies within one bin of
// c = x n + s n, s in {-1, 0, 1}.  Only the five bins around floor(c) are evaluated (two bins of margin against rounding),
// in ascending order, with the same expressions as the loop over all n + 1 edges: identical results for finite inputs
// from 18 + 6 (the last bin, see below) instead of 51 kernel evaluations per coordinate.  fn(bin, G(bin + 1) - G(bin)) is called for every bin that may be
// non-zero.  (An Inf / NaN in a far bin's upstream gradient no longer turns 0 * Inf into NaN in the backward.)
template <bool PDF, typename F>
__device__ __forceinline__ void oneblob_windows(uint32_t n_bins, float n, float xa, F fn) {
  const float xn = xa * n;
#pragma unroll
  for (int w = -1; w <= 1; ++w) {
    const float c = xn + (float)w * n;
    if (!(c > -3.0f && c < n + 3.0f)) continue;          // also skips NaN
    const int k = (int)floorf(c);
    const int j0 = max(k - 2, 0), j1 = min(k + 2, (int)n_bins - 2);     // the last bin: below
    if (j0 > j1) continue;
    float left = oneblob_edge<PDF>((uint32_t)j0, n_bins, n, xa);
    for (int j = j0; j <= j1; ++j) {
      const float right = oneblob_edge<PDF>((uint32_t)j + 1u, n_bins, n, xa);
      fn((uint32_t)j, right - left);
      left = right;
    }
  }
  // The LAST bin is always evaluated: its right edge is DEFINED as edge 0 (+1 for the cdf) -- the wrap of kernel_one_blob --,
  // so it is non-zero whenever edge 0 lies in ANY image's support (e.g. x = -0.96: edge 0 is inside the image at x + 1 and
  // bin n-1 sees it although no image is near edge n), and for the cdf even with both edges saturated (x = 3: G = 0
  // everywhere, bin n-1 = 1).
  fn(n_bins - 1u, oneblob_edge<PDF>(n_bins, n_bins, n, xa) - oneblob_edge<PDF>(n_bins - 1u, n_bins, n, xa));
}

// OneBlob of one coordinate into out[0 .. n_bins): the windowed form where the windows of different images cannot overlap, the
// loop over all n + 1 edges otherwise
template <typename RowP>
__device__ __forceinline__ void oneblob_axis_fwd(float xa, uint32_t n_bins, RowP out) {
#pragma clang fp contract(off)
  const float n = (float)n_bins;
  if (n_bins >= 8u && fabsf(xa) < 4.0f) {
    for (uint32_t b = 0; b < n_bins; ++b) out[b] = 0.f;
    oneblob_windows<false>(n_bins, n, xa, [&](uint32_t j, float v) { out[j] = v; });
    return;
  }
  float first = 0.f, left = 0.f;
  for (uint32_t b = 0; b <= n_bins; ++b) {
    float g;
    if (b < n_bins) {
      g = oneblob_edge<false>(b, n_bins, n, xa);
      if (b == 0) first = g;
    } else {
      g = first + 1.0f;  // right edge of the last bin wraps (tcnn kernel_one_blob)
    }
    if (b > 0) out[b - 1] = g - left;
    left = g;
  }
}

// d OneBlob / d coordinate contracted with that axis' upstream gradient grad[0 .. n_bins), added to dx: the same two forms.  (The
// sum joins dx in here, uncontracted like the rest: the tracker's units would flag the caller's add for contraction.)
template <typename RowP>
__device__ __forceinline__ void oneblob_axis_bwd(float xa, uint32_t n_bins, RowP grad, float& dx) {
#pragma clang fp contract(off)
  const float n = (float)n_bins;
  float acc = 0.f;
  if (n_bins >= 8u && fabsf(xa) < 4.0f) {
    oneblob_windows<true>(n_bins, n, xa, [&](uint32_t j, float v) { acc -= grad[j] * v; });
    dx += acc;
    return;
  }
  float first = 0.f, left = 0.f;
  for (uint32_t b = 0; b <= n_bins; ++b) {
    float g;
    if (b < n_bins) {
      g = oneblob_edge<true>(b, n_bins, n, xa);
      if (b == 0) first = g;
    } else {
      g = first;
    }
    if (b > 0) acc -= grad[b - 1] * (g - left);  // d out_b / dx = -(g(b+1) - g(b))
    left = g;
  }
  dx += acc;
}

__device__ __forceinline__ void load_point(const float* __restrict__ in, const Bound6& bd, bool normalise,
                                           uint32_t p, float x[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float v = in[(size_t)p * 3 + a];
    if (normalise) v = (float)(((double)v - bd.b0[a]) / (bd.b1[a] - bd.b0[a]));
    x[a] = v;
  }
}

}  // namespace dns
