// The feature branch's lookup of a point in a reference view: the projection to a rounded pixel and the bilinear value of the
// half-resolution channels-last stem map [views, h, w, C] at that integer full-resolution pixel -- F.interpolate(bilinear,
// align_corners=True) of the map, read at (u, v), without the up-sampled map.  Callers: feature_gather_kernel and
// feature_gather4_kernel (feature.hip), pair_code (frame_codes.hip) and kf_pair_rows_kernel (mesh_feature.hip, which takes the pixel
// from its record and has no projection).  The fused paths are held to the launch paths bit for bit, so the expressions exist
// here and nowhere else.  This is the FEATURE convention (reference utils/common.py:645-673): the meshing and evaluation
// projections are dev_project.hpp's.
// Every function with floating-point arithmetic carries the contraction setting itself: sx = scale * u must be ROUNDED before lx = sx - floor(sx) (a fused
// multiply-subtract shifts the weight by up to half an ulp of sx ~ 1e-5 at 300 px, visible against F.interpolate), and a unit
// compiled with contraction (frame_codes.hip) must give the bits of the units compiled without.
#pragma once
#include "common.hpp"
namespace dns {
struct Mat3 {
  float k[9];
};
struct FeaturePixel { float u, v; bool ok; };                      // the rounded pixel, as floats; ok: inside the view
// m: one pose of w2c (16 floats).  The camera-frame point with y and z flipped (utils/common.py:650-652), K @ cam, the pixel
// rounded; inside iff 0 < u < W - 1, 0 < v < H - 1 and the point is in front of the camera.  live: a caller's own condition on the
// pair (frame_codes.hip's keep mask), the first term of ok.
__device__ __forceinline__ FeaturePixel feature_project(const float* m, const Mat3& K, float x, float y, float z, int H,
                                                        int W, bool live = true) {
#pragma clang fp contract(off)
  const float cx_ = fmaf(m[3], 1.0f, fmaf(m[2], z, fmaf(m[1], y, m[0] * x)));
  const float cy_ = -fmaf(m[7], 1.0f, fmaf(m[6], z, fmaf(m[5], y, m[4] * x)));
  const float cz_ = -fmaf(m[11], 1.0f, fmaf(m[10], z, fmaf(m[9], y, m[8] * x)));
  const float q0 = fmaf(K.k[2], cz_, fmaf(K.k[1], cy_, K.k[0] * cx_));
  const float q1 = fmaf(K.k[5], cz_, fmaf(K.k[4], cy_, K.k[3] * cx_));
  const float q2 = fmaf(K.k[8], cz_, fmaf(K.k[7], cy_, K.k[6] * cx_));
  const float u = rintf(q0 / (q2 + 1e-5f));            // torch.round: half to even
  const float v = rintf(q1 / (q2 + 1e-5f));
  const bool ok = live && (u > 0.f) && (u < (float)(W - 1)) && (v > 0.f) && (v < (float)(H - 1)) && (cz_ > 0.f);
  return {u, v, ok};
}
// The four taps of the [h, w] map under the pixel (u, v) of the [H, W] frame and their weights.  CLAMP: x0 / y0 held to the map,
// a bound on the tap addresses for a caller that does not know its pixel to be inside the view (sx <= w - 1 for every pixel of
// the frame, so no value changes).
struct FeatureTaps { int x0, y0, x1, y1; float lx, ly; };
template <bool CLAMP = false>
__device__ __forceinline__ FeatureTaps feature_taps(float u, float v, int h, int w, int H, int W) {
#pragma clang fp contract(off)
  const float sx_scale = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  const float sy_scale = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
  const float sx = __fmul_rn(sx_scale, u), sy = __fmul_rn(sy_scale, v);
  FeatureTaps t;
  t.x0 = CLAMP ? min((int)sx, w - 1) : (int)sx, t.y0 = CLAMP ? min((int)sy, h - 1) : (int)sy;
  t.lx = sx - (float)t.x0, t.ly = sy - (float)t.y0;
  t.x1 = t.x0 + (t.x0 < w - 1 ? 1 : 0), t.y1 = t.y0 + (t.y0 < h - 1 ? 1 : 0);
  return t;
}
// one channel: a, b the taps of row y0 at x0, x1; d, e those of row y1
__device__ __forceinline__ float feature_blend(float lx, float ly, float a, float b, float d, float e) {
#pragma clang fp contract(off)
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * d + lx * e);
}
__device__ __forceinline__ float4 feature_blend(float lx, float ly, const float4& a, const float4& b, const float4& d, const float4& e) {
  return make_float4(feature_blend(lx, ly, a.x, b.x, d.x, e.x), feature_blend(lx, ly, a.y, b.y, d.y, e.y),
                     feature_blend(lx, ly, a.z, b.z, d.z, e.z), feature_blend(lx, ly, a.w, b.w, d.w, e.w));
}
// A pair's channels -> out, by LANES lanes of which this is lane `sub`, one V (float, or float4 where C % 4 == 0 and the rows are
// 16-byte aligned) per lane and step; n = C in units of V.  f00 .. f11: the four tap rows, f + ((size_t)y * w + x) * C with f the
// map of the pair's view, formed by the caller.
template <uint32_t LANES, typename V>
__device__ __forceinline__ void feature_row(const V* f00, const V* f01, const V* f10, const V* f11, float lx, float ly, uint32_t n,
                                            uint32_t sub, V* out) {
  for (uint32_t c = sub; c < n; c += LANES) {
    const V a = f00[c], b = f01[c], d = f10[c], e = f11[c];
    out[c] = feature_blend(lx, ly, a, b, d, e);
  }
}
}  // namespace dns
