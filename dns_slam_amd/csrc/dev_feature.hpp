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

// ---- a (point, view) pair of the in-kernel 2-D branch: frame_codes.hip (phase A) and track_fused.inc (phase 3a) -----------------
// The pair's code -> dst[0 .. C) (16-byte aligned, C % 4 == 0), lane `sub` of the pair's 16: what feature_gather4_kernel does.
// m: the view's w2c (its first 12 floats are read), f: the view's map [h, w, C].  Not valid, or not kept: zeros, and no tap is read.
__device__ __forceinline__ void pair_code(const float* m, const Mat3& K, const float* __restrict__ f, uint32_t C, int h, int w, int H,
                                          int W, float x, float y, float z, bool kept, uint32_t sub, float* __restrict__ dst) {
  const FeaturePixel q = feature_project(m, K, x, y, z, H, W, kept);
  const uint32_t C4 = C / 4u;
  float4* out = reinterpret_cast<float4*>(dst);
  if (!q.ok) {
    for (uint32_t c = sub; c < C4; c += 16) out[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const FeatureTaps t = feature_taps(q.u, q.v, h, w, H, W);
  const float4* f00 = reinterpret_cast<const float4*>(f + ((size_t)t.y0 * w + t.x0) * C);
  const float4* f01 = reinterpret_cast<const float4*>(f + ((size_t)t.y0 * w + t.x1) * C);
  const float4* f10 = reinterpret_cast<const float4*>(f + ((size_t)t.y1 * w + t.x0) * C);
  const float4* f11 = reinterpret_cast<const float4*>(f + ((size_t)t.y1 * w + t.x1) * C);
  feature_row<16>(f00, f01, f10, f11, t.lx, t.ly, C4, sub, out);
}
// rel = p - o_r (fp32, utils/common.py:675), normalised with Merge's bound in fp64 (dev_encode.hpp load_point's expression)
__device__ __forceinline__ void pair_rel(const float (&p)[3], const float (&o)[3], const double (&b0)[3], const double (&b1)[3],
                                         float (&x)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float rel = p[k] - o[k];
    x[k] = (float)(((double)rel - b0[k]) / (b1[k] - b0[k]));
  }
}

// ---- a reference view's pose -> w2c and origin: refer_poses_kernel (feature.hip) and the fused tracker's following views --------
// Rotation of the quaternion AS IT STANDS IN THE OPTIMISER (get_rotation_from_quad, utils/common.py:406-429: two_s = 2 / |q|^2, no
// normalisation) and the translation, as float64 A [3 x 3], t [3]
__device__ __forceinline__ void pose_from_quat(const float* q, const float* trans, double (&A)[9], double (&t)[3]) {
#pragma clang fp contract(off)
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float two_s = 2.0f / (qw * qw + qx * qx + qy * qy + qz * qz);
  const float Rm[9] = {1.0f - two_s * (qy * qy + qz * qz), two_s * (qx * qy - qz * qw), two_s * (qx * qz + qy * qw),
                       two_s * (qx * qy + qz * qw), 1.0f - two_s * (qx * qx + qz * qz), two_s * (qy * qz - qx * qw),
                       two_s * (qx * qz - qy * qw), two_s * (qy * qz + qx * qw), 1.0f - two_s * (qx * qx + qy * qy)};
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = (double)Rm[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = (double)trans[i];
}
// w2c = the affine inverse of [A | t] (the 3 x 3 block inverted by cofactors in float64; torch.inverse in the reference), rows
// 0..2 -> o[0 .. 12), the last row -> o[12 .. 16) unless ROWS3; origin = t (refer_o, utils/common.py:674)
template <bool ROWS3 = false, typename OutP>
__device__ __forceinline__ void pose_inverse(const double (&A)[9], const double (&t)[3], OutP o, OutP origin) {
#pragma clang fp contract(off)
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  const double id = 1.0 / det;
  const double I[9] = {c00 * id, (A[2] * A[7] - A[1] * A[8]) * id, (A[1] * A[5] - A[2] * A[4]) * id,
                       c01 * id, (A[0] * A[8] - A[2] * A[6]) * id, (A[2] * A[3] - A[0] * A[5]) * id,
                       c02 * id, (A[1] * A[6] - A[0] * A[7]) * id, (A[0] * A[4] - A[1] * A[3]) * id};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)I[3 * i + j];
    o[4 * i + 3] = (float)(-(I[3 * i] * t[0] + I[3 * i + 1] * t[1] + I[3 * i + 2] * t[2]));
  }
  if (!ROWS3) { o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f; }
#pragma unroll
  for (int i = 0; i < 3; ++i) origin[i] = (float)t[i];
}
}  // namespace dns
