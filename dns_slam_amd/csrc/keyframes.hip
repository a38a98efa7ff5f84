// Keyframe overlap counts (include/dns_hip.h, "keyframe overlap"): the projection block of keyframe_selection_overlap
// (slams/mapping.py:208-226) for every keyframe of a bank in one launch, no host read.
//
// keyframe_overlap_kernel: blockIdx.y = keyframe, blockIdx.x strides over the points.  Thread 0 of a workgroup inverts the
// keyframe's pose in float64 into LDS (the adjugate from the twelve 2 x 2 minors of rows 0-1 and rows 2-3, every entry divided by
// the determinant; ~150 float64 operations against 256+ points x ~30), then every thread projects its points.  The order of
// operations IS the specification (tests/keyframe_overlap_ref.py restates it in numpy), so the unit is compiled with
// -ffp-contract=off (Makefile) and the two device functions carry the setting themselves: every product, sum and quotient below
// rounds once.  Counting: a wave ballot per pass, the waves' sums through LDS, ONE integer atomic add per workgroup into
// out[keyframe] (zeroed by fill_words ahead of the launch): the counts do not depend on any order.
// Bounds: points are read at i < P only, the pose at keyframe < n (= gridDim.y), out at keyframe.
#include "common.hpp"

namespace dns {
namespace {

constexpr uint32_t KFO_BLOCK = 256;
constexpr uint32_t KFO_WAVES = KFO_BLOCK / WAVE;
constexpr uint32_t KFO_MAX_BLOCKS_X = 64;      // 16384 points per pass of a keyframe's workgroups; more points are strided over

struct KfoArgs {
  const float* pts;      // [P,3]
  const float* c2w;      // [n,4,4]
  int32_t* out;          // [n]
  uint32_t P;
  double fx, fy, cx, cy, eps;
  float lo, u_hi, v_hi;  // edge, W - edge, H - edge
};

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// rows 0-2 of inverse(a) -> w [12]; false (pose counts nothing) for a non-finite entry or a determinant that is 0 or non-finite
__device__ bool invert_pose(const float* __restrict__ m, double* __restrict__ w) {
#pragma clang fp contract(off)
  bool ok = true;
  double a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    a[i] = (double)m[i];
    ok = ok && finite_d(a[i]);
  }
  const double a00 = a[0], a01 = a[1], a02 = a[2], a03 = a[3], a10 = a[4], a11 = a[5], a12 = a[6], a13 = a[7];
  const double a20 = a[8], a21 = a[9], a22 = a[10], a23 = a[11], a30 = a[12], a31 = a[13], a32 = a[14], a33 = a[15];
  const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03;
  const double s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
  const double c0 = a20 * a31 - a30 * a21, c1 = a20 * a32 - a30 * a22, c2 = a20 * a33 - a30 * a23;
  const double c3 = a21 * a32 - a31 * a22, c4 = a21 * a33 - a31 * a23, c5 = a22 * a33 - a32 * a23;
  const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
  ok = ok && finite_d(det) && det != 0.0;
  w[0] = ((a11 * c5 - a12 * c4) + a13 * c3) / det;
  w[1] = ((a02 * c4 - a01 * c5) - a03 * c3) / det;
  w[2] = ((a31 * s5 - a32 * s4) + a33 * s3) / det;
  w[3] = ((a22 * s4 - a21 * s5) - a23 * s3) / det;
  w[4] = ((a12 * c2 - a10 * c5) - a13 * c1) / det;
  w[5] = ((a00 * c5 - a02 * c2) + a03 * c1) / det;
  w[6] = ((a32 * s2 - a30 * s5) - a33 * s1) / det;
  w[7] = ((a20 * s5 - a22 * s2) + a23 * s1) / det;
  w[8] = ((a10 * c4 - a11 * c2) + a13 * c0) / det;
  w[9] = ((a01 * c2 - a00 * c4) - a03 * c0) / det;
  w[10] = ((a30 * s4 - a31 * s2) + a33 * s0) / det;
  w[11] = ((a21 * s2 - a20 * s4) - a23 * s0) / det;
  return ok;
}

// mapping.py:213-224 for one point: camera coordinates, x flipped, K, z = zc + eps, u and v rounded to fp32, five strict comparisons
__device__ __forceinline__ bool point_inside(const KfoArgs& a, const double* __restrict__ w, float px, float py, float pz) {
#pragma clang fp contract(off)
  const double x = (double)px, y = (double)py, z = (double)pz;
  if (!(finite_d(x) && finite_d(y) && finite_d(z))) return false;
  const double xc = -(((w[0] * x + w[1] * y) + w[2] * z) + w[3]);
  const double yc = ((w[4] * x + w[5] * y) + w[6] * z) + w[7];
  const double zc = ((w[8] * x + w[9] * y) + w[10] * z) + w[11];
  const double ze = zc + a.eps;
  const float u = (float)((a.fx * xc + a.cx * zc) / ze);
  const float v = (float)((a.fy * yc + a.cy * zc) / ze);
  return (u < a.u_hi) && (u > a.lo) && (v < a.v_hi) && (v > a.lo) && (ze < 0.0);
}

__global__ __launch_bounds__(KFO_BLOCK) void keyframe_overlap_kernel(const KfoArgs a) {
  __shared__ double w[12];
  __shared__ int pose_ok;
  __shared__ uint32_t wave_count[KFO_WAVES];
  const uint32_t k = blockIdx.y, t = threadIdx.x;
  if (t == 0) pose_ok = invert_pose(a.c2w + (size_t)k * 16u, w) ? 1 : 0;
  __syncthreads();
  if (!pose_ok) return;                                   // workgroup-uniform: out[k] stays 0
  uint32_t count = 0;                                     // wave-uniform
  const uint32_t stride = gridDim.x * KFO_BLOCK;
  for (uint32_t base = blockIdx.x * KFO_BLOCK; base < a.P; base += stride) {   // workgroup-uniform trip count
    const uint32_t i = base + t;
    bool in = false;
    if (i < a.P) {
      const float* p = a.pts + (size_t)i * 3u;
      in = point_inside(a, w, p[0], p[1], p[2]);
    }
    count += (uint32_t)__popcll(__ballot(in));
  }
  if ((t & (WAVE - 1)) == 0) wave_count[t / WAVE] = count;
  __syncthreads();
  if (t == 0) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t v = 0; v < KFO_WAVES; ++v) total += wave_count[v];
    if (total) atomicAdd(a.out + k, (int32_t)total);
  }
}

}  // namespace
}  // namespace dns

using namespace dns;

extern "C" int dns_keyframe_overlap(const float* pts, uint32_t P, const float* c2w, uint32_t n, int H, int W, double fx, double fy,
                                    double cx, double cy, int edge, double eps, int32_t* out, void* stream) {
  DNS_REQUIRE(n <= 65535u, "dns_keyframe_overlap: %u keyframes (must be <= 65535)", n);
  DNS_REQUIRE(P < (1u << 31), "dns_keyframe_overlap: %u points (must be < 2^31)", P);
  DNS_REQUIRE(H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24) && edge >= 0 && edge <= (1 << 24),
              "dns_keyframe_overlap: H %d, W %d, edge %d (sides 1..2^24, edge 0..2^24: exact in fp32)", H, W, edge);
  if (n == 0) return DNS_OK;
  DNS_REQUIRE(out, "dns_keyframe_overlap: NULL out");
  hipStream_t st = (hipStream_t)stream;
  const int rc = fill_words(out, 0u, n, st, "dns_keyframe_overlap");
  if (rc != DNS_OK || P == 0) return rc;
  DNS_REQUIRE(pts && c2w, "dns_keyframe_overlap: NULL argument");
  KfoArgs a;
  a.pts = pts, a.c2w = c2w, a.out = out, a.P = P;
  a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.eps = eps;
  a.lo = (float)edge, a.u_hi = (float)(W - edge), a.v_hi = (float)(H - edge);
  const uint32_t bx = (P + KFO_BLOCK - 1) / KFO_BLOCK;
  DNS_LAUNCH(keyframe_overlap_kernel, dim3(bx < KFO_MAX_BLOCKS_X ? bx : KFO_MAX_BLOCKS_X, n), dim3(KFO_BLOCK), 0, st, a);
  return check_launch("dns_keyframe_overlap");
}
