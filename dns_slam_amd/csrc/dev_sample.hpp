// Device helpers of the ray generation / depth-guided sampling kernels (sample.hip) -- shared with the fused tracker iteration
// (track_fused.inc).  Every product or sum that decides a value bit for bit is spelled __fmul_rn / __fadd_rn / __dmul_rn, so
// the result does not depend on the translation unit's -ffp-contract setting -- through dev_rn.hpp's spellings DNS_FMUL ..., which
// says why the intrinsics alone do not achieve that.
#pragma once
#include "common.hpp"
#include "dev_rn.hpp"

namespace dns {

struct Cam {
  float fx, fy, cx, cy;
};
struct BoundD {
  double b[6];  // b0x,b1x,b0y,b1y,b0z,b1z
};

__device__ __forceinline__ uint32_t f2key(float f) {
  if (f != f) return 0xFFC00000u;  // every NaN sorts after +inf (torch.sort puts NaN last), below the pad key
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __uint_as_float(b);
}

__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }
__device__ __forceinline__ double min_nan(double a, double b) { return (a != a || b != b) ? (a + b) : (a < b ? a : b); }

__device__ __forceinline__ void quat_to_R(const float* __restrict__ q, float R[9]) {
  const float qr = q[0], qi = q[1], qj = q[2], qk = q[3];
  const float nrm = DNS_FADD(DNS_FADD(DNS_FADD(DNS_FMUL(qr, qr), DNS_FMUL(qi, qi)), DNS_FMUL(qj, qj)), DNS_FMUL(qk, qk));
  const float two_s = 2.0f / nrm;
  const float jj = DNS_FMUL(qj, qj), kk = DNS_FMUL(qk, qk), ii = DNS_FMUL(qi, qi);
  const float ij = DNS_FMUL(qi, qj), kr = DNS_FMUL(qk, qr), ik = DNS_FMUL(qi, qk), jr = DNS_FMUL(qj, qr);
  const float jk = DNS_FMUL(qj, qk), ir = DNS_FMUL(qi, qr);
  R[0] = DNS_FSUB(1.0f, DNS_FMUL(two_s, DNS_FADD(jj, kk)));
  R[1] = DNS_FMUL(two_s, DNS_FSUB(ij, kr));
  R[2] = DNS_FMUL(two_s, DNS_FADD(ik, jr));
  R[3] = DNS_FMUL(two_s, DNS_FADD(ij, kr));
  R[4] = DNS_FSUB(1.0f, DNS_FMUL(two_s, DNS_FADD(ii, kk)));
  R[5] = DNS_FMUL(two_s, DNS_FSUB(jk, ir));
  R[6] = DNS_FMUL(two_s, DNS_FSUB(ik, jr));
  R[7] = DNS_FMUL(two_s, DNS_FADD(jk, ir));
  R[8] = DNS_FSUB(1.0f, DNS_FMUL(two_s, DNS_FADD(ii, jj)));
}

__device__ __forceinline__ void pixel_dir(int64_t q, int H0, int W0, int wwin, Cam cam, int& row, int& col, float dir[3]) {
  row = H0 + (int)(q / wwin);
  col = W0 + (int)(q % wwin);
  dir[0] = DNS_FDIV(DNS_FSUB((float)col, cam.cx), cam.fx);
  dir[1] = -DNS_FDIV(DNS_FSUB((float)row, cam.cy), cam.fy);
  dir[2] = -1.0f;
}

// z values of one ray (utils/common.py:561-599) as sorted order-preserving keys; lane owns elements e*64+lane.
// `far` is far_bb AFTER the +0.01 (fp64).  Surface part fp32, uniform part fp64 then rounded, as the reference.
template <int E>
__device__ __forceinline__ void sample_and_sort(float gd, double far, float dmax, const float* __restrict__ t_uniform,
                                                const float* __restrict__ t_surf, const float* __restrict__ t_zero,
                                                int nu, int ns, uint32_t lane, uint32_t (&key)[E]) {
  const int S = nu + ns;
  const double hi = (double)DNS_FMUL(dmax, 1.2f);
  double farc = far;                      // torch.clamp(far, 0, hi): NaN propagates
  if (farc == farc) {
    farc = farc < 0.0 ? 0.0 : farc;
    farc = farc > hi ? hi : farc;
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int s = e * 64 + (int)lane;
    float zv;
    if (s < nu) {
      const float tv = t_uniform[s];
      const float near = DNS_FMUL(gd, 0.001f);
      const float a = DNS_FMUL(near, DNS_FSUB(1.0f, tv));
      zv = (float)DNS_DADD((double)a, DNS_DMUL(farc, (double)tv));
    } else if (s < S) {
      const int k = s - nu;
      if (gd > 0.f) {
        const float t = t_surf[k];
        zv = DNS_FADD(DNS_FMUL(DNS_FMUL(0.95f, gd), DNS_FSUB(1.0f, t)), DNS_FMUL(DNS_FMUL(1.05f, gd), t));
      } else {
        const float t = t_zero[k];
        zv = DNS_FADD(DNS_FMUL(0.001f, DNS_FSUB(1.0f, t)), DNS_FMUL(dmax, t));
      }
    } else {
      zv = 0.f;
    }
    key[e] = (s < S) ? f2key(zv) : 0xFFFFFFFFu;
  }
  // bitonic sort of 64*E keys; element id g = e*64 + lane
  constexpr int NTOT = 64 * E;
#pragma unroll
  for (int k = 2; k <= NTOT; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      if (j >= 64) {
        const int je = j >> 6;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int pe = e ^ je;
          if (pe > e) {
            const int g = e * 64 + (int)lane;
            const bool up = (g & k) == 0;
            const uint32_t lo = min(key[e], key[pe]), hi2 = max(key[e], key[pe]);
            key[e] = up ? lo : hi2;
            key[pe] = up ? hi2 : lo;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int g = e * 64 + (int)lane;
          const uint32_t other = (uint32_t)__shfl_xor((int)key[e], j);
          const bool up = (g & k) == 0;
          const bool lower = (g & j) == 0;
          key[e] = (lower == up) ? min(key[e], other) : max(key[e], other);
        }
      }
    }
  }
}

}  // namespace dns
