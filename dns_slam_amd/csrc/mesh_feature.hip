// Keyframe codes of the mesh vertex query: get_2d_feature (reference slams/meshing.py:311-377) as a pair list.
//
// The reference loops over the keyframes and, for every point a keyframe sees, runs the stem map through Merge, masks the
// latent with the truncation test against the keyframe's depth image, and adds it to the point's code; the sum is divided
// by the number of unmasked views.  A masked view adds zeros, so only the (point, keyframe) pairs that are seen AND pass
// the truncation test matter.  Here those pairs are listed first (a counting pass, an exclusive prefix made by the caller,
// an emitting pass: point-major, keyframes ascending within a point), then three passes run over the list: the Merge
// network's input rows (relative point + bilinear stem value), the network itself (dns_encode_fwd + dns_mlp_fwd, driven by
// the caller), and the per-point mean.  No atomics anywhere: a point's latents are added in list order, which is the
// reference's keyframe order, so every result is the same bits from call to call and for every chunking by points.
#include "common.hpp"
#include "dev_feature.hpp"
#include "dev_project.hpp"

namespace dns {

namespace {

constexpr int KFP_BLOCK = 256;
constexpr int KFP_TILE = 256;   // keyframes staged in LDS at a time (12 KB), as kf_project_kernel (mesh.hip) does

// One thread per point, keyframes in ASCENDING order.  The meshing convention of dev_project.hpp, as kf_project_kernel (mesh.hip)
// without its maximum-depth test: labels and codes agree on which keyframes see a point.  EMIT = false: count[p] = number of contributing keyframes.  EMIT = true:
// record i of point p goes to rec[offset[p] + i] = {p, keyframe, iu, iv}; nothing is stored at or beyond cap.
template <bool EMIT>
__global__ __launch_bounds__(KFP_BLOCK) void kf_pair_kernel(const float* __restrict__ pts, uint32_t P, const float* __restrict__ w2c,
                                                            uint32_t K, const float* __restrict__ depth, int H, int W, float fx,
                                                            float fy, float cx, float cy, int32_t* __restrict__ count,
                                                            const int64_t* __restrict__ offset, int4* __restrict__ rec,
                                                            uint64_t cap) {
  __shared__ float s_w[KFP_TILE * 12];
  const uint32_t p = blockIdx.x * KFP_BLOCK + threadIdx.x;
  const bool live = p < P;
  const float3 pt = load_point3(pts, p, live);
  const float fW = (float)W, fH = (float)H;
  uint32_t n_pairs = 0;
  uint64_t base = 0;
  if (EMIT && live) base = (uint64_t)offset[p];
  for (uint32_t lo = 0; lo < K; lo += KFP_TILE) {
    const int n = (int)min((uint32_t)KFP_TILE, K - lo);
    __syncthreads();
    stage_poses<KFP_BLOCK>(s_w, w2c, lo, n);
    __syncthreads();
    if (!live) continue;
    for (int kk = 0; kk < n; ++kk) {
      const Projected q = project(s_w + kk * 12, pt, fx, fy, cx, cy, PROJ_EPS_MESHING);
      if (!inside_meshing(q, fW, fH)) continue;
      const int iu = round_pixel(q.u, W), iv = round_pixel(q.v, H);
      const float d = depth[((size_t)(lo + kk) * H + iv) * W + iu];
      const float dp = -q.z;
      // trunc = (1 - front) (1 - back), meshing.py:352-356; a depth hole (d = 0) is behind the surface: dp > 0
      if (dp < d * 0.95f || dp > d * 1.05f) continue;
      if (EMIT) {
        const uint64_t at = base + n_pairs;
        if (at < cap) rec[at] = make_int4((int)p, (int)(lo + kk), iu, iv);
      }
      ++n_pairs;
    }
  }
  if (!EMIT && live) count[p] = (int32_t)n_pairs;
}

// 16 lanes per pair, one float4 of channels per lane (feature_gather4_kernel's layout, feature.hip): rel[pair] = p - o_k and
// the bilinear value of the half-resolution channels-last stem map [K, h, w, C] at the integer full-resolution pixel (iu, iv)
// -- F.interpolate(align_corners=True) read at that pixel: feature_taps and feature_row of dev_feature.hpp -- written at a row
// stride.  The pixel comes from a record, not from feature_project's inside test, so the taps are taken with CLAMP: x0 / y0 held
// to the map (a bound on the tap addresses; sx <= w - 1 for every pixel inside the image, so no value changes).
__global__ __launch_bounds__(256) void kf_pair_rows_kernel(const int4* __restrict__ rec, uint64_t n, const float* __restrict__ pts,
                                                           uint32_t P, const float* __restrict__ origin, uint32_t K,
                                                           const float* __restrict__ feat, uint32_t C, int h, int w, int H, int W,
                                                           float* __restrict__ rel_out, float* __restrict__ code, uint32_t ld_code) {
  const uint32_t sub = threadIdx.x & 15u;
  const uint64_t pair = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (pair >= n) return;
  const int4 r = rec[pair];
  if ((uint32_t)r.x >= P || (uint32_t)r.y >= K || (uint32_t)r.z >= (uint32_t)W || (uint32_t)r.w >= (uint32_t)H) return;
  if (sub < 3u) rel_out[pair * 3 + sub] = pts[(size_t)r.x * 3 + sub] - origin[(size_t)r.y * 3 + sub];
  const FeatureTaps t = feature_taps<true>((float)r.z, (float)r.w, h, w, H, W);
  const float* f = feat + (size_t)r.y * h * w * C;
  const float4* f00 = reinterpret_cast<const float4*>(f + ((size_t)t.y0 * w + t.x0) * C);
  const float4* f01 = reinterpret_cast<const float4*>(f + ((size_t)t.y0 * w + t.x1) * C);
  const float4* f10 = reinterpret_cast<const float4*>(f + ((size_t)t.y1 * w + t.x0) * C);
  const float4* f11 = reinterpret_cast<const float4*>(f + ((size_t)t.y1 * w + t.x1) * C);
  feature_row<16>(f00, f01, f10, f11, t.lx, t.ly, C / 4u, sub, reinterpret_cast<float4*>(code + pair * ld_code));
}

// 8 lanes per point, one float4 of channels per lane and step: the point's segment of latents added in list order (the order
// of the reference's `+=` over the keyframes, meshing.py:372), divided by (float)count (:375); zeros where count == 0.
__global__ __launch_bounds__(256) void kf_code_mean_kernel(const float* __restrict__ lat, uint32_t ld_lat, uint64_t n,
                                                           const int64_t* __restrict__ offset, const int32_t* __restrict__ count,
                                                           uint32_t P, uint32_t D, float* __restrict__ code) {
  const uint32_t sub = threadIdx.x & 7u;
  const uint64_t p = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (p >= P) return;
  const int32_t cnt = count[p];
  const uint64_t s0 = (uint64_t)offset[p];
  const bool ok = cnt > 0 && s0 <= n && (uint64_t)cnt <= n - s0;          // a segment inside the list (always, from the pair kernels)
  const float fc = (float)cnt;
  for (uint32_t c = sub; c < D / 4u; c += 8) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      for (int32_t i = 0; i < cnt; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(lat + (s0 + i) * ld_lat + 4u * c);
        s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
      }
      s.x /= fc, s.y /= fc, s.z /= fc, s.w /= fc;
    }
    *reinterpret_cast<float4*>(code + p * D + 4u * c) = s;
  }
}

int pair_args(const char* who, const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* depth, int H, int W,
              const float* intr) {
  DNS_REQUIRE(pts && intr, "%s: NULL argument", who);
  DNS_REQUIRE(K == 0 || (w2c && depth), "%s: K > 0 needs w2c and depth", who);
  DNS_REQUIRE(H > 0 && W > 0, "%s: image %d x %d", who, H, W);
  DNS_REQUIRE((uint64_t)P * (K ? K : 1) < (1ull << 31), "%s: %u points x %u keyframes (must be < 2^31 pairs)", who, P, K);
  return DNS_OK;
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" int dns_kf_pair_count(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* depth, int H, int W,
                                 const float* intr, int32_t* count, void* stream) {
  if (P == 0) return DNS_OK;
  if (int rc = pair_args("dns_kf_pair_count", pts, P, w2c, K, depth, H, W, intr)) return rc;
  DNS_REQUIRE(count, "dns_kf_pair_count: NULL count");
  DNS_LAUNCH(kf_pair_kernel<false>, dim3((P + KFP_BLOCK - 1) / KFP_BLOCK), dim3(KFP_BLOCK), 0, (hipStream_t)stream, pts, P, w2c, K,
             depth, H, W, intr[0], intr[1], intr[2], intr[3], count, (const int64_t*)nullptr, (int4*)nullptr, (uint64_t)0);
  return check_launch("dns_kf_pair_count");
}

extern "C" int dns_kf_pair_emit(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* depth, int H, int W,
                                const float* intr, const int64_t* offset, int32_t* records, uint64_t capacity, void* stream) {
  if (P == 0 || K == 0 || capacity == 0) return DNS_OK;
  if (int rc = pair_args("dns_kf_pair_emit", pts, P, w2c, K, depth, H, W, intr)) return rc;
  DNS_REQUIRE(offset && records, "dns_kf_pair_emit: NULL offset / records");
  DNS_REQUIRE(((uintptr_t)records & 15) == 0, "dns_kf_pair_emit: records must be 16-byte aligned");
  DNS_LAUNCH(kf_pair_kernel<true>, dim3((P + KFP_BLOCK - 1) / KFP_BLOCK), dim3(KFP_BLOCK), 0, (hipStream_t)stream, pts, P, w2c, K,
             depth, H, W, intr[0], intr[1], intr[2], intr[3], (int32_t*)nullptr, offset, reinterpret_cast<int4*>(records), capacity);
  return check_launch("dns_kf_pair_emit");
}

extern "C" int dns_kf_pair_rows(const int32_t* records, uint64_t n, const float* pts, uint32_t P, const float* origin, uint32_t K,
                                const float* feat, uint32_t C, int h, int w, int H, int W, float* rel, float* code, uint32_t ld_code,
                                void* stream) {
  if (n == 0) return DNS_OK;
  DNS_REQUIRE(records && pts && origin && feat && rel && code, "dns_kf_pair_rows: NULL argument");
  DNS_REQUIRE(P >= 1 && K >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "dns_kf_pair_rows: bad dimensions");
  DNS_REQUIRE(C >= 4 && C % 4 == 0 && ld_code >= C && ld_code % 4 == 0, "dns_kf_pair_rows: C %u / ld %u (C %% 4 == 0, ld %% 4 == 0)", C,
              ld_code);
  DNS_REQUIRE((((uintptr_t)records | (uintptr_t)feat | (uintptr_t)code) & 15) == 0, "dns_kf_pair_rows: 16-byte alignment");
  DNS_REQUIRE(n < (1ull << 31), "dns_kf_pair_rows: too many pairs");
  DNS_LAUNCH(kf_pair_rows_kernel, dim3((uint32_t)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream,
             reinterpret_cast<const int4*>(records), n, pts, P, origin, K, feat, C, h, w, H, W, rel, code, ld_code);
  return check_launch("dns_kf_pair_rows");
}

extern "C" int dns_kf_code_mean(const float* latents, uint32_t ld_lat, uint64_t n, const int64_t* offset, const int32_t* count,
                                uint32_t P, uint32_t D, float* code, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(offset && count && code, "dns_kf_code_mean: NULL argument");
  DNS_REQUIRE(n == 0 || latents, "dns_kf_code_mean: NULL latents with n > 0");
  DNS_REQUIRE(D >= 4 && D % 4 == 0 && ld_lat >= D && ld_lat % 4 == 0, "dns_kf_code_mean: D %u / ld %u (D %% 4 == 0, ld %% 4 == 0)", D,
              ld_lat);
  DNS_REQUIRE((((uintptr_t)latents | (uintptr_t)code) & 15) == 0, "dns_kf_code_mean: 16-byte alignment");
  DNS_LAUNCH(kf_code_mean_kernel, dim3((P + 31) / 32), dim3(256), 0, (hipStream_t)stream, latents, ld_lat, n, offset, count, P, D, code);
  return check_launch("dns_kf_code_mean");
}
