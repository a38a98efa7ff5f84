// TSDF fusion of posed depth images into 16^3-voxel units and the vertices of its zero crossing: the volume behind
// Mesher.get_bound_from_frames (slams/meshing.py:380-445: Open3D's ScalableTSDFVolume with integrate() per keyframe and the
// vertices of extract_triangle_mesh()).  tests/tsdf_ref.py is the definition; every expression here is that file's, in its order,
// and the unit is compiled with -ffp-contract=off (Makefile), so units, weights, tsdf values and vertices agree bit for bit.
//
//   tsdf_touch:     thread = one sampled (frame, pixel), pixels (i, j) with i % stride == 0 and j % stride == 0 and
//                   0 < depth < 1000.  The float64 back-projection p = pose (x, y, z, 1) touches the units floor((p - trunc) / L)
//                   .. floor((p + trunc) / L) per axis (L = 16 voxel_length; 2 trunc < L is required, so at most 2 x 2 x 2).  Each
//                   (unit, frame) is a 64-bit key claimed in an open-addressing set by compare-and-swap against the all-ones
//                   word (dev_keytable.hpp's key_claim); a probe sequence that runs out sets status[0] and the caller retries
//                   with a larger table -- nothing is dropped silently.  The caller compacts and sorts the keys: that is the
//                   sorted unit list and, per unit, its frames in ascending order.
//   tsdf_integrate: workgroup = unit, thread = one (x, y) column of 16 voxels kept in registers, looping over the unit's frames in
//                   ascending order; every (tsdf, weight) is stored once.  No atomics.
//   tsdf_vertices:  workgroup = unit.  An 18^3 tile in LDS (23 KB) holds the unit and one voxel on every side, unobserved
//                   (weight 0) or missing voxels as NaN; neighbouring units are found by binary search in the sorted unit keys.
//                   Voxel a, axis e emits a vertex when a and a + e are observed with different (tsdf < 0) and one of the four
//                   cubes around that edge has eight observed corners.  Count -> caller's exclusive prefix over units -> emit; a
//                   workgroup scan orders the vertices by voxel ((x 16 + y) 16 + z), then axis.
#include "common.hpp"
#include "dev_keytable.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

constexpr int TS_BLOCK = 256;
constexpr int TS_UNIT = 16;
constexpr int TS_TILE = TS_UNIT + 2;
constexpr int TS_MAX_PROBE = 4096;

// Signed 64-bit order of the keys = lexicographic order of (ux, uy, uz, frame): ux in two's complement on top, the rest biased.
__device__ __forceinline__ uint64_t ts_key(int ux, int uy, int uz, uint32_t k) {
  return ((uint64_t)(uint16_t)(int16_t)ux << 48) | ((uint64_t)(uint32_t)(uy + 32768) << 32) | ((uint64_t)(uint32_t)(uz + 32768) << 16) |
         (uint64_t)k;
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_touch_kernel(const float* __restrict__ depth, const double* __restrict__ pose,
                                                              uint32_t K, int H, int W, int stride, int Hs, int Ws, double fx,
                                                              double fy, double cx, double cy, double L, double trunc,
                                                              uint64_t* __restrict__ table, uint32_t cap,
                                                              uint32_t* __restrict__ status) {
  const uint64_t t = (uint64_t)blockIdx.x * TS_BLOCK + threadIdx.x;
  const uint64_t per = (uint64_t)Hs * Ws;
  if (t >= per * K) return;
  const uint32_t k = (uint32_t)(t / per);
  const uint32_t r = (uint32_t)(t - (uint64_t)k * per);
  const int i = (int)(r / (uint32_t)Ws) * stride, j = (int)(r % (uint32_t)Ws) * stride;
  const float d = depth[((size_t)k * H + i) * W + j];
  if (!(d > 0.0f && d < 1000.0f)) return;
  const double z = (double)d;
  const double x = (((double)j - cx) * z) / fx, y = (((double)i - cy) * z) / fy;
  const double* P = pose + 16 * (size_t)k;
  int lo[3], hi[3];
  bool bad = false;
  for (int a = 0; a < 3; ++a) {
    const double p = ((P[4 * a] * x + P[4 * a + 1] * y) + P[4 * a + 2] * z) + P[4 * a + 3];
    const double l = floor((p - trunc) / L), h = floor((p + trunc) / L);
    if (!(l >= -32768.0 && h <= 32767.0)) bad = true;            // also catches NaN
    lo[a] = (int)l, hi[a] = (int)h;
  }
  if (bad) {
    atomicOr(&status[0], 2u);
    return;
  }
  const uint32_t limit = cap < (uint32_t)TS_MAX_PROBE ? cap : (uint32_t)TS_MAX_PROBE;
  for (int c = 0; c < 8; ++c) {
    if (((c & 1) && hi[0] == lo[0]) || ((c & 2) && hi[1] == lo[1]) || ((c & 4) && hi[2] == lo[2])) continue;
    const uint64_t key = ts_key((c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2], k);
    if (key_claim(table, cap, key, limit) == KEY_NONE) {
      atomicOr(&status[0], 1u);
      return;
    }
  }
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_integrate_kernel(const int32_t* __restrict__ units, const int64_t* __restrict__ offset,
                                                                  const int32_t* __restrict__ frames, const float* __restrict__ depth,
                                                                  const double* __restrict__ extr, const float* __restrict__ mult,
                                                                  uint32_t K, int H, int W, float fx, float fy, float cx, float cy,
                                                                  double vl, double L, float trunc, float* __restrict__ tsdf,
                                                                  float* __restrict__ weight) {
  const uint32_t b = blockIdx.x;
  const int x = threadIdx.x / TS_UNIT, y = threadIdx.x % TS_UNIT;
  const double ox = (double)units[3 * (size_t)b] * L, oy = (double)units[3 * (size_t)b + 1] * L, oz = (double)units[3 * (size_t)b + 2] * L;
  const float px = (float)(((double)x + 0.5) * vl + ox), py = (float)(((double)y + 0.5) * vl + oy);
  float pz[TS_UNIT], tv[TS_UNIT], wv[TS_UNIT];
#pragma unroll
  for (int z = 0; z < TS_UNIT; ++z) {
    pz[z] = (float)(((double)z + 0.5) * vl + oz);
    tv[z] = 0.0f, wv[z] = 0.0f;
  }
  const float u_hi = (float)W - 1e-4f, v_hi = (float)H - 1e-4f;
  for (int64_t q = offset[b]; q < offset[b + 1]; ++q) {
    const uint32_t k = (uint32_t)frames[q];
    if (k >= K) continue;                                        // the caller's list is checked; never read outside depth
    const double* Ed = extr + 16 * (size_t)k;
    float E[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) E[a] = (float)Ed[a];
    const float* dk = depth + (size_t)k * H * W;
    const float ax = E[0] * px + E[1] * py, ay = E[4] * px + E[5] * py, az = E[8] * px + E[9] * py;
#pragma unroll
    for (int z = 0; z < TS_UNIT; ++z) {
      const float xc = (ax + E[2] * pz[z]) + E[3], yc = (ay + E[6] * pz[z]) + E[7], zc = (az + E[10] * pz[z]) + E[11];
      if (!(zc > 0.0f)) continue;
      const float u = ((xc * fx) / zc + cx) + 0.5f, v = ((yc * fy) / zc + cy) + 0.5f;
      if (!(u >= 1e-4f && u < u_hi && v >= 1e-4f && v < v_hi)) continue;
      const int iu = (int)u, iv = (int)v;
      const float d = dk[(size_t)iv * W + iu];
      const float sdf = (d - zc) * mult[(size_t)iv * W + iu];
      if (!(d > 0.0f && sdf > -trunc)) continue;
      const float t = fminf(1.0f, sdf / trunc);
      tv[z] = (tv[z] * wv[z] + t) / (wv[z] + 1.0f);
      wv[z] = wv[z] + 1.0f;
    }
  }
  float* to = tsdf + ((size_t)b * TS_BLOCK + threadIdx.x) * TS_UNIT;
  float* wo = weight + ((size_t)b * TS_BLOCK + threadIdx.x) * TS_UNIT;
#pragma unroll
  for (int z = 0; z < TS_UNIT; z += 4) {
    *(float4*)(to + z) = make_float4(tv[z], tv[z + 1], tv[z + 2], tv[z + 3]);
    *(float4*)(wo + z) = make_float4(wv[z], wv[z + 1], wv[z + 2], wv[z + 3]);
  }
}

// 48-bit unit key in ts_key's order (the sort key of the caller's unit list), without the frame
__device__ __forceinline__ int64_t ts_unit_key(int ux, int uy, int uz) { return (int64_t)ts_key(ux, uy, uz, 0) >> 16; }

__device__ __forceinline__ int ts_find(const int32_t* __restrict__ units, uint32_t B, int ux, int uy, int uz) {
  if (ux < -32768 || ux > 32767 || uy < -32768 || uy > 32767 || uz < -32768 || uz > 32767) return -1;
  const int64_t want = ts_unit_key(ux, uy, uz);
  uint32_t lo = 0, hi = B;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const int64_t got = ts_unit_key(units[3 * (size_t)mid], units[3 * (size_t)mid + 1], units[3 * (size_t)mid + 2]);
    if (got < want) lo = mid + 1;
    else hi = mid;
  }
  if (lo < B && units[3 * (size_t)lo] == ux && units[3 * (size_t)lo + 1] == uy && units[3 * (size_t)lo + 2] == uz) return (int)lo;
  return -1;
}

template <bool EMIT>
__global__ __launch_bounds__(TS_BLOCK) void tsdf_vertices_kernel(const int32_t* __restrict__ units, uint32_t B,
                                                                 const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                 double vl, int64_t* __restrict__ count,
                                                                 const int64_t* __restrict__ offset, double* __restrict__ verts,
                                                                 uint64_t capacity) {
  __shared__ float tile[TS_TILE * TS_TILE * TS_TILE];
  __shared__ int nb[27];
  __shared__ uint32_t scan[TS_BLOCK];
  const uint32_t b = blockIdx.x;
  const int ux = units[3 * (size_t)b], uy = units[3 * (size_t)b + 1], uz = units[3 * (size_t)b + 2];
  if (threadIdx.x < 27) {
    const int dx = (int)threadIdx.x / 9 - 1, dy = ((int)threadIdx.x / 3) % 3 - 1, dz = (int)threadIdx.x % 3 - 1;
    nb[threadIdx.x] = threadIdx.x == 13 ? (int)b : ts_find(units, B, ux + dx, uy + dy, uz + dz);
  }
  __syncthreads();
  const float nan = __int_as_float(0x7fc00000);
  for (int c = threadIdx.x; c < TS_TILE * TS_TILE * TS_TILE; c += TS_BLOCK) {
    const int tx = c / (TS_TILE * TS_TILE), ty = (c / TS_TILE) % TS_TILE, tz = c % TS_TILE;
    const int gx = tx - 1, gy = ty - 1, gz = tz - 1;             // voxel relative to this unit: -1 .. 16
    const int dx = gx < 0 ? -1 : (gx >= TS_UNIT ? 1 : 0), dy = gy < 0 ? -1 : (gy >= TS_UNIT ? 1 : 0), dz = gz < 0 ? -1 : (gz >= TS_UNIT ? 1 : 0);
    const int u = nb[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
    float val = nan;
    if (u >= 0) {
      const size_t at = (((size_t)u * TS_UNIT + (gx - dx * TS_UNIT)) * TS_UNIT + (gy - dy * TS_UNIT)) * TS_UNIT + (gz - dz * TS_UNIT);
      if (weight[at] > 0.0f) val = tsdf[at];
    }
    tile[c] = val;
  }
  __syncthreads();
  const int x = threadIdx.x / TS_UNIT, y = threadIdx.x % TS_UNIT;
  const int step[3] = {TS_TILE * TS_TILE, TS_TILE, 1};
  uint32_t mask[TS_UNIT];                                        // 3 bits per voxel of this thread's column
  uint32_t n = 0;
#pragma unroll
  for (int z = 0; z < TS_UNIT; ++z) {
    const int p = ((x + 1) * TS_TILE + (y + 1)) * TS_TILE + (z + 1);
    const float fa = tile[p];
    uint32_t m = 0;
    if (fa == fa) {
      for (int e = 0; e < 3; ++e) {
        const float fb = tile[p + step[e]];
        if (!(fb == fb) || ((fa < 0.0f) == (fb < 0.0f))) continue;
        const int s1 = step[(e + 1) % 3], s2 = step[(e + 2) % 3];
        bool any = false;
        for (int o = 0; o < 4 && !any; ++o) {
          const int q = p - (o & 1) * s1 - (o >> 1) * s2;        // the cube's base corner
          bool all = true;
          for (int c = 0; c < 8; ++c) {
            const float f = tile[q + (c & 1) * step[0] + ((c >> 1) & 1) * step[1] + (c >> 2) * step[2]];
            all = all && (f == f);
          }
          any = all;
        }
        if (any) m |= 1u << e;
      }
    }
    mask[z] = m;
    n += (uint32_t)__popc(m);
  }
  const uint32_t incl = block_scan_inclusive<TS_BLOCK>(scan, n);  // over the columns, in voxel order
  if (!EMIT) {
    if (threadIdx.x == TS_BLOCK - 1) count[b] = (int64_t)incl;
    return;
  }
  uint64_t at = (uint64_t)offset[b] + (incl - n);
  for (int z = 0; z < TS_UNIT; ++z) {
    if (!mask[z]) continue;
    const int p = ((x + 1) * TS_TILE + (y + 1)) * TS_TILE + (z + 1);
    const double fa = fabs((double)tile[p]);
    const double base[3] = {0.5 * vl + vl * (double)((int64_t)ux * TS_UNIT + x), 0.5 * vl + vl * (double)((int64_t)uy * TS_UNIT + y),
                            0.5 * vl + vl * (double)((int64_t)uz * TS_UNIT + z)};
    for (int e = 0; e < 3; ++e) {
      if (!((mask[z] >> e) & 1u)) continue;
      const double fb = fabs((double)tile[p + step[e]]);
      const double off = (fa * vl) / (fa + fb);
      if (at < capacity) {
        verts[3 * at] = e == 0 ? base[0] + off : base[0];
        verts[3 * at + 1] = e == 1 ? base[1] + off : base[1];
        verts[3 * at + 2] = e == 2 ? base[2] + off : base[2];
      }
      ++at;
    }
  }
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" int dns_tsdf_touch(const float* depth, const double* pose, uint32_t K, int H, int W, int stride, const double* intr,
                              double voxel_length, double sdf_trunc, uint64_t* table, uint32_t cap, uint32_t* status, void* stream) {
  DNS_REQUIRE(K <= 65535u, "dns_tsdf_touch: K = %u keyframes (at most 65535: the frame is 16 bits of the key)", K);
  DNS_REQUIRE(H >= 1 && W >= 1 && stride >= 1, "dns_tsdf_touch: H, W and stride must be >= 1 (got %d, %d, %d)", H, W, stride);
  DNS_REQUIRE(voxel_length > 0.0 && sdf_trunc > 0.0 && 2.0 * sdf_trunc < TS_UNIT * voxel_length,
              "dns_tsdf_touch: voxel_length and sdf_trunc must be positive with 2 sdf_trunc < 16 voxel_length (got %g, %g)",
              voxel_length, sdf_trunc);
  DNS_REQUIRE(table && status && intr && cap >= 8u, "dns_tsdf_touch: NULL table / status / intr, or fewer than 8 slots");
  hipStream_t st = (hipStream_t)stream;
  int rc = fill_words2(table, 0xffffffffu, 2 * (size_t)cap, status, 0u, 1, st, "dns_tsdf_touch");
  if (rc != DNS_OK) return rc;
  if (K == 0) return DNS_OK;
  DNS_REQUIRE(depth && pose, "dns_tsdf_touch: NULL depth / pose with K > 0");
  const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
  const uint64_t n = (uint64_t)K * Hs * Ws;
  DNS_REQUIRE(n < (1ull << 31) * TS_BLOCK, "dns_tsdf_touch: too many samples");
  DNS_LAUNCH(tsdf_touch_kernel, dim3((uint32_t)((n + TS_BLOCK - 1) / TS_BLOCK)), dim3(TS_BLOCK), 0, st, depth, pose, K, H, W, stride, Hs,
             Ws, intr[0], intr[1], intr[2], intr[3], TS_UNIT * voxel_length, sdf_trunc, table, cap, status);
  return check_launch("dns_tsdf_touch");
}

extern "C" int dns_tsdf_integrate(const int32_t* units, uint32_t B, const int64_t* offset, const int32_t* frames, const float* depth,
                                  const double* extrinsic, const float* mult, uint32_t K, int H, int W, const double* intr,
                                  double voxel_length, double sdf_trunc, float* tsdf, float* weight, void* stream) {
  DNS_REQUIRE(K <= 65535u && H >= 1 && W >= 1, "dns_tsdf_integrate: K = %u (at most 65535), H = %d, W = %d (>= 1)", K, H, W);
  DNS_REQUIRE(voxel_length > 0.0 && sdf_trunc > 0.0, "dns_tsdf_integrate: voxel_length and sdf_trunc must be positive");
  if (B == 0) return DNS_OK;
  DNS_REQUIRE(units && offset && frames && depth && extrinsic && mult && intr && tsdf && weight, "dns_tsdf_integrate: NULL argument");
  DNS_REQUIRE(((uintptr_t)tsdf | (uintptr_t)weight) % 16 == 0, "dns_tsdf_integrate: tsdf / weight must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(tsdf_integrate_kernel, dim3(B), dim3(TS_BLOCK), 0, st, units, offset, frames, depth, extrinsic, mult, K, H, W,
             (float)intr[0], (float)intr[1], (float)intr[2], (float)intr[3], voxel_length, TS_UNIT * voxel_length, (float)sdf_trunc,
             tsdf, weight);
  return check_launch("dns_tsdf_integrate");
}

extern "C" int dns_tsdf_vertex_count(const int32_t* units, uint32_t B, const float* tsdf, const float* weight, int64_t* count,
                                     void* stream) {
  if (B == 0) return DNS_OK;
  DNS_REQUIRE(units && tsdf && weight && count, "dns_tsdf_vertex_count: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(tsdf_vertices_kernel<false>, dim3(B), dim3(TS_BLOCK), 0, st, units, B, tsdf, weight, 0.0, count, (const int64_t*)nullptr,
             (double*)nullptr, (uint64_t)0);
  return check_launch("dns_tsdf_vertex_count");
}

extern "C" int dns_tsdf_vertex_emit(const int32_t* units, uint32_t B, const float* tsdf, const float* weight, double voxel_length,
                                    const int64_t* offset, double* verts, uint64_t capacity, void* stream) {
  DNS_REQUIRE(voxel_length > 0.0, "dns_tsdf_vertex_emit: voxel_length must be positive");
  if (B == 0 || capacity == 0) return DNS_OK;
  DNS_REQUIRE(units && tsdf && weight && offset && verts, "dns_tsdf_vertex_emit: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(tsdf_vertices_kernel<true>, dim3(B), dim3(TS_BLOCK), 0, st, units, B, tsdf, weight, voxel_length, (int64_t*)nullptr, offset,
             verts, capacity);
  return check_launch("dns_tsdf_vertex_emit");
}
