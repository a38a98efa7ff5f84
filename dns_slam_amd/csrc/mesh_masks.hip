// Point masks (Mesher.point_masks, slams/meshing.py:124-291): the split of P points into seen / forecast / unseen against K poses.
//   seen      some pose has the point inside its image (inside_meshing) and the mode's depth rule holds;
//   forecast  not seen, and some pose has it inside the image widened by 1000 px (inside_forecast) under the mode's rule;
//   unseen    the rest.
// Three modes, by the optional inputs:
//   frustum only   no depth rule (get_mask_use_all_frames, :164-201);
//   depth limit    dz < 1.2 max_depth[k] for both masks, dz = -cam_z (:257-271) -- kf_project_kernel's seen rule, the same bits;
//   depth test     ds = bilinear sample of depth[k] at (u, v) (grid_sample, zeros padding, align_corners: pixel i at coordinate i);
//                  seen needs dz < ds + 0.1 and ds - 2.5 < dz; forecast needs dz < m[c,k], the maximum of ds over ALL points of
//                  the point's chunk c (the reference's torch.max(depth_sample) per points_batch_size chunk, :243).
// The depth test is two passes: pm_chunk_max_kernel fills m [n_chunks, K] (wave max -> LDS max -> one integer atomicMax per
// workgroup and pose on an order-preserving key of the float: order-independent, so the table is the same bits for every call),
// pm_kernel<PM_TEST> recomputes ds instead of reading a [P,K] buffer.  No workgroup straddles a chunk: the grid is n_chunks x
// ceil(chunk / 256) workgroups, workgroup b of chunk c owning the points c chunk + 256 b ... of that chunk alone.
// A non-finite (u, v) (cam_z + 1e-8 == 0) samples as 0 and is inside nothing (the reference would carry a NaN into the chunk max).
// Compiled with -ffp-contract=off (Makefile): dev_project.hpp's expressions, and the tap weights as written.
#include <cmath>
#include "common.hpp"
#include "dev_project.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

constexpr int PM_BLOCK = 256;
constexpr int PM_TILE = 256;   // poses staged in LDS at a time (12 KB + 1 KB)
enum PmMode { PM_FRUSTUM = 0, PM_LIMIT = 1, PM_TEST = 2 };

struct PmArgs {
  const float* pts;
  const float* w2c;
  const float* max_depth;   // [K] (PM_LIMIT)
  const float* depths;      // [K,H,W] (PM_TEST)
  uint32_t P, K;
  uint32_t chunk;           // points per chunk, 1 .. P (P outside PM_TEST: one chunk)
  uint32_t bpc;             // workgroups per chunk = ceil(chunk / PM_BLOCK)
  int H, W;
  float fx, fy, cx, cy;
};

// Signed-integer key of a float whose order is the floats' (negative values: the magnitude bits flipped); its own inverse.
__host__ __device__ __forceinline__ int32_t max_key(int32_t bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }
constexpr int32_t KEY_NEG_INF = (int32_t)0xff800000u ^ 0x7fffffff;

// the workgroup's chunk and this thread's point of it
__device__ __forceinline__ bool pm_point(const PmArgs& a, uint32_t& c, uint32_t& p) {
  c = blockIdx.x / a.bpc;
  const uint32_t off = (blockIdx.x - c * a.bpc) * PM_BLOCK + threadIdx.x;      // < chunk + 256
  p = c * a.chunk + off;                                                      // c chunk < P < 2^31: no wrap
  return off < a.chunk && p < a.P;
}

// Bilinear sample of the image d [H,W] at (u, v), pixel i at coordinate i, taps outside the image 0: the four weights and the
// order of the sum are grid_sample's (nw, ne, sw, se).
__device__ __forceinline__ float sample_depth(const float* __restrict__ d, int H, int W, float u, float v) {
  if (!(fabsf(u) < INFINITY && fabsf(v) < INFINITY)) return 0.f;
  const float x0f = floorf(u), y0f = floorf(v);
  if (!(x0f >= -1.f && x0f <= (float)(W - 1) && y0f >= -1.f && y0f <= (float)(H - 1))) return 0.f;      // no tap inside
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
  const float x1f = x0f + 1.f, y1f = y0f + 1.f;
  const float nw = (x1f - u) * (y1f - v), ne = (u - x0f) * (y1f - v), sw = (x1f - u) * (v - y0f), se = (u - x0f) * (v - y0f);
  const bool xl = x0 >= 0, xr = x1 < W, yt = y0 >= 0, yb = y1 < H;
  float s = 0.f;
  if (xl && yt) s += d[(size_t)y0 * W + x0] * nw;
  if (xr && yt) s += d[(size_t)y0 * W + x1] * ne;
  if (xl && yb) s += d[(size_t)y1 * W + x0] * sw;
  if (xr && yb) s += d[(size_t)y1 * W + x1] * se;
  return s;
}

// pass 1 of the depth test: m [n_chunks, K] keys, preset to KEY_NEG_INF by the caller
__global__ __launch_bounds__(PM_BLOCK) void pm_chunk_max_kernel(PmArgs a, int32_t* __restrict__ m) {
  __shared__ float s_w[PM_TILE * 12];
  __shared__ int32_t s_k[PM_TILE];
  uint32_t c, p;
  const bool live = pm_point(a, c, p);
  const float3 pt = load_point3(a.pts, p, live);
  const bool wave_live = __ballot(live) != 0;
  const size_t hw = (size_t)a.H * a.W;
  for (uint32_t lo = 0; lo < a.K; lo += PM_TILE) {
    const int n = (int)min((uint32_t)PM_TILE, a.K - lo);
    __syncthreads();
    stage_poses<PM_BLOCK>(s_w, a.w2c, lo, n);
    for (int x = threadIdx.x; x < n; x += PM_BLOCK) s_k[x] = KEY_NEG_INF;
    __syncthreads();
    if (wave_live) {
      for (int kk = 0; kk < n; ++kk) {
        int32_t key = KEY_NEG_INF;
        if (live) {
          const Projected q = project(s_w + kk * 12, pt, a.fx, a.fy, a.cx, a.cy, PROJ_EPS_MESHING);
          key = max_key(__float_as_int(sample_depth(a.depths + (size_t)(lo + kk) * hw, a.H, a.W, q.u, q.v)));
        }
        key = wave_max(key);
        if (threadIdx.x % WAVE == 0) atomicMax(&s_k[kk], key);
      }
    }
    __syncthreads();
    for (int x = threadIdx.x; x < n; x += PM_BLOCK) atomicMax(&m[(size_t)c * a.K + lo + x], s_k[x]);
  }
}

template <int MODE>
__global__ __launch_bounds__(PM_BLOCK) void pm_kernel(PmArgs a, const int32_t* __restrict__ m, uint8_t* __restrict__ cls) {
  __shared__ float s_w[PM_TILE * 12];
  __shared__ float s_d[PM_TILE];          // the depth below which pose k forecasts (and, PM_LIMIT, sees)
  uint32_t c, p;
  const bool live = pm_point(a, c, p);
  const float3 pt = load_point3(a.pts, p, live);
  const float fW = (float)a.W, fH = (float)a.H;
  const size_t hw = (size_t)a.H * a.W;
  bool seen = false, fore = false;
  for (uint32_t lo = 0; lo < a.K; lo += PM_TILE) {
    const int n = (int)min((uint32_t)PM_TILE, a.K - lo);
    __syncthreads();
    stage_poses<PM_BLOCK>(s_w, a.w2c, lo, n);
    if (MODE == PM_LIMIT)
      for (int x = threadIdx.x; x < n; x += PM_BLOCK) s_d[x] = a.max_depth[lo + x] * 1.2f;
    if (MODE == PM_TEST)
      for (int x = threadIdx.x; x < n; x += PM_BLOCK) s_d[x] = __int_as_float(max_key(m[(size_t)c * a.K + lo + x]));
    __syncthreads();
    if (live && !seen) {
      for (int kk = 0; kk < n; ++kk) {
        const Projected q = project(s_w + kk * 12, pt, a.fx, a.fy, a.cx, a.cy, PROJ_EPS_MESHING);
        if (!inside_forecast(q, fW, fH)) continue;               // the widened image contains the image
        const float dz = -q.czw;
        const bool in = inside_meshing(q, fW, fH);
        if (MODE == PM_FRUSTUM) {
          fore = true;
          seen = in;
        } else if (MODE == PM_LIMIT) {
          if (dz < s_d[kk]) fore = true, seen = in;
        } else {
          if (dz < s_d[kk]) fore = true;
          if (in) {
            const float ds = sample_depth(a.depths + (size_t)(lo + kk) * hw, a.H, a.W, q.u, q.v);
            seen = dz < ds + 0.1f && ds - 2.5f < dz;
          }
        }
        if (seen) break;                                         // a seen point is not forecast, whatever the other poses say
      }
    }
    if (__syncthreads_and(!live || seen)) break;
  }
  if (live) cls[p] = seen ? 1 : fore ? 2 : 0;
}

// chunk length and grid of a call: outside the depth test the points form one chunk
struct PmGrid {
  uint32_t chunk, bpc;
  uint64_t n_chunks;
};
PmGrid pm_grid(uint32_t P, uint32_t chunk, bool test) {
  PmGrid g;
  g.chunk = test ? (chunk < P ? chunk : P) : P;
  g.bpc = (g.chunk + PM_BLOCK - 1) / PM_BLOCK;
  g.n_chunks = ((uint64_t)P + g.chunk - 1) / g.chunk;
  return g;
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_point_masks_ws_bytes(uint32_t P, uint32_t K, uint32_t chunk) {
  if (P == 0 || K == 0 || chunk == 0 || P >= (1u << 31)) return 0;
  return pm_grid(P, chunk, true).n_chunks * K * sizeof(int32_t);
}

extern "C" int dns_point_masks(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* max_depth, const float* depths,
                               uint32_t chunk, int H, int W, const float* intr, void* ws, uint8_t* cls, void* stream) {
  DNS_REQUIRE(P < (1u << 31), "dns_point_masks: %u points (must be < 2^31)", P);
  DNS_REQUIRE(!(max_depth && depths), "dns_point_masks: max_depth (depth limit) and depths (depth test) exclude each other");
  DNS_REQUIRE(!depths || chunk > 0, "dns_point_masks: the depth test needs chunk > 0 (the reference's points_batch_size)");
  DNS_REQUIRE(depths || chunk == 0, "dns_point_masks: chunk is the depth test's (depths is NULL)");
  DNS_REQUIRE(H > 0 && W > 0, "dns_point_masks: image %d x %d", H, W);
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(pts && cls && intr, "dns_point_masks: NULL argument");
  DNS_REQUIRE(K == 0 || w2c, "dns_point_masks: K > 0 needs w2c");
  const bool test = depths && K > 0;
  DNS_REQUIRE(!test || ws, "dns_point_masks: the depth test needs a workspace of dns_point_masks_ws_bytes");
  const PmGrid g = pm_grid(P, chunk, test);
  const uint64_t n_blocks = g.n_chunks * g.bpc;
  DNS_REQUIRE(n_blocks < (1ull << 31), "dns_point_masks: %llu workgroups (chunk %u of %u points)", (unsigned long long)n_blocks, chunk, P);
  const PmArgs a{pts, w2c, max_depth, depths, P, K, g.chunk, g.bpc, H, W, intr[0], intr[1], intr[2], intr[3]};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((uint32_t)n_blocks), block(PM_BLOCK);
  int32_t* m = (int32_t*)ws;
  if (test) {
    if (int rc = fill_words(m, (uint32_t)KEY_NEG_INF, (size_t)(g.n_chunks * K), st, "dns_point_masks")) return rc;
    DNS_LAUNCH(pm_chunk_max_kernel, grid, block, 0, st, a, m);
    DNS_LAUNCH(pm_kernel<PM_TEST>, grid, block, 0, st, a, m, cls);
  } else if (max_depth && K > 0) {
    DNS_LAUNCH(pm_kernel<PM_LIMIT>, grid, block, 0, st, a, m, cls);
  } else {
    DNS_LAUNCH(pm_kernel<PM_FRUSTUM>, grid, block, 0, st, a, m, cls);      // K = 0: every point unseen
  }
  return check_launch("dns_point_masks");
}
