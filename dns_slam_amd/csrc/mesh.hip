// Mesh extraction (Mesher.get_mesh, slams/meshing.py:562-784): marching cubes over a dense occupancy volume and the keyframe
// projection that gives the query points their class and their seen mask.
//
// Marching cubes is count -> scan -> emit with no atomics: thread = grid point p = (i, j, k) (C order), which owns the three
// grid edges p -> p + 1 along x, y, z (edge index 3 p + axis, the order of the output vertices) and the cube whose lowest
// corner is p (the order of the output faces, then table order).
//   mc_count: per 64-point wave chunk, the ballots of the three edge axes (the vertex rank of any grid edge is then a few
//             popcounts away); per 256-point block, the vertex and triangle counts.
//   mc_scan:  one workgroup: exclusive prefix of the block counts (uint64) and the two totals.
//   mc_emit:  redoes the in-block scan with ballots and LDS, writes its vertices and its cube's triangles; a triangle's
//             corner is the rank of a grid edge, read off the ballots of the edge's chunk.  Every store is checked against
//             the capacities the caller passed.
// Compiled with -ffp-contract=off (Makefile): the vertex positions are the float64 expression tests/mc_ref.py evaluates.
#include <cmath>
#include "common.hpp"
#include "dev_project.hpp"
#include "dev_reduce.hpp"
#define MC_TABLE_SPACE __constant__
#include "mc_table.hpp"

namespace dns {

namespace {

constexpr int MC_BLOCK = 256;
constexpr int MC_WAVES = MC_BLOCK / WAVE;

struct Vec3d {
  double v[3];
};

struct McGrid {
  uint32_t nx, ny, nz;
  uint32_t N;        // nx ny nz
  uint32_t syz;      // ny nz
};

struct McWs {
  uint64_t* masks;   // [n_chunks][3] ballots of the x, y, z edges of 64 consecutive points
  uint32_t* bcount;  // [n_blocks][2] vertices, triangles of 256 consecutive points
  uint64_t* bpre;    // [n_blocks][2] exclusive prefixes of bcount
};

// The parts of N points' workspace into *w; returns its bytes (ws NULL: the size only).  The last part is not padded.
size_t ws_layout(void* ws, uint32_t N, McWs* w) {
  const size_t n_chunks = (N + WAVE - 1) / WAVE, n_blocks = (N + MC_BLOCK - 1) / MC_BLOCK;
  WsCarve c(ws);
  w->masks = c.take<uint64_t>(n_chunks * 3);
  w->bcount = c.take<uint32_t>(n_blocks * 2);
  w->bpre = c.take<uint64_t>(n_blocks * 2);
  return c.end();
}

// The point's 8 cube corners (corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1)); corners outside the grid read as
// outside and are never used: an edge or the cube exists only where all its corners do.
struct McPoint {
  uint32_t i, j, k;
  float v[8];
  bool ex, ey, ez;   // the grid edges along x, y, z start here and cross the level
  uint32_t ncase;    // cube case (0 when there is no cube)
};

__device__ __forceinline__ McPoint load_point(const float* __restrict__ vol, const McGrid g, uint32_t p, float level) {
  McPoint q;
  q.i = p / g.syz;
  const uint32_t r = p - q.i * g.syz;
  q.j = r / g.nz;
  q.k = r - q.j * g.nz;
  const bool hx = q.i + 1 < g.nx, hy = q.j + 1 < g.ny, hz = q.k + 1 < g.nz;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
    const bool ok = (!dx || hx) && (!dy || hy) && (!dz || hz);
    q.v[c] = ok ? vol[p + (dx ? g.syz : 0u) + (dy ? g.nz : 0u) + (dz ? 1u : 0u)] : level;
  }
  const bool in0 = q.v[0] > level;
  q.ex = hx && ((q.v[1] > level) != in0);
  q.ey = hy && ((q.v[2] > level) != in0);
  q.ez = hz && ((q.v[4] > level) != in0);
  uint32_t cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cs |= (q.v[c] > level ? 1u : 0u) << c;
  q.ncase = (hx && hy && hz) ? cs : 0u;
  return q;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const float* __restrict__ vol, McGrid g, float level, McWs ws) {
  __shared__ uint32_t s_v[MC_WAVES], s_t[MC_WAVES];
  const uint32_t p = blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
  bool ex = false, ey = false, ez = false;
  uint32_t nt = 0;
  if (p < g.N) {
    const McPoint q = load_point(vol, g, p, level);
    ex = q.ex, ey = q.ey, ez = q.ez;
    nt = mc_ntri[q.ncase];
  }
  const uint64_t mx = __ballot(ex), my = __ballot(ey), mz = __ballot(ez);
  const uint32_t chunk0 = blockIdx.x * MC_BLOCK + w * WAVE;
  if (lane == 0 && chunk0 < g.N) {
    uint64_t* m = ws.masks + (size_t)(chunk0 / WAVE) * 3;
    m[0] = mx, m[1] = my, m[2] = mz;
  }
  const uint32_t tsum = wave_sum(nt);
  if (lane == 0) {
    s_v[w] = __popcll(mx) + __popcll(my) + __popcll(mz);
    s_t[w] = tsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < MC_WAVES; ++i) a += s_v[i], b += s_t[i];
    ws.bcount[2 * blockIdx.x] = a;
    ws.bcount[2 * blockIdx.x + 1] = b;
  }
}

// One workgroup: dev_reduce.hpp's carry scan of the block counts into uint64 prefixes; the two totals go into totals[0..1].
using McCounts = Counts2<uint64_t>;      // a = vertices, b = triangles
__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_kernel(McWs ws, uint32_t n_blocks, uint64_t* __restrict__ totals) {
  __shared__ McCounts s[SCAN_THREADS];
  const McCounts tot = carry_scan(s, ws.bcount, ws.bpre, n_blocks);
  if (threadIdx.x == SCAN_THREADS - 1) totals[0] = tot.a, totals[1] = tot.b;
}

// rank of grid edge (q, axis) among the crossing edges = its vertex index
__device__ __forceinline__ uint64_t edge_vertex(const McWs ws, uint32_t q, uint32_t axis) {
  const uint32_t blk = q / MC_BLOCK, wq = (q / WAVE) % MC_WAVES, lane = q % WAVE;
  uint64_t r = ws.bpre[2 * blk];
  const uint64_t* m = ws.masks + (size_t)blk * MC_WAVES * 3;
  for (uint32_t w = 0; w < wq; ++w) r += __popcll(m[3 * w]) + __popcll(m[3 * w + 1]) + __popcll(m[3 * w + 2]);
  const uint64_t* mq = m + 3 * wq;
  const uint64_t below = (1ull << lane) - 1;
  r += __popcll(mq[0] & below) + __popcll(mq[1] & below) + __popcll(mq[2] & below);
  if (axis > 0) r += (mq[0] >> lane) & 1;
  if (axis > 1) r += (mq[1] >> lane) & 1;
  return r;
}

__device__ __forceinline__ void put_vertex(float* __restrict__ verts, uint64_t id, uint64_t v_cap, const McPoint& q, uint32_t axis,
                                           float level, const Vec3d& o, const Vec3d& s) {
  if (id >= v_cap) return;
  const float v0 = q.v[0], v1 = q.v[1u << axis];
  const float t = (level - v0) / (v1 - v0);
  const uint32_t idx[3] = {q.i, q.j, q.k};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double p0 = o.v[d] + (double)idx[d] * s.v[d];
    double x = p0;
    if (d == (int)axis) {
      const double p1 = o.v[d] + (double)(idx[d] + 1) * s.v[d];
      x = p0 + (double)t * (p1 - p0);
    }
    verts[3 * id + d] = (float)x;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_kernel(const float* __restrict__ vol, McGrid g, float level, Vec3d o, Vec3d s,
                                                           McWs ws, float* __restrict__ verts, uint64_t v_cap,
                                                           int32_t* __restrict__ faces, uint64_t f_cap) {
  __shared__ uint32_t s_v[MC_WAVES], s_t[MC_WAVES];
  const uint32_t p = blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
  McPoint q;
  uint32_t nt = 0;
  q.ex = q.ey = q.ez = false;
  if (p < g.N) {
    q = load_point(vol, g, p, level);
    nt = mc_ntri[q.ncase];
  }
  const uint64_t mx = __ballot(q.ex), my = __ballot(q.ey), mz = __ballot(q.ez);
  const uint64_t below = (1ull << lane) - 1;
  const uint32_t vrank = __popcll(mx & below) + __popcll(my & below) + __popcll(mz & below);
  uint32_t tinc = nt;                                            // inclusive scan of the triangle counts over the wave
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const uint32_t y = __shfl_up(tinc, off);
    if ((int)lane >= off) tinc += y;
  }
  if (lane == WAVE - 1) {
    s_v[w] = __popcll(mx) + __popcll(my) + __popcll(mz);
    s_t[w] = tinc;
  }
  __syncthreads();
  if (p >= g.N) return;
  uint64_t vb = ws.bpre[2 * blockIdx.x] + vrank, tb = ws.bpre[2 * blockIdx.x + 1] + tinc - nt;
  for (uint32_t i = 0; i < w; ++i) vb += s_v[i], tb += s_t[i];
  if (q.ex) put_vertex(verts, vb++, v_cap, q, 0, level, o, s);
  if (q.ey) put_vertex(verts, vb++, v_cap, q, 1, level, o, s);
  if (q.ez) put_vertex(verts, vb, v_cap, q, 2, level, o, s);
  for (uint32_t tr = 0; tr < nt; ++tr) {
    const uint64_t f = tb + tr;
    if (f >= f_cap) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int e = mc_tri[q.ncase][3 * tr + c];
      const uint32_t qq = p + (mc_edge[e][0] ? g.syz : 0u) + (mc_edge[e][1] ? g.nz : 0u) + (mc_edge[e][2] ? 1u : 0u);
      faces[3 * f + c] = (int32_t)edge_vertex(ws, qq, mc_edge[e][3]);
    }
  }
}

// ---- keyframe projection --------------------------------------------------------------------------------------------------
constexpr int KF_BLOCK = 256;
constexpr int KF_TILE = 256;   // keyframes staged in LDS at a time (17 KB)

__global__ __launch_bounds__(KF_BLOCK) void kf_project_kernel(const float* __restrict__ pts, uint32_t P, const float* __restrict__ w2c,
                                                              uint32_t K, const float* __restrict__ labels,
                                                              const float* __restrict__ max_depth, int H, int W, float fx, float fy,
                                                              float cx, float cy, float* __restrict__ label_out,
                                                              uint8_t* __restrict__ seen_out) {
  __shared__ float s_w[KF_TILE * 12];
  __shared__ float s_d[KF_TILE];
  const uint32_t p = blockIdx.x * KF_BLOCK + threadIdx.x;
  const bool live = p < P;
  const float3 pt = load_point3(pts, p, live);
  bool found = false, seen = false;
  float lab = 0.f;
  const float fW = (float)W, fH = (float)H;
  // keyframes from the last to the first: the label is the last keyframe's that sees the point (get_2d_feature overwrites)
  for (int hi = (int)K; hi > 0; hi -= KF_TILE) {
    const int lo = max(hi - KF_TILE, 0), n = hi - lo;
    __syncthreads();
    stage_poses<KF_BLOCK>(s_w, w2c, (uint32_t)lo, n);
    for (int x = threadIdx.x; x < n; x += KF_BLOCK) s_d[x] = max_depth[lo + x] * 1.2f;
    __syncthreads();
    if (live && !(found && seen)) {
      for (int kk = n - 1; kk >= 0; --kk) {
        const Projected q = project(s_w + kk * 12, pt, fx, fy, cx, cy, PROJ_EPS_MESHING);      // the meshing convention
        if (!inside_meshing(q, fW, fH)) continue;
        if (!found) {
          found = true;
          const int iu = round_pixel(q.u, W), iv = round_pixel(q.v, H);
          lab = labels[((size_t)(lo + kk) * H + iv) * W + iu];
        }
        if (-q.czw < s_d[kk]) seen = true;
        if (seen) break;
      }
    }
    if (__syncthreads_and(!live || (found && seen))) break;
  }
  if (live) {
    label_out[p] = lab;
    seen_out[p] = seen ? 1 : 0;
  }
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_mc_ws_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
  const uint64_t N = (uint64_t)nx * ny * nz;
  if (N == 0 || N >= (1ull << 31)) return 0;
  McWs w;
  return ws_layout(nullptr, (uint32_t)N, &w);
}

static int mc_args(const char* who, uint32_t nx, uint32_t ny, uint32_t nz) {
  const uint64_t N = (uint64_t)nx * ny * nz;
  const uint64_t edges = (uint64_t)(nx ? nx - 1 : 0) * ny * nz + (uint64_t)nx * (ny ? ny - 1 : 0) * nz + (uint64_t)nx * ny * (nz ? nz - 1 : 0);
  DNS_REQUIRE(edges < (1ull << 31) && N < (1ull << 31), "%s: grid %u x %u x %u has %llu edges (must be < 2^31)", who, nx, ny, nz,
              (unsigned long long)edges);
  return DNS_OK;
}

extern "C" int dns_mc_count(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void* ws, uint64_t* totals,
                            void* stream) {
  if (int rc = mc_args("dns_mc_count", nx, ny, nz)) return rc;
  DNS_REQUIRE(totals, "dns_mc_count: NULL totals");
  const uint64_t N = (uint64_t)nx * ny * nz;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return fill_words(totals, 0u, 4, st, "dns_mc_count");
  DNS_REQUIRE(vol && ws, "dns_mc_count: NULL argument");
  const McGrid g{nx, ny, nz, (uint32_t)N, ny * nz};
  McWs w;
  ws_layout(ws, g.N, &w);
  const uint32_t n_blocks = (g.N + MC_BLOCK - 1) / MC_BLOCK;
  DNS_LAUNCH(mc_count_kernel, dim3(n_blocks), dim3(MC_BLOCK), 0, st, vol, g, level, w);
  DNS_LAUNCH(mc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, w, n_blocks, totals);
  return check_launch("dns_mc_count");
}

extern "C" int dns_mc_emit(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const double* origin,
                           const double* spacing, const void* ws, float* verts, uint64_t v_cap, int32_t* faces, uint64_t f_cap,
                           void* stream) {
  if (int rc = mc_args("dns_mc_emit", nx, ny, nz)) return rc;
  DNS_REQUIRE(origin && spacing, "dns_mc_emit: NULL origin / spacing");
  Vec3d o, s;
  for (int d = 0; d < 3; ++d) {
    DNS_REQUIRE(std::isfinite(spacing[d]) && std::isfinite(origin[d]), "dns_mc_emit: non-finite origin / spacing");
    o.v[d] = origin[d], s.v[d] = spacing[d];
  }
  const uint64_t N = (uint64_t)nx * ny * nz;
  if (N == 0 || (v_cap == 0 && f_cap == 0)) return DNS_OK;
  DNS_REQUIRE(vol && ws, "dns_mc_emit: NULL argument");
  DNS_REQUIRE(v_cap == 0 || verts, "dns_mc_emit: NULL verts with v_cap > 0");
  DNS_REQUIRE(f_cap == 0 || faces, "dns_mc_emit: NULL faces with f_cap > 0");
  const McGrid g{nx, ny, nz, (uint32_t)N, ny * nz};
  McWs w;
  ws_layout(const_cast<void*>(ws), g.N, &w);
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(mc_emit_kernel, dim3((g.N + MC_BLOCK - 1) / MC_BLOCK), dim3(MC_BLOCK), 0, st, vol, g, level, o, s, w, verts, v_cap,
             faces, f_cap);
  return check_launch("dns_mc_emit");
}

extern "C" int dns_keyframe_project(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* labels,
                                    const float* max_depth, int H, int W, const float* intr, float* label, uint8_t* seen,
                                    void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(pts && label && seen && intr, "dns_keyframe_project: NULL argument");
  DNS_REQUIRE(K == 0 || (w2c && labels && max_depth), "dns_keyframe_project: K > 0 needs w2c, labels and max_depth");
  DNS_REQUIRE(H > 0 && W > 0, "dns_keyframe_project: image %d x %d", H, W);
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(kf_project_kernel, dim3((P + KF_BLOCK - 1) / KF_BLOCK), dim3(KF_BLOCK), 0, st, pts, P, w2c, K, labels, max_depth, H, W,
             intr[0], intr[1], intr[2], intr[3], label, seen);
  return check_launch("dns_keyframe_project");
}
