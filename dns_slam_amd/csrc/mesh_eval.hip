// Mesh evaluation (the reference's eval_3d.py / cull_mesh.py): nearest reference point of every query, the ICP alignment built
// on it (dns_icp_point_to_point, described at its kernels below), and the frustum test.
//
// dns_nearest_points: for each query the Euclidean distance to the nearest of M reference points and that point's index
// (cKDTree(ref).query(query) of eval_3d.py:24-42), over a uniform cell grid of the reference cloud:
//   nn_init:    cell counters, status and the bounding box words cleared.
//   nn_box:     bounding box of the finite reference points (block reduction, six ordered-integer atomics per block) and the
//               non-finite flags of both clouds (status[0]).
//   nn_header:  one thread sizes the grid: about two cells per point (clouds sampled from surfaces leave most cells empty),
//               at most 2^21, near-cubic cells; an axis of zero (or unusable) extent gets one cell and inv = 0.
//   nn_count / nn_scan_* / nn_fill: counting sort of the points by cell (z fastest).  Integer atomics on the cell counters:
//               with a few points per cell the adds are spread over as many addresses as there are occupied cells, and
//               three small launches replace a device radix sort of (key, index) pairs.  The order inside a cell depends on
//               scheduling; the query's result does not, because equal distances are decided by the smaller index.
//   nn_query:   thread = query.  The query is clamped to the box (a projection onto a box never increases the distance to a
//               point in the box), its cell found with the expression that assigned the points, and the cells are visited in
//               growing Chebyshev rings, a z-row of cells being one contiguous range of the sorted points.  After ring r a
//               point not yet seen lies, on some axis d, in a cell >= c_d + r + 1 or <= c_d - r - 1.  With t(x) = fl(fl(x - lo)
//               * inv) the cell coordinate (monotone in x, relative error below 2^-23) such a point has t >= B = c_d + r + 1,
//               so its distance on that axis is at least ((B - t(q)) - slack_d) * cellw_d, slack_d = 2^-21 (dim_d + 1) covering
//               the rounding of both t and cellw_d = (1 - 2^-20) / inv rounded down; a side with no cells left bounds nothing.
//               The search stops once best <= (min over the sides)^2.  A query that reaches max_ring rings without stopping
//               is appended to the todo list with the best candidate it has.
//   nn_brute:   tiled all pairs over the todo list: a workgroup holds 256 queries in registers, walks an 8192-point chunk of
//               the reference cloud through LDS tiles and merges through a 64-bit atomicMin on (distance^2 bits, index).
//               With DNS_NEAREST_BRUTE every query goes this way (nn_pack instead of the grid build): the baseline the grid
//               is timed against.
//   nn_finish:  distance and index of the todo queries from the packed minimum.
// Every pair distance is the same fp32 expression (dx dx + dy dy + dz dz, compiled with -ffp-contract=off), and the minimum of
// a set does not depend on the order: grid and brute force return identical distances, identical over repeated calls.
//
// dns_frustum_seen: check_proj of eval_3d.py:62-88 / the loop of cull_mesh.py:53-74 for all poses: thread = point, poses in
// LDS tiles, a workgroup leaves at the first tile after which all its points are seen.
#include <algorithm>
#include "common.hpp"
#include "dev_project.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

constexpr int NN_BLOCK = 256;
constexpr uint32_t NN_CELLS_CAP = 1u << 21;
constexpr int NN_SCAN_PER = 8;                                   // cells per thread of the scan kernels
constexpr uint32_t NN_SCAN_TILE = NN_BLOCK * NN_SCAN_PER;        // 2048 cells per workgroup, at most 1024 workgroups
constexpr int NN_SUMS_BLOCK = 1024;
constexpr int NN_BOX_BLOCK = 1024, NN_BOX_GRID = 64;
constexpr int NN_BRUTE_TILE = 1024;                              // reference points per LDS tile (16 KiB)
constexpr uint32_t NN_BRUTE_CHUNK = 8192;                        // reference points per workgroup
constexpr uint32_t NN_BRUTE_GRID_Y = 256;                        // query tiles walked with this stride
constexpr uint32_t NN_BAD_REF = 1u, NN_BAD_QUERY = 2u;           // status[0] bits
constexpr uint64_t NN_NONE = 0x7f800000ffffffffull;              // (+inf, no index)

struct NnHeader {                                                // first 256 bytes of the workspace
  uint32_t box[6];                                               // ordered-integer min xyz, max xyz
  float lo[3], hi[3], inv[3], cellw[3], slack[3];
  int32_t dim[3];
  uint32_t n_cells;
};

struct NnWs {
  NnHeader* head;
  uint32_t* count;       // [cells_alloc + 1]
  uint32_t* start;       // [cells_alloc + 1]
  uint32_t* sums;        // [1024]
  uint32_t* point_cell;  // [M]
  float4* sorted;        // [M] (x, y, z, index bits)
  uint32_t* todo;        // [N]
  uint64_t* best;        // [N]
  uint32_t target, cells_alloc;
};

inline uint32_t cells_target(uint32_t M) {
  const uint64_t t = 2ull * M;
  return (uint32_t)(t < 1 ? 1 : (t > NN_CELLS_CAP ? NN_CELLS_CAP : t));
}

// The nearest-point parts of M reference points and N queries, taken from c into *w (icp_layout goes on from there).
void nn_take(WsCarve& c, uint32_t M, uint32_t N, NnWs* w) {
  w->target = cells_target(M);
  w->cells_alloc = (w->target + NN_SCAN_TILE - 1) / NN_SCAN_TILE * NN_SCAN_TILE;
  w->head = c.take<NnHeader>(1);
  w->count = c.take<uint32_t>((uint64_t)w->cells_alloc + 1);
  w->start = c.take<uint32_t>((uint64_t)w->cells_alloc + 1);
  w->sums = c.take<uint32_t>(1024);
  w->point_cell = c.take<uint32_t>(M);
  w->sorted = c.take<float4>(M);
  w->todo = c.take<uint32_t>(N);
  w->best = c.take<uint64_t>(N);
}

// dns_nearest_points' workspace into *w; returns its bytes (ws NULL: the size only).
size_t nn_layout(void* ws, uint32_t M, uint32_t N, NnWs* w) {
  WsCarve c(ws);
  nn_take(c, M, N, w);
  return c.end256();
}

__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__global__ __launch_bounds__(NN_BLOCK) void nn_init_kernel(NnWs w, bool grid, uint32_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (grid && t <= w.cells_alloc) w.count[t] = 0u;
  if (t < 4) status[t] = 0u;
  if (t < 3) w.head->box[t] = 0xffffffffu, w.head->box[3 + t] = 0u;
}

__global__ __launch_bounds__(NN_BOX_BLOCK) void nn_box_kernel(const float* __restrict__ ref, uint32_t M, const float* __restrict__ query,
                                                              uint32_t N, NnHeader* __restrict__ head, uint32_t* __restrict__ status) {
  __shared__ float s_v[6][NN_BOX_BLOCK / WAVE];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0u;
  __syncthreads();
  const float inf = __builtin_inff();
  float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  uint32_t bad = 0u;
  const uint32_t stride = gridDim.x * NN_BOX_BLOCK, t0 = blockIdx.x * NN_BOX_BLOCK + threadIdx.x;
  for (uint32_t i = t0; i < M; i += stride) {
    const float x = ref[3 * (size_t)i], y = ref[3 * (size_t)i + 1], z = ref[3 * (size_t)i + 2];
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      mn[0] = fminf(mn[0], x), mn[1] = fminf(mn[1], y), mn[2] = fminf(mn[2], z);
      mx[0] = fmaxf(mx[0], x), mx[1] = fmaxf(mx[1], y), mx[2] = fmaxf(mx[2], z);
    } else {
      bad |= NN_BAD_REF;
    }
  }
  for (uint32_t i = t0; i < N; i += stride) {
    const float x = query[3 * (size_t)i], y = query[3 * (size_t)i + 1], z = query[3 * (size_t)i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) bad |= NN_BAD_QUERY;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[d] = fminf(mn[d], __shfl_xor(mn[d], o));
      mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o));
    }
  if (bad) atomicOr(&s_bad, bad);
  const int lane = threadIdx.x % WAVE, wv = threadIdx.x / WAVE;
  if (lane == 0)
    for (int d = 0; d < 3; ++d) s_v[d][wv] = mn[d], s_v[3 + d][wv] = mx[d];
  __syncthreads();
  if (threadIdx.x < 6) {
    const bool is_min = threadIdx.x < 3;
    float v = s_v[threadIdx.x][0];
    for (int k = 1; k < NN_BOX_BLOCK / WAVE; ++k) v = is_min ? fminf(v, s_v[threadIdx.x][k]) : fmaxf(v, s_v[threadIdx.x][k]);
    if (is_min) {
      if (v < inf) atomicMin(&head->box[threadIdx.x], f2ord(v));
    } else {
      if (v > -inf) atomicMax(&head->box[threadIdx.x], f2ord(v));
    }
  }
  if (threadIdx.x == 0 && s_bad) atomicOr(&status[0], s_bad);
}

__global__ void nn_header_kernel(NnHeader* __restrict__ h, uint32_t target, uint32_t* __restrict__ status) {
  if (threadIdx.x || blockIdx.x) return;
  const bool ok = (status[0] & NN_BAD_REF) == 0u;
  double ext[3], vol = 1.0;
  bool live[3];
  int k = 0;
  for (int d = 0; d < 3; ++d) {
    const float lo = ok ? ord2f(h->box[d]) : 0.f, hi = ok ? ord2f(h->box[3 + d]) : 0.f;
    h->lo[d] = lo, h->hi[d] = hi;
    ext[d] = (double)hi - (double)lo;
    live[d] = ok && ext[d] >= 1e-30 && ext[d] <= 1e30;
    if (live[d]) vol *= ext[d], ++k;
  }
  // near-cubic cells of volume (box volume) / target over the axes at least one cell long; a shorter axis gets one cell and
  // leaves the product (three rounds at the most).  Rounding the counts down keeps their product at or under target.
  double cell = 1.0;
  for (int round = 0; round < 3 && k; ++round) {
    cell = pow(vol / (double)target, 1.0 / k);
    bool changed = false;
    for (int d = 0; d < 3; ++d)
      if (live[d] && !(ext[d] >= cell)) live[d] = false, changed = true;
    if (!changed) break;
    vol = 1.0, k = 0;
    for (int d = 0; d < 3; ++d)
      if (live[d]) vol *= ext[d], ++k;
  }
  int64_t dim[3];
  for (int d = 0; d < 3; ++d) {
    double n = live[d] && cell > 0.0 ? floor(ext[d] / cell) : 1.0;
    n = n >= 1.0 ? n : 1.0;                                      // also a NaN
    dim[d] = (int64_t)(n > (double)target ? (double)target : n);
  }
  while (dim[0] * dim[1] * dim[2] > (int64_t)target) {           // only through the rounding of pow and the quotients
    const int a = dim[0] >= dim[1] ? (dim[0] >= dim[2] ? 0 : 2) : (dim[1] >= dim[2] ? 1 : 2);
    --dim[a];
  }
  for (int d = 0; d < 3; ++d) {
    float inv = dim[d] > 1 ? (float)((double)dim[d] / ext[d]) : 0.f;
    if (!(inv >= 1e-30f && inv <= 1e30f)) inv = 0.f, dim[d] = 1;
    h->inv[d] = inv;
    h->dim[d] = (int32_t)dim[d];
    // rounded towards zero: never above (1 - 2^-20) / inv
    h->cellw[d] = inv > 0.f ? __double2float_rz((1.0 - 0x1p-20) / (double)inv) : 0.f;
    h->slack[d] = (float)(dim[d] + 1) * 0x1p-21f;
  }
  h->n_cells = (uint32_t)(dim[0] * dim[1] * dim[2]);
  status[2] = h->n_cells;
}

// The cell coordinate of x on one axis; the SAME expression places the points and bounds the search (two roundings: the file is
// compiled with -ffp-contract=off).
__device__ __forceinline__ float nn_t(float x, float lo, float inv) { return (x - lo) * inv; }
__device__ __forceinline__ int nn_cell(float t, int dim) { return (int)fminf(fmaxf(floorf(t), 0.f), (float)(dim - 1)); }

__device__ __forceinline__ uint64_t nn_pack(float4 p, float qx, float qy, float qz) {
  const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
  const float d2 = dx * dx + dy * dy + dz * dz;                  // >= +0, or NaN (whose bits order above +inf's)
  return ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)__float_as_uint(p.w);
}

__global__ __launch_bounds__(NN_BLOCK) void nn_count_kernel(const float* __restrict__ ref, uint32_t M, NnWs w) {
  const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= M) return;
  const NnHeader* h = w.head;
  const int cx = nn_cell(nn_t(ref[3 * (size_t)i], h->lo[0], h->inv[0]), h->dim[0]);
  const int cy = nn_cell(nn_t(ref[3 * (size_t)i + 1], h->lo[1], h->inv[1]), h->dim[1]);
  const int cz = nn_cell(nn_t(ref[3 * (size_t)i + 2], h->lo[2], h->inv[2]), h->dim[2]);
  const uint32_t c = ((uint32_t)cx * (uint32_t)h->dim[1] + (uint32_t)cy) * (uint32_t)h->dim[2] + (uint32_t)cz;   // < n_cells
  w.point_cell[i] = c;
  atomicAdd(&w.count[c], 1u);
}

// exclusive scan of count[0 .. cells_alloc) into start: per-workgroup totals, their scan by one workgroup, the local scans
__global__ __launch_bounds__(NN_BLOCK) void nn_scan_sums_kernel(NnWs w) {
  __shared__ uint32_t s[NN_BLOCK / WAVE];
  const uint32_t base = blockIdx.x * NN_SCAN_TILE + threadIdx.x * NN_SCAN_PER;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k) v += w.count[base + k];
  v = wave_sum(v);
  if (threadIdx.x % WAVE == 0) s[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) w.sums[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(NN_SUMS_BLOCK) void nn_scan_top_kernel(NnWs w, uint32_t n_blocks) {
  __shared__ uint32_t s[NN_SUMS_BLOCK];
  const uint32_t t = threadIdx.x;
  const uint32_t own = t < n_blocks ? w.sums[t] : 0u;
  const uint32_t incl = block_scan_inclusive<NN_SUMS_BLOCK>(s, own);
  if (t < n_blocks) w.sums[t] = incl - own;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_scan_local_kernel(NnWs w, uint32_t M) {
  __shared__ uint32_t s[NN_BLOCK];
  const uint32_t t = threadIdx.x, base = blockIdx.x * NN_SCAN_TILE + t * NN_SCAN_PER;
  uint32_t c[NN_SCAN_PER], own = 0;
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k) c[k] = w.count[base + k], own += c[k];
  uint32_t run = w.sums[blockIdx.x] + block_scan_inclusive<NN_BLOCK>(s, own) - own;
#pragma unroll
  for (int k = 0; k < NN_SCAN_PER; ++k) {
    w.start[base + k] = run;
    run += c[k];
  }
  if (blockIdx.x == gridDim.x - 1 && t == NN_BLOCK - 1) w.start[w.cells_alloc] = M;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_fill_kernel(const float* __restrict__ ref, uint32_t M, NnWs w) {
  const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= M) return;
  const uint32_t c = w.point_cell[i];
  const uint32_t k = atomicSub(&w.count[c], 1u) - 1u;            // count[c] holds the cell's population once more
  const uint32_t pos = w.start[c] + k;
  if (pos < M) w.sorted[pos] = make_float4(ref[3 * (size_t)i], ref[3 * (size_t)i + 1], ref[3 * (size_t)i + 2], __uint_as_float(i));
}

__global__ __launch_bounds__(NN_BLOCK) void nn_pack_kernel(const float* __restrict__ ref, uint32_t M, uint32_t N, NnWs w,
                                                           uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i < M) w.sorted[i] = make_float4(ref[3 * (size_t)i], ref[3 * (size_t)i + 1], ref[3 * (size_t)i + 2], __uint_as_float(i));
  if (i < N) w.todo[i] = i, w.best[i] = NN_NONE;
  if (i == 0) status[1] = N;
}

__device__ __forceinline__ uint64_t nn_range(const float4* __restrict__ sorted, uint32_t s, uint32_t e, float qx, float qy, float qz,
                                             uint64_t best) {
  for (uint32_t j = s; j < e; ++j) {
    const uint64_t pk = nn_pack(sorted[j], qx, qy, qz);
    best = pk < best ? pk : best;
  }
  return best;
}

// The ring search of one query qv: -> true with the packed minimum in `best` once it is decided, false after max_ring rings.
// BOUNDED (the ICP correspondence search): the search is also over -- with whatever candidate it holds, none of them within the
// radius -- once the lower bound of every unseen point exceeds the radius (lb^2 > stop_d2, stop_d2 at or above every d2 the
// correspondence rule accepts).
template <bool BOUNDED>
__device__ __forceinline__ bool nn_search(const NnWs& w, uint32_t M, const float (&qv)[3], uint32_t max_ring, float stop_d2,
                                          uint64_t& best) {
  const NnHeader* h = w.head;
  float t[3], slack[3], cellw[3];
  int c[3], dim[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    dim[d] = h->dim[d], slack[d] = h->slack[d], cellw[d] = h->cellw[d];
    t[d] = nn_t(fminf(fmaxf(qv[d], h->lo[d]), h->hi[d]), h->lo[d], h->inv[d]);     // a NaN coordinate clamps to lo
    c[d] = nn_cell(t[d], dim[d]);
  }
  const uint32_t* __restrict__ start = w.start;
  const float4* __restrict__ sorted = w.sorted;
  for (uint32_t ring = 0; ring <= max_ring; ++ring) {
    const int r = (int)ring;
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, dim[0] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, dim[1] - 1);
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, dim[2] - 1);
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) {
        const uint32_t row = ((uint32_t)x * (uint32_t)dim[1] + (uint32_t)y) * (uint32_t)dim[2];
        if (abs(x - c[0]) == r || abs(y - c[1]) == r) {            // a face of the ring: the whole z-row is one range
          best = nn_range(sorted, start[row + z0], min(start[row + z1 + 1], M), qv[0], qv[1], qv[2], best);
        } else {                                                   // inside: the row's two end cells
          if (c[2] - r >= 0) best = nn_range(sorted, start[row + c[2] - r], min(start[row + c[2] - r + 1], M), qv[0], qv[1], qv[2], best);
          if (c[2] + r < dim[2]) best = nn_range(sorted, start[row + c[2] + r], min(start[row + c[2] + r + 1], M), qv[0], qv[1], qv[2], best);
        }
      }
    float lb = __builtin_inff();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int up = c[d] + r + 1, dn = c[d] - r;                  // unseen cells: >= up, < dn
      if (up <= dim[d] - 1) lb = fminf(lb, fmaxf(((float)up - t[d]) - slack[d], 0.f) * cellw[d]);
      if (dn >= 1) lb = fminf(lb, fmaxf((t[d] - (float)dn) - slack[d], 0.f) * cellw[d]);
    }
    if (__uint_as_float((uint32_t)(best >> 32)) <= lb * lb) return true;      // lb = inf: every cell has been seen
    if (BOUNDED && lb * lb > stop_d2) return true;
  }
  return false;
}

__global__ __launch_bounds__(NN_BLOCK) void nn_query_kernel(NnWs w, uint32_t M, const float* __restrict__ query, uint32_t N,
                                                            uint32_t max_ring, float* __restrict__ dist, int32_t* __restrict__ idx,
                                                            uint32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (q >= N) return;
  const float qv[3] = {query[3 * (size_t)q], query[3 * (size_t)q + 1], query[3 * (size_t)q + 2]};
  uint64_t best = NN_NONE;
  if (nn_search<false>(w, M, qv, max_ring, 0.f, best)) {
    dist[q] = sqrtf(__uint_as_float((uint32_t)(best >> 32)));
    idx[q] = (int32_t)(uint32_t)best;
  } else {
    const uint32_t pos = atomicAdd(&status[1], 1u);
    if (pos < N) w.todo[pos] = q;
    w.best[q] = best;
  }
}

__global__ __launch_bounds__(NN_BLOCK) void nn_brute_kernel(NnWs w, uint32_t M, const float* __restrict__ query, uint32_t N,
                                                            const uint32_t* __restrict__ status) {
  __shared__ float4 tile[NN_BRUTE_TILE];
  const uint32_t n_todo = min(status[1], N);
  const uint32_t j0 = blockIdx.x * NN_BRUTE_CHUNK, j1 = min(j0 + NN_BRUTE_CHUNK, M);
  for (uint32_t tq = blockIdx.y; (uint64_t)tq * NN_BLOCK < n_todo; tq += gridDim.y) {
    const uint32_t i = tq * NN_BLOCK + threadIdx.x;
    const bool live = i < n_todo;
    const uint32_t q = live ? min(w.todo[i], N - 1) : 0u;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) qx = query[3 * (size_t)q], qy = query[3 * (size_t)q + 1], qz = query[3 * (size_t)q + 2];
    uint64_t best = NN_NONE;
    for (uint32_t b = j0; b < j1; b += NN_BRUTE_TILE) {
      const uint32_t n = min((uint32_t)NN_BRUTE_TILE, j1 - b);
      __syncthreads();
      for (uint32_t x = threadIdx.x; x < n; x += NN_BLOCK) tile[x] = w.sorted[b + x];
      __syncthreads();
      if (live)
        for (uint32_t x = 0; x < n; ++x) {
          const uint64_t pk = nn_pack(tile[x], qx, qy, qz);
          best = pk < best ? pk : best;
        }
    }
    if (live && best < __hip_atomic_load(&w.best[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin((unsigned long long*)&w.best[q], (unsigned long long)best);
  }
}

__global__ __launch_bounds__(NN_BLOCK) void nn_finish_kernel(NnWs w, uint32_t N, float* __restrict__ dist, int32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= min(status[1], N)) return;
  const uint32_t q = min(w.todo[i], N - 1);
  const uint64_t best = w.best[q];
  dist[q] = sqrtf(__uint_as_float((uint32_t)(best >> 32)));
  idx[q] = (int32_t)(uint32_t)best;
}

// ---- point-to-point ICP (get_align_transformation of eval_3d.py:45-59) ---------------------------------------------------------
// dns_icp_point_to_point: the grid over the target cloud built once, then max_iter + 1 passes of four launches:
//   icp_query:  thread = source point.  p' = fl32(T p) from the float64 T in the workspace (kept in xf for the kernels after it),
//               the ring search of nn_query bounded by the radius; the packed minimum of EVERY point goes to best[], the
//               undecided ones to the todo list.
//   nn_brute:   the all-pairs finish of the todo list, as in dns_nearest_points.
//   icp_reduce: thread = source point (grid-stride over at most ICP_ROWS workgroups).  The correspondence rule, the 17 float64
//               sums in registers, a butterfly over the wave, the waves through LDS in order, one row per workgroup.
//   icp_solve:  one workgroup adds the rows in a fixed order; one thread applies the stopping rule or computes the rigid update
//               (Horn's quaternion: the eigenvector of the largest eigenvalue of a symmetric 4x4, cyclic Jacobi) and composes it.
// No floating-point atomics anywhere: the result is the same bits for every call.  After the stop `done` is set and every kernel
// of the remaining passes returns at once (the all-pairs kernel over an empty todo list).
constexpr uint32_t ICP_ROWS = 1024;                              // partial rows (workgroups of icp_reduce) at the most
constexpr int ICP_SUMS = 17;                                     // n, sum p' (3), sum q (3), sum q p'^T (9), sum |p' - q|^2
constexpr int ICP_RESULT = 21 + ICP_SUMS;                        // doubles of `result` (include/dns_hip.h)

struct IcpInit {
  double m[16];
};

struct IcpState {
  double T[16];
  double prev_fit, prev_rmse;
  uint32_t qst[4];                                               // qst[1]: the todo count of the pass (the status words nn_brute reads)
  uint32_t done, updates, pad[2];
};

__global__ void icp_begin_kernel(IcpState* __restrict__ s, IcpInit init, uint32_t* __restrict__ status, double* __restrict__ result) {
  if (threadIdx.x || blockIdx.x) return;
  for (int k = 0; k < 16; ++k) s->T[k] = init.m[k], result[k] = init.m[k];
  for (int k = 16; k < ICP_RESULT; ++k) result[k] = 0.0;
  s->prev_fit = 0.0, s->prev_rmse = 0.0;
  for (int k = 0; k < 4; ++k) s->qst[k] = 0u;
  s->updates = 0u;
  const bool bad = status[0] != 0u;                              // a non-finite coordinate: nothing is evaluated
  s->done = bad ? 1u : 0u;
  status[3] = bad ? DNS_ICP_STOP_NONFINITE : DNS_ICP_STOP_MAX_ITER;
}

__global__ __launch_bounds__(NN_BLOCK) void icp_query_kernel(NnWs w, uint32_t M, const float* __restrict__ src, uint32_t N,
                                                             uint32_t max_ring, float stop_d2, IcpState* __restrict__ s,
                                                             float* __restrict__ xf) {
  if (s->done) return;
  const uint32_t q = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (q >= N) return;
  const double* T = s->T;
  const double x = (double)src[3 * (size_t)q], y = (double)src[3 * (size_t)q + 1], z = (double)src[3 * (size_t)q + 2];
  float qv[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) qv[d] = (float)(((T[4 * d] * x + T[4 * d + 1] * y) + T[4 * d + 2] * z) + T[4 * d + 3]);
  xf[3 * (size_t)q] = qv[0], xf[3 * (size_t)q + 1] = qv[1], xf[3 * (size_t)q + 2] = qv[2];
  uint64_t best = NN_NONE;
  const bool decided = nn_search<true>(w, M, qv, max_ring, stop_d2, best);
  w.best[q] = best;
  if (!decided) {
    const uint32_t pos = atomicAdd(&s->qst[1], 1u);
    if (pos < N) w.todo[pos] = q;
  }
}

__global__ __launch_bounds__(NN_BLOCK) void icp_reduce_kernel(NnWs w, const float* __restrict__ tgt, uint32_t M,
                                                              const float* __restrict__ xf, uint32_t N, float max_dist,
                                                              const IcpState* __restrict__ s, double* __restrict__ partial) {
  __shared__ double s_w[NN_BLOCK / WAVE][ICP_SUMS];
  if (s->done) return;
  double a[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) a[k] = 0.0;
  for (uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x; i < N; i += gridDim.x * NN_BLOCK) {
    const uint64_t best = w.best[i];
    const uint32_t j = (uint32_t)best;
    const float d = sqrtf(__uint_as_float((uint32_t)(best >> 32)));
    if (j < M && d <= max_dist) {                                // the correspondence rule (a NaN distance fails it)
      const double p[3] = {(double)xf[3 * (size_t)i], (double)xf[3 * (size_t)i + 1], (double)xf[3 * (size_t)i + 2]};
      const double g[3] = {(double)tgt[3 * (size_t)j], (double)tgt[3 * (size_t)j + 1], (double)tgt[3 * (size_t)j + 2]};
      a[0] += 1.0;
      double d2 = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        a[1 + r] += p[r], a[4 + r] += g[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[7 + 3 * r + c] += g[r] * p[c];
        const double e = p[r] - g[r];
        d2 += e * e;
      }
      a[16] += d2;
    }
  }
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) a[k] = wave_sum(a[k]);
  if (threadIdx.x % WAVE == 0)
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) s_w[threadIdx.x / WAVE][k] = a[k];
  __syncthreads();
  if (threadIdx.x < ICP_SUMS) {
    double v = s_w[0][threadIdx.x];
    for (int k = 1; k < NN_BLOCK / WAVE; ++k) v += s_w[k][threadIdx.x];
    partial[(size_t)blockIdx.x * ICP_SUMS + threadIdx.x] = v;
  }
}

// The eigenvector of the largest eigenvalue of the symmetric 4x4 A (cyclic Jacobi, float64); the first of equal eigenvalues.
__device__ void icp_top_eigenvector(double A[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        all += A[i][j] * A[i][j];
        if (i != j) off += A[i][j] * A[i][j];
      }
    if (!(off > 1e-30 * all)) break;                          // off-diagonal entries under 1e-15 of the matrix
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) {
        if (A[p][r] == 0.0) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 4; ++k) {                            // A <- A J
          const double akp = A[k][p], akr = A[k][r];
          A[k][p] = c * akp - sn * akr, A[k][r] = sn * akp + c * akr;
        }
        for (int k = 0; k < 4; ++k) {                            // A <- J^T A
          const double apk = A[p][k], ark = A[r][k];
          A[p][k] = c * apk - sn * ark, A[r][k] = sn * apk + c * ark;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - sn * vkr, V[k][r] = sn * vkp + c * vkr;
        }
      }
  }
  int top = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[top][top]) top = k;
  double nrm = 0.0;
  for (int k = 0; k < 4; ++k) nrm += V[k][top] * V[k][top];
  nrm = sqrt(nrm);
  for (int k = 0; k < 4; ++k) q[k] = nrm > 0.0 ? V[k][top] / nrm : (k == 0 ? 1.0 : 0.0);
}

__global__ __launch_bounds__(NN_BLOCK) void icp_solve_kernel(const double* __restrict__ partial, uint32_t n_rows, uint32_t N,
                                                             uint32_t pass, uint32_t max_iter, double rel_fit, double rel_rmse,
                                                             IcpState* __restrict__ s, double* __restrict__ result,
                                                             uint32_t* __restrict__ status) {
  __shared__ double s_w[NN_BLOCK / WAVE][ICP_SUMS];
  if (s->done) return;
  double a[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) {
    a[k] = 0.0;
    for (uint32_t r = threadIdx.x; r < n_rows; r += NN_BLOCK) a[k] += partial[(size_t)r * ICP_SUMS + k];
    a[k] = wave_sum(a[k]);
  }
  if (threadIdx.x % WAVE == 0)
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) s_w[threadIdx.x / WAVE][k] = a[k];
  __syncthreads();
  if (threadIdx.x) return;
  double sum[ICP_SUMS];
  for (int k = 0; k < ICP_SUMS; ++k) {
    sum[k] = s_w[0][k];
    for (int v = 1; v < NN_BLOCK / WAVE; ++v) sum[k] += s_w[v][k];
  }
  const double n = sum[0];
  const double fitness = n / (double)N, rmse = n > 0.0 ? sqrt(sum[16] / n) : 0.0;
  status[1] += s->qst[1];
  s->qst[1] = 0u;
  uint32_t stop = 0xffffffffu;                                   // none
  if (pass > 0 && fabs(fitness - s->prev_fit) < rel_fit && fabs(rmse - s->prev_rmse) < rel_rmse)
    stop = DNS_ICP_STOP_CONVERGED;
  else if (pass == max_iter)
    stop = DNS_ICP_STOP_MAX_ITER;
  else if (n < 3.0)
    stop = DNS_ICP_STOP_FEW;
  s->prev_fit = fitness, s->prev_rmse = rmse;
  if (stop == 0xffffffffu) {
    // M[i][j] = sum (p'_i - mean p'_i)(q_j - mean q_j) / n; Horn's N from it; R rotates the p' onto the q
    double Mx[3][3], mp[3], mq[3];
    for (int i = 0; i < 3; ++i) mp[i] = sum[1 + i] / n, mq[i] = sum[4 + i] / n;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Mx[i][j] = sum[7 + 3 * j + i] / n - mp[i] * mq[j];
    double A[4][4] = {
        {Mx[0][0] + Mx[1][1] + Mx[2][2], Mx[1][2] - Mx[2][1], Mx[2][0] - Mx[0][2], Mx[0][1] - Mx[1][0]},
        {Mx[1][2] - Mx[2][1], Mx[0][0] - Mx[1][1] - Mx[2][2], Mx[0][1] + Mx[1][0], Mx[2][0] + Mx[0][2]},
        {Mx[2][0] - Mx[0][2], Mx[0][1] + Mx[1][0], -Mx[0][0] + Mx[1][1] - Mx[2][2], Mx[1][2] + Mx[2][1]},
        {Mx[0][1] - Mx[1][0], Mx[2][0] + Mx[0][2], Mx[1][2] + Mx[2][1], -Mx[0][0] - Mx[1][1] + Mx[2][2]}};
    double qt[4];
    icp_top_eigenvector(A, qt);
    const double qw = qt[0], qx = qt[1], qy = qt[2], qz = qt[3];
    const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
                            {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
                            {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
    double U[3][4], Tn[3][4];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) U[i][j] = R[i][j];
      U[i][3] = mq[i] - (R[i][0] * mp[0] + R[i][1] * mp[1] + R[i][2] * mp[2]);
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j)
        Tn[i][j] = U[i][0] * s->T[j] + U[i][1] * s->T[4 + j] + U[i][2] * s->T[8 + j] + (j == 3 ? U[i][3] : 0.0);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) s->T[4 * i + j] = Tn[i][j];
    s->updates += 1u;
  } else {
    s->done = 1u;
    status[3] = stop;
  }
  for (int k = 0; k < 16; ++k) result[k] = s->T[k];
  result[16] = fitness, result[17] = rmse, result[18] = n, result[19] = (double)s->updates;
  result[20] = stop == DNS_ICP_STOP_CONVERGED ? 1.0 : 0.0;
  for (int k = 0; k < ICP_SUMS; ++k) result[21 + k] = sum[k];
}

// dns_icp_point_to_point's workspace (host side only; the kernels take its members): the nearest-point parts, then its own three.
struct IcpWs {
  NnWs nn;
  IcpState* state;
  float* xf;             // [N][3] the transformed source points of the pass
  double* partial;       // [ICP_ROWS][ICP_SUMS]
};

// Its parts into *w; returns its bytes (ws NULL: the size only).
size_t icp_layout(void* ws, uint32_t M, uint32_t N, IcpWs* w) {
  WsCarve c(ws);
  nn_take(c, M, N, &w->nn);
  w->state = c.take<IcpState>(1);
  w->xf = c.take<float>(3ull * N);
  w->partial = c.take<double>((uint64_t)ICP_ROWS * ICP_SUMS);
  return c.end256();
}

// ---- frustum test --------------------------------------------------------------------------------------------------------
constexpr int FR_BLOCK = 256, FR_TILE = 128;                     // poses per LDS tile (12 floats each)

__global__ __launch_bounds__(FR_BLOCK) void frustum_seen_kernel(const float* __restrict__ pts, uint32_t P, const float* __restrict__ w2c,
                                                                uint32_t K, float fW, float fH, float fx, float fy, float cx, float cy,
                                                                uint8_t* __restrict__ seen_out) {
  __shared__ float s_w[FR_TILE * 12];
  const uint32_t p = blockIdx.x * FR_BLOCK + threadIdx.x;
  const bool live = p < P;
  const float3 pt = load_point3(pts, p, live);
  bool seen = false;
  for (uint32_t lo = 0; lo < K; lo += FR_TILE) {
    const int n = (int)min((uint32_t)FR_TILE, K - lo);
    __syncthreads();
    stage_poses<FR_BLOCK>(s_w, w2c, lo, n);
    __syncthreads();
    if (live && !seen) {
      for (int kk = 0; kk < n; ++kk) {
        if (inside_eval(project(s_w + kk * 12, pt, fx, fy, cx, cy, PROJ_EPS_EVAL), fW, fH)) {      // the evaluation convention
          seen = true;
          break;
        }
      }
    }
    if (__syncthreads_and(!live || seen)) break;
  }
  if (live) seen_out[p] = seen ? 1 : 0;
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_nearest_ws_bytes(uint32_t M, uint32_t N) {
  if (M >= (1u << 31) || N >= (1u << 31)) return 0;
  NnWs w;
  return nn_layout(nullptr, M, N, &w);
}

namespace {

inline dim3 nn_blocks(uint64_t n) { return dim3((uint32_t)((n + NN_BLOCK - 1) / NN_BLOCK)); }

// cleared counters and status, the box of ref and the non-finite flags of both clouds
void nn_launch_box(const NnWs& w, bool grid, const float* ref, uint32_t M, const float* query, uint32_t N, uint32_t* status,
                   hipStream_t st) {
  DNS_LAUNCH(nn_init_kernel, nn_blocks(grid ? (uint64_t)w.cells_alloc + 1 : 4), dim3(NN_BLOCK), 0, st, w, grid, status);
  const uint32_t box_grid = (uint32_t)std::min<uint64_t>(NN_BOX_GRID, ((uint64_t)std::max(M, N) + NN_BOX_BLOCK - 1) / NN_BOX_BLOCK);
  DNS_LAUNCH(nn_box_kernel, dim3(box_grid), dim3(NN_BOX_BLOCK), 0, st, ref, M, query, N, w.head, status);
}

// the build half: the cell grid over ref (after nn_launch_box), queried any number of times
void nn_launch_build(const NnWs& w, const float* ref, uint32_t M, uint32_t* status, hipStream_t st) {
  const uint32_t n_scan = w.cells_alloc / NN_SCAN_TILE;          // <= 1024
  DNS_LAUNCH(nn_header_kernel, dim3(1), dim3(1), 0, st, w.head, w.target, status);
  DNS_LAUNCH(nn_count_kernel, nn_blocks(M), dim3(NN_BLOCK), 0, st, ref, M, w);
  DNS_LAUNCH(nn_scan_sums_kernel, dim3(n_scan), dim3(NN_BLOCK), 0, st, w);
  DNS_LAUNCH(nn_scan_top_kernel, dim3(1), dim3(NN_SUMS_BLOCK), 0, st, w, n_scan);
  DNS_LAUNCH(nn_scan_local_kernel, dim3(n_scan), dim3(NN_BLOCK), 0, st, w, M);
  DNS_LAUNCH(nn_fill_kernel, nn_blocks(M), dim3(NN_BLOCK), 0, st, ref, M, w);
}

// the all-pairs finish of the todo list (count in status[1]) over w.sorted
void nn_launch_brute(const NnWs& w, uint32_t M, const float* query, uint32_t N, const uint32_t* status, hipStream_t st) {
  const uint32_t chunks = (M + NN_BRUTE_CHUNK - 1) / NN_BRUTE_CHUNK;
  const uint32_t tiles = std::min(NN_BRUTE_GRID_Y, (N + NN_BLOCK - 1) / NN_BLOCK);
  DNS_LAUNCH(nn_brute_kernel, dim3(chunks, tiles), dim3(NN_BLOCK), 0, st, w, M, query, N, status);
}

}  // namespace

extern "C" int dns_nearest_points(const float* ref, uint32_t M, const float* query, uint32_t N, uint32_t max_ring, uint32_t flags,
                                  void* ws, float* dist, int32_t* idx, uint32_t* status, void* stream) {
  DNS_REQUIRE(M < (1u << 31) && N < (1u << 31), "dns_nearest_points: %u reference points, %u queries (must be < 2^31)", M, N);
  DNS_REQUIRE((flags & ~DNS_NEAREST_BRUTE) == 0u, "dns_nearest_points: unknown flags %#x", flags);
  DNS_REQUIRE(max_ring <= 64u, "dns_nearest_points: max_ring %u (must be <= 64)", max_ring);
  if (N == 0) return DNS_OK;
  DNS_REQUIRE(M > 0, "dns_nearest_points: no reference points for %u queries", N);
  DNS_REQUIRE(ref && query && ws && dist && idx && status, "dns_nearest_points: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  NnWs w;
  nn_layout(ws, M, N, &w);
  const bool grid = !(flags & DNS_NEAREST_BRUTE);
  nn_launch_box(w, grid, ref, M, query, N, status, st);
  if (grid) {
    nn_launch_build(w, ref, M, status, st);
    DNS_LAUNCH(nn_query_kernel, nn_blocks(N), dim3(NN_BLOCK), 0, st, w, M, query, N, max_ring, dist, idx, status);
  } else {
    DNS_LAUNCH(nn_pack_kernel, nn_blocks(std::max(M, N)), dim3(NN_BLOCK), 0, st, ref, M, N, w, status);
  }
  nn_launch_brute(w, M, query, N, (const uint32_t*)status, st);
  DNS_LAUNCH(nn_finish_kernel, nn_blocks(N), dim3(NN_BLOCK), 0, st, w, N, dist, idx, (const uint32_t*)status);
  return check_launch("dns_nearest_points");
}

extern "C" uint64_t dns_icp_ws_bytes(uint32_t M, uint32_t N) {
  if (M >= (1u << 31) || N >= (1u << 31) || M == 0 || N == 0) return 0;
  IcpWs w;
  return icp_layout(nullptr, M, N, &w);
}

extern "C" int dns_icp_point_to_point(const float* src, uint32_t N, const float* tgt, uint32_t M, const double* init, float max_dist,
                                      uint32_t max_iter, double rel_fitness, double rel_rmse, uint32_t max_ring, void* ws,
                                      double* result, uint32_t* status, void* stream) {
  DNS_REQUIRE(M > 0 && N > 0, "dns_icp_point_to_point: %u source points, %u target points (an empty cloud)", N, M);
  DNS_REQUIRE(M < (1u << 31) && N < (1u << 31), "dns_icp_point_to_point: %u source points, %u target points (must be < 2^31)", N, M);
  DNS_REQUIRE(max_ring <= 64u, "dns_icp_point_to_point: max_ring %u (must be <= 64)", max_ring);
  DNS_REQUIRE(max_iter <= DNS_ICP_MAX_ITER, "dns_icp_point_to_point: max_iter %u (must be <= %u)", max_iter, DNS_ICP_MAX_ITER);
  DNS_REQUIRE(max_dist > 0.f && max_dist <= 3.0e38f, "dns_icp_point_to_point: max_dist %g (must be positive and finite)",
              (double)max_dist);
  DNS_REQUIRE(rel_fitness >= 0.0 && rel_rmse >= 0.0, "dns_icp_point_to_point: negative (or NaN) relative_fitness / relative_rmse");
  DNS_REQUIRE(src && tgt && ws && result && status, "dns_icp_point_to_point: NULL argument");
  IcpInit t0;
  for (int k = 0; k < 16; ++k) {
    t0.m[k] = init ? init[k] : (k % 5 == 0 ? 1.0 : 0.0);
    DNS_REQUIRE(t0.m[k] - t0.m[k] == 0.0, "dns_icp_point_to_point: init[%d] is not finite", k);
  }
  hipStream_t st = (hipStream_t)stream;
  IcpWs w;
  icp_layout(ws, M, N, &w);
  // at or above every d2 whose fp32 root is <= max_dist (2^-21 covers the rounding of the square and of the root)
  const double md2 = (double)max_dist * (double)max_dist * (1.0 + 0x1p-21);
  const float stop_d2 = md2 < 3.0e38 ? (float)md2 : __builtin_inff();
  const uint32_t rows = std::min(ICP_ROWS, (N + NN_BLOCK - 1) / NN_BLOCK);
  nn_launch_box(w.nn, true, tgt, M, src, N, status, st);
  nn_launch_build(w.nn, tgt, M, status, st);
  DNS_LAUNCH(icp_begin_kernel, dim3(1), dim3(1), 0, st, w.state, t0, status, result);
  for (uint32_t pass = 0; pass <= max_iter; ++pass) {
    DNS_LAUNCH(icp_query_kernel, nn_blocks(N), dim3(NN_BLOCK), 0, st, w.nn, M, src, N, max_ring, stop_d2, w.state, w.xf);
    nn_launch_brute(w.nn, M, w.xf, N, (const uint32_t*)w.state->qst, st);
    DNS_LAUNCH(icp_reduce_kernel, dim3(rows), dim3(NN_BLOCK), 0, st, w.nn, tgt, M, (const float*)w.xf, N, max_dist,
               (const IcpState*)w.state, w.partial);
    DNS_LAUNCH(icp_solve_kernel, dim3(1), dim3(NN_BLOCK), 0, st, (const double*)w.partial, rows, N, pass, max_iter, rel_fitness,
               rel_rmse, w.state, result, status);
  }
  return check_launch("dns_icp_point_to_point");
}

extern "C" int dns_frustum_seen(const float* pts, uint32_t P, const float* w2c, uint32_t K, int H, int W, const float* intr,
                                uint8_t* seen, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(pts && seen && intr, "dns_frustum_seen: NULL argument");
  DNS_REQUIRE(K == 0 || w2c, "dns_frustum_seen: K > 0 needs w2c");
  DNS_REQUIRE(H > 0 && W > 0, "dns_frustum_seen: image %d x %d", H, W);
  hipStream_t st = (hipStream_t)stream;
  DNS_LAUNCH(frustum_seen_kernel, dim3((P + FR_BLOCK - 1) / FR_BLOCK), dim3(FR_BLOCK), 0, st, pts, P, w2c, K, (float)W, (float)H,
             intr[0], intr[1], intr[2], intr[3], seen);
  return check_launch("dns_frustum_seen");
}
