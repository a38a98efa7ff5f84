// Connected components of a triangle mesh by shared edges (the reference's mesh.split(only_watertight=False) of
// slams/meshing.py:721-733, i.e. trimesh's face_adjacency): two faces are adjacent iff they are the only two holders of an
// undirected edge.  Boundary edges (one holder), non-manifold edges (three or more) and shared vertices join nothing.
//
// Four plain launches after an initialising one; no workgroup waits on another:
//   cc_init:    edge table empty, parent[f] = f, comp_area = 0, status = 0.
//   cc_edges:   thread = one of the 3F face edges.  The 64-bit key (min << 32 | max) claims a slot of dev_keytable.hpp's
//               open-addressing table (4F slots for at most 3F keys).  A returning add on the slot's counter orders the
//               holders; the first two leave their face id.
//   cc_union:   thread = slot.  A slot with exactly two holders unions them in a lock-free union-find over parent[F]:
//               find with path halving, the larger root hooked under the smaller one by compare-and-swap.  parent[x] <= x
//               always holds and a non-root never becomes a root again, so a halving store only ever replaces an ancestor
//               by an ancestor, and the root of a finished tree is its smallest face whatever the interleaving.  A failed
//               hook continues from the value the compare-and-swap returned, which is strictly smaller than the node it
//               tried: the loop ends even if every plain load it makes is stale.
//   cc_flatten: thread = face.  Walks to the root (no stores into parent), writes comp, adds the face's float64 area to
//               comp_area[root] and counts the roots.  Adds to one address run at about one per 11 ns, so the faces of one
//               large component must not add one by one: the lanes of a wave that share a root are summed first (up to
//               four distinct roots per wave, the rest add on their own), and the first of those sums of the 16 waves of a
//               workgroup are merged through LDS -- 2.4 M faces of one component make 2400 adds.
//   cc_spread:  comp_area[f] = comp_area[comp[f]] for the non-roots.
// A vertex index outside [0, V) is never dereferenced: it sets status[1] and the face contributes no edge and no area.
// Compiled with -ffp-contract=off (Makefile): the area is the float64 expression tests/mesh_cc_ref.py evaluates.
#include "common.hpp"
#include "dev_keytable.hpp"
#include "dev_reduce.hpp"

namespace dns {

namespace {

constexpr int CC_BLOCK = 256;
constexpr uint32_t CC_BAD_INDEX = 1u;      // status[1] bits
constexpr uint32_t CC_TABLE_FULL = 2u;     // cannot happen with 4F slots; checked rather than assumed
constexpr int CC_FLAT_BLOCK = 1024;        // cc_flatten: 16 waves merge their first sums through LDS
constexpr int CC_FLAT_WAVES = CC_FLAT_BLOCK / WAVE;
constexpr int CC_AGG_ROUNDS = 4;           // distinct roots summed per wave before the rest add on their own

struct CcWs {
  uint64_t* keys;    // [cap] edge key, KEY_EMPTY = free
  uint32_t* count;   // [cap] holders of the key
  int32_t* holder;   // [cap][2] the first two holders
  int32_t* parent;   // [F]
  uint32_t cap;      // 4 F
};

// The parts of F faces' workspace into *w; returns its bytes (ws NULL: the size only).  The last part is not padded.
size_t ws_layout(void* ws, uint32_t F, CcWs* w) {
  WsCarve c(ws);
  w->cap = 4u * F;
  w->keys = c.take<uint64_t>(w->cap);
  w->count = c.take<uint32_t>(w->cap);
  w->holder = c.take<int32_t>(2ull * w->cap);
  w->parent = c.take<int32_t>(F);
  return c.end();
}

__global__ __launch_bounds__(CC_BLOCK) void cc_init_kernel(CcWs ws, uint32_t F, double* __restrict__ comp_area,
                                                           uint32_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (t < ws.cap) {
    ws.keys[t] = KEY_EMPTY;
    ws.count[t] = 0u;
  }
  if (t < F) {
    ws.parent[t] = (int32_t)t;
    comp_area[t] = 0.0;
  }
  if (t < 2) status[t] = 0u;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_edges_kernel(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, CcWs ws,
                                                            uint32_t* __restrict__ status) {
  const uint32_t e = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (e >= 3u * F) return;
  const FaceEdge q = face_edge(faces, e);
  if (!face_in_range(faces, q, V)) {
    if (q.k == 0u) atomicOr(&status[1], CC_BAD_INDEX);
    return;
  }
  const uint32_t s = key_claim(ws.keys, ws.cap, edge_key(q.a, q.b), ws.cap);
  if (s == KEY_NONE) {
    atomicOr(&status[1], CC_TABLE_FULL);
    return;
  }
  const uint32_t n = atomicAdd(&ws.count[s], 1u);
  if (n < 2u) ws.holder[2 * (size_t)s + n] = (int32_t)q.f;
}

__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t x) {
  while (true) {
    const int32_t p = parent[x];
    if (p == x) return x;
    const int32_t g = parent[p];
    if (g == p) return p;
    parent[x] = g;                                               // path halving: an ancestor for an ancestor
    x = g;
  }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_union_kernel(CcWs ws) {
  const uint32_t s = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (s >= ws.cap || ws.count[s] != 2u) return;
  int32_t a = ws.holder[2 * (size_t)s], b = ws.holder[2 * (size_t)s + 1];
  while (true) {
    a = cc_find(ws.parent, a);
    b = cc_find(ws.parent, b);
    if (a == b) return;
    const int32_t hi = max(a, b), lo = min(a, b);
    const int32_t old = atomicCAS(&ws.parent[hi], hi, lo);
    if (old == hi) return;
    a = old, b = lo;                                             // hi was hooked meanwhile: old < hi is its parent
  }
}

__global__ __launch_bounds__(CC_FLAT_BLOCK) void cc_flatten_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                              uint32_t F, uint32_t V, const int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ comp, double* __restrict__ comp_area,
                                                              uint32_t* __restrict__ status) {
  __shared__ int32_t s_root[CC_FLAT_WAVES];
  __shared__ double s_sum[CC_FLAT_WAVES];
  const uint32_t f = blockIdx.x * CC_FLAT_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
  const bool live = f < F;
  int32_t r = -1;
  double area = 0.0;
  if (live) {
    r = (int32_t)f;
    for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;
    comp[f] = r;
    const uint32_t i0 = (uint32_t)faces[3 * (size_t)f], i1 = (uint32_t)faces[3 * (size_t)f + 1], i2 = (uint32_t)faces[3 * (size_t)f + 2];
    if (i0 < V && i1 < V && i2 < V) {
      const float* p0 = verts + 3 * (size_t)i0;
      const float* p1 = verts + 3 * (size_t)i1;
      const float* p2 = verts + 3 * (size_t)i2;
      const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
      const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
      const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
      area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    }
  }
  const uint64_t roots = __ballot(live && r == (int32_t)f);
  if (lane == 0 && roots) atomicAdd(&status[0], (uint32_t)__popcll(roots));
  uint64_t todo = __ballot(live);
  for (int round = 0; round < CC_AGG_ROUNDS; ++round) {
    int32_t r0 = -1;
    double s = 0.0;
    if (todo) {                                                  // wave-uniform
      const int leader = __ffsll((unsigned long long)todo) - 1;
      r0 = __shfl(r, leader);
      const bool mine = live && r == r0;
      s = wave_sum(mine ? area : 0.0);
      todo &= ~__ballot(mine);
    }
    if (round > 0) {
      if (lane == 0 && r0 >= 0) atomicAdd(&comp_area[r0], s);
      continue;
    }
    if (lane == 0) s_root[w] = r0, s_sum[w] = s;                 // round 0: one add per distinct root of the workgroup
    __syncthreads();
    if (threadIdx.x < CC_FLAT_WAVES && s_root[threadIdx.x] >= 0) {
      const int32_t mine_root = s_root[threadIdx.x];
      bool first = true;
      double tot = 0.0;
      for (uint32_t j = 0; j < CC_FLAT_WAVES; ++j)
        if (s_root[j] == mine_root) {
          first = first && j >= threadIdx.x;
          tot += s_sum[j];
        }
      if (first) atomicAdd(&comp_area[mine_root], tot);
    }
  }
  if ((todo >> lane) & 1ull) atomicAdd(&comp_area[r], area);
}

__global__ __launch_bounds__(CC_BLOCK) void cc_spread_kernel(const int32_t* __restrict__ comp, uint32_t F, double* comp_area) {
  const uint32_t f = blockIdx.x * CC_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int32_t r = comp[f];
  if (r != (int32_t)f) comp_area[f] = comp_area[r];              // the roots' entries are only read here
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_mesh_cc_ws_bytes(uint32_t F) {
  if (F == 0 || F >= (1u << 29)) return 0;
  CcWs w;
  return ws_layout(nullptr, F, &w);
}

extern "C" int dns_mesh_components(const float* verts, uint32_t V, const int32_t* faces, uint32_t F, void* ws, int32_t* comp,
                                   double* comp_area, uint32_t* status, void* stream) {
  DNS_REQUIRE(F < (1u << 29), "dns_mesh_components: %u faces (must be < 2^29)", F);
  DNS_REQUIRE(V < (1u << 31), "dns_mesh_components: %u vertices (must be < 2^31)", V);
  if (F == 0) return DNS_OK;
  DNS_REQUIRE(faces && ws && comp && comp_area && status, "dns_mesh_components: NULL argument");
  DNS_REQUIRE(V == 0 || verts, "dns_mesh_components: NULL verts with V > 0");
  hipStream_t st = (hipStream_t)stream;
  CcWs w;
  ws_layout(ws, F, &w);
  const auto blocks = [](uint64_t n) { return dim3((uint32_t)((n + CC_BLOCK - 1) / CC_BLOCK)); };
  DNS_LAUNCH(cc_init_kernel, blocks(w.cap), dim3(CC_BLOCK), 0, st, w, F, comp_area, status);
  DNS_LAUNCH(cc_edges_kernel, blocks(3ull * F), dim3(CC_BLOCK), 0, st, faces, F, V, w, status);
  DNS_LAUNCH(cc_union_kernel, blocks(w.cap), dim3(CC_BLOCK), 0, st, w);
  DNS_LAUNCH(cc_flatten_kernel, dim3((F + CC_FLAT_BLOCK - 1) / CC_FLAT_BLOCK), dim3(CC_FLAT_BLOCK), 0, st, verts, faces, F, V, (const int32_t*)w.parent, comp, comp_area,
             status);
  DNS_LAUNCH(cc_spread_kernel, blocks(F), dim3(CC_BLOCK), 0, st, (const int32_t*)comp, F, comp_area);
  return check_launch("dns_mesh_components");
}
