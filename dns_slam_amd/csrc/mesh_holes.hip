// Hole filling of a triangle mesh (the reference's mesh.fill_holes() of slams/meshing.py:770, i.e. trimesh.repair.fill_holes): the
// boundary loops of three and four edges -- up to max_edges here -- are closed with new faces wound against the faces across their
// boundary edges; no vertex is added.  The definition, and where it differs from trimesh, is in include/dns_hip.h.
//
// Plain launches, kernel boundaries the only ordering; no workgroup waits on another:
//   holes_init:     edge table empty, the per-vertex words and info zero.
//   holes_edges:    thread = one of the 3F face edges.  The 64-bit key (min << 32 | max) claims a slot of dev_keytable.hpp's
//                   open-addressing table (4F slots for at most 3F keys).  A returning add on the slot's counter counts the
//                   holders; the first leaves its face-edge id 3f + e, which is only read where the count is 1 -- there it is the
//                   only one, so nothing depends on scheduling.
//   holes_boundary: thread = slot.  Count 1: the directed boundary half-edge a -> b as its face winds it: n_out[a]++, n_in[b]++,
//                   next[a] = b (a plain store: where n_out[a] > 1 the value is arbitrary and never read).
//   holes_count:    thread = vertex v.  A vertex is simple iff n_out == 1 and n_in == 1.  The thread walks v -> next[v] -> ... for
//                   at most max_edges steps through simple vertices above v; back at v after L steps it is the smallest vertex of a
//                   simple loop and owns it: cnt[v] = L - 2.  Per workgroup the (faces, loops) sums.
//   holes_scan:     one workgroup: exclusive prefix of the workgroup sums and the two totals (into info): marching cubes' carry scan.
//   holes_emit:     the owner repeats its walk v0 -> v1 -> ... and writes the fan (v0, v_{i+1}, v_i), i = 1 .. L - 2, at its scanned
//                   offset.
// Every index read from `faces` is compared with V before it is used as an index; next[] holds only such indices; a walk reads
// next[u] only where n_out[u] == 1, i.e. where exactly one store wrote it.  Every offset holes_emit stores at is below the total
// the caller sized new_faces by (the sum of the cnt it rescans).  No floating point in here.
#include "common.hpp"
#include "dev_keytable.hpp"
#include "dev_reduce.hpp"
#include "mesh_holes_plan.hpp"

namespace dns {

namespace {

using namespace holesp;

static_assert(INFO_WORDS == DNS_HOLES_INFO_WORDS, "info layout of dns_hip.h");

struct HolesWs {
  uint32_t *n_out, *n_in, *next, *cnt;   // [V]
  uint32_t *bcount, *bpre;               // [v_blocks][2] (faces, loops)
  uint64_t* keys;                        // [cap] edge key, KEY_EMPTY = free
  uint32_t* count;                       // [cap] holders of the key
  uint32_t* holder;                      // [cap] face-edge id 3 f + e of the first holder
  uint32_t cap;
};

HolesWs ws_vertex_parts(void* ws, const Plan& p) {
  char* b = (char*)ws;
  HolesWs w{};
  w.n_out = (uint32_t*)(b + p.off_n_out), w.n_in = (uint32_t*)(b + p.off_n_in);
  w.next = (uint32_t*)(b + p.off_next), w.cnt = (uint32_t*)(b + p.off_cnt);
  w.bcount = (uint32_t*)(b + p.off_bcount), w.bpre = (uint32_t*)(b + p.off_bpre);
  return w;
}

HolesWs ws_layout(void* ws, const Plan& p) {
  char* b = (char*)ws;
  HolesWs w = ws_vertex_parts(ws, p);
  w.keys = (uint64_t*)(b + p.off_keys);
  w.count = (uint32_t*)(b + p.off_count);
  w.holder = (uint32_t*)(b + p.off_holder);
  w.cap = p.cap;
  return w;
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_init_kernel(HolesWs ws, uint32_t V, uint32_t* __restrict__ info) {
  const uint32_t t = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  if (t < ws.cap) {
    ws.keys[t] = KEY_EMPTY;
    ws.count[t] = 0u;
  }
  if (t < V) ws.n_out[t] = 0u, ws.n_in[t] = 0u, ws.next[t] = 0u;
  if (t < INFO_WORDS) info[t] = 0u;
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_edges_kernel(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, HolesWs ws,
                                                                  uint32_t* __restrict__ info) {
  const uint32_t e = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  if (e >= 3u * F) return;
  const FaceEdge q = face_edge(faces, e);
  if (!face_in_range(faces, q, V)) {
    if (q.k == 0u) atomicOr(&info[DNS_HOLES_INFO_BAD_INDEX], 1u);
    return;
  }
  if (q.a == q.b) {
    atomicAdd(&info[DNS_HOLES_INFO_DEGENERATE], 1u);
    return;
  }
  const uint32_t s = key_claim(ws.keys, ws.cap, edge_key(q.a, q.b), ws.cap);
  if (s == KEY_NONE) {                                           // cannot happen with 4F slots; checked rather than assumed
    atomicOr(&info[DNS_HOLES_INFO_TABLE_FULL], 1u);
    return;
  }
  if (atomicAdd(&ws.count[s], 1u) == 0u) ws.holder[s] = e;
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_boundary_kernel(const int32_t* __restrict__ faces, HolesWs ws,
                                                                     uint32_t* __restrict__ info) {
  const uint32_t s = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  if (s >= ws.cap) return;
  const uint32_t n = ws.count[s];
  if (n == 1u) {
    const FaceEdge q = face_edge(faces, ws.holder[s]);           // 3 f + k of a face holes_edges found in range
    atomicAdd(&ws.n_out[q.a], 1u);
    atomicAdd(&ws.n_in[q.b], 1u);
    ws.next[q.a] = q.b;
    atomicAdd(&info[DNS_HOLES_INFO_BOUNDARY_EDGES], 1u);
  } else if (n >= 3u) {
    atomicAdd(&info[DNS_HOLES_INFO_NONMANIFOLD_EDGES], 1u);
  }
}

__device__ __forceinline__ bool holes_simple(const HolesWs& ws, uint32_t v) { return ws.n_out[v] == 1u && ws.n_in[v] == 1u; }

// The length of the simple loop v owns (v its smallest vertex, 3 .. max_edges edges), or 0.
__device__ __forceinline__ uint32_t holes_loop(const HolesWs& ws, uint32_t v, uint32_t max_edges) {
  if (!holes_simple(ws, v)) return 0u;
  uint32_t u = ws.next[v];
  for (uint32_t steps = 1u; steps <= max_edges; ++steps) {
    if (u == v) return steps >= 3u ? steps : 0u;
    if (u < v || !holes_simple(ws, u)) return 0u;
    u = ws.next[u];
  }
  return 0u;
}

using HolesCounts = Counts2<uint32_t>;   // a = faces, b = loops

__global__ __launch_bounds__(HOLES_BLOCK) void holes_count_kernel(HolesWs ws, uint32_t V, uint32_t max_edges, uint32_t* __restrict__ info) {
  __shared__ HolesCounts s[HOLES_BLOCK];
  const uint32_t v = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  HolesCounts own{0u, 0u};
  bool skipped = false;
  if (v < V) {
    const uint32_t L = holes_loop(ws, v, max_edges);
    own.a = L ? L - 2u : 0u, own.b = L ? 1u : 0u;
    ws.cnt[v] = own.a;
    skipped = ws.n_out[v] + ws.n_in[v] > 0u && !holes_simple(ws, v);
  }
  const uint64_t sk = __ballot(skipped);
  if (threadIdx.x % WAVE == 0 && sk) atomicAdd(&info[DNS_HOLES_INFO_VERTICES_SKIPPED], (uint32_t)__popcll(sk));
  const HolesCounts incl = block_scan_inclusive<HOLES_BLOCK>(s, own);
  if (threadIdx.x == HOLES_BLOCK - 1) ws.bcount[2 * blockIdx.x] = incl.a, ws.bcount[2 * blockIdx.x + 1] = incl.b;
}

// One workgroup: dev_reduce.hpp's carry scan of the workgroup sums; the two totals go into info.
__global__ __launch_bounds__(SCAN_THREADS) void holes_scan_kernel(HolesWs ws, uint32_t n_blocks, uint32_t* __restrict__ info) {
  __shared__ HolesCounts s[SCAN_THREADS];
  const HolesCounts tot = carry_scan(s, ws.bcount, ws.bpre, n_blocks);
  if (threadIdx.x == SCAN_THREADS - 1) info[DNS_HOLES_INFO_FACES_ADDED] = tot.a, info[DNS_HOLES_INFO_LOOPS_FILLED] = tot.b;
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_emit_kernel(HolesWs ws, uint32_t V, uint32_t max_edges, int32_t* __restrict__ new_faces) {
  __shared__ uint32_t s[HOLES_BLOCK];
  const uint32_t v = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  const uint32_t own = v < V ? ws.cnt[v] : 0u;
  const uint32_t incl = block_scan_inclusive<HOLES_BLOCK>(s, own);
  if (own == 0u || own + 2u > max_edges) return;                 // the second cannot happen with holes_count's max_edges
  size_t at = (size_t)ws.bpre[2 * blockIdx.x] + incl - own;
  uint32_t prev = ws.next[v];                                    // v1
  for (uint32_t i = 0; i < own; ++i, ++at) {
    const uint32_t cur = ws.next[prev];                          // v_{i+2}
    new_faces[3 * at] = (int32_t)v, new_faces[3 * at + 1] = (int32_t)cur, new_faces[3 * at + 2] = (int32_t)prev;
    prev = cur;
  }
}

}  // namespace

}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_mesh_holes_ws_bytes(uint32_t F, uint32_t V) {
  Plan p;
  if (F == 0 || !make_plan(F, V, &p)) return 0;
  return p.bytes;
}

extern "C" int dns_mesh_holes_count(const int32_t* faces, uint32_t F, uint32_t V, uint32_t max_edges, void* ws, uint32_t* info,
                                    void* stream) {
  DNS_REQUIRE(F < MAX_FACES, "dns_mesh_holes_count: %u faces (must be < 2^29)", F);
  DNS_REQUIRE(V < MAX_VERTS, "dns_mesh_holes_count: %u vertices (must be < 2^31)", V);
  DNS_REQUIRE(max_edges >= MIN_EDGES && max_edges <= MAX_EDGES, "dns_mesh_holes_count: max_edges %u (must be 3 .. 32)", max_edges);
  DNS_REQUIRE(info, "dns_mesh_holes_count: NULL info");
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) return fill_words(info, 0u, INFO_WORDS, st, "dns_mesh_holes_count");
  DNS_REQUIRE(faces && ws, "dns_mesh_holes_count: NULL argument");
  Plan p;
  make_plan(F, V, &p);
  const HolesWs w = ws_layout(ws, p);
  DNS_LAUNCH(holes_init_kernel, dim3(p.grid_init), dim3(HOLES_BLOCK), 0, st, w, V, info);
  DNS_LAUNCH(holes_edges_kernel, dim3(p.grid_edges), dim3(HOLES_BLOCK), 0, st, faces, F, V, w, info);
  DNS_LAUNCH(holes_boundary_kernel, dim3(p.grid_slots), dim3(HOLES_BLOCK), 0, st, faces, w, info);
  if (p.grid_verts) DNS_LAUNCH(holes_count_kernel, dim3(p.grid_verts), dim3(HOLES_BLOCK), 0, st, w, V, max_edges, info);
  DNS_LAUNCH(holes_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, w, p.v_blocks, info);
  return check_launch("dns_mesh_holes_count");
}

extern "C" int dns_mesh_holes_emit(const void* ws, uint32_t V, uint32_t max_edges, int32_t* new_faces, void* stream) {
  DNS_REQUIRE(V < MAX_VERTS, "dns_mesh_holes_emit: %u vertices (must be < 2^31)", V);
  DNS_REQUIRE(max_edges >= MIN_EDGES && max_edges <= MAX_EDGES, "dns_mesh_holes_emit: max_edges %u (must be 3 .. 32)", max_edges);
  if (V == 0) return DNS_OK;
  DNS_REQUIRE(ws && new_faces, "dns_mesh_holes_emit: NULL argument");
  Plan p;
  vertex_plan(V, &p);
  const HolesWs w = ws_vertex_parts((void*)ws, p);
  DNS_LAUNCH(holes_emit_kernel, dim3(p.grid_verts), dim3(HOLES_BLOCK), 0, (hipStream_t)stream, w, V, max_edges, new_faces);
  return check_launch("dns_mesh_holes_emit");
}
