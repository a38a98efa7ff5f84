// Hole filling of a triangle mesh (the reference's mesh.fill_holes() of slams/meshing.py:770, i.e. trimesh.repair.fill_holes): the
// boundary loops of three and four edges -- up to max_edges here -- are closed with new faces wound against the faces across their
// boundary edges; no vertex is added.  The definition, and where it differs from trimesh, is in include/dns_hip.h.
//
// Plain launches, kernel boundaries the only ordering; no workgroup waits on another:
//   holes_init:     edge table empty, the per-vertex words and info zero.
//   holes_edges:    thread = one of the 3F face edges.  The 64-bit key (min << 32 | max) claims a slot of an open-addressing table
//                   (linear probing that wraps, 4F slots for at most 3F keys) with a 64-bit compare-and-swap against the all-ones
//                   word, which no key equals (indices are below 2^31).  A returning add on the slot's counter counts the
//                   holders; the first leaves its face-edge id 3f + e, which is only read where the count is 1 -- there it is the
//                   only one, so nothing depends on scheduling.
//   holes_boundary: thread = slot.  Count 1: the directed boundary half-edge a -> b as its face winds it: n_out[a]++, n_in[b]++,
//                   next[a] = b (a plain store: where n_out[a] > 1 the value is arbitrary and never read).
//   holes_count:    thread = vertex v.  A vertex is simple iff n_out == 1 and n_in == 1.  The thread walks v -> next[v] -> ... for
//                   at most max_edges steps through simple vertices above v; back at v after L steps it is the smallest vertex of a
//                   simple loop and owns it: cnt[v] = L - 2.  Per workgroup the (faces, loops) sums.
//   holes_scan:     one workgroup: exclusive prefix of the workgroup sums and the two totals (into info).
//   holes_emit:     the owner repeats its walk v0 -> v1 -> ... and writes the fan (v0, v_{i+1}, v_i), i = 1 .. L - 2, at its scanned
//                   offset.
// Every index read from `faces` is compared with V before it is used as an index; next[] holds only such indices; a walk reads
// next[u] only where n_out[u] == 1, i.e. where exactly one store wrote it.  Every offset holes_emit stores at is below the total
// the caller sized new_faces by (the sum of the cnt it rescans).  No floating point in here.
#include "common.hpp"
#include "dev_reduce.hpp"
#include "mesh_holes_plan.hpp"

namespace dns {

namespace {

using namespace holesp;

constexpr uint64_t HOLES_EMPTY = ~0ull;
static_assert(INFO_WORDS == DNS_HOLES_INFO_WORDS, "info layout of dns_hip.h");

struct HolesWs {
  uint32_t *n_out, *n_in, *next, *cnt;   // [V]
  uint32_t *bcount, *bpre;               // [v_blocks][2] (faces, loops)
  uint64_t* keys;                        // [cap] edge key, HOLES_EMPTY = free
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
    ws.keys[t] = HOLES_EMPTY;
    ws.count[t] = 0u;
  }
  if (t < V) ws.n_out[t] = 0u, ws.n_in[t] = 0u, ws.next[t] = 0u;
  if (t < INFO_WORDS) info[t] = 0u;
}

__device__ __forceinline__ uint32_t holes_slot(uint64_t key, uint32_t cap) {
  uint64_t h = key;                                              // murmur3's 64-bit finaliser
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return (uint32_t)(((h >> 32) * cap) >> 32);                    // [0, cap)
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_edges_kernel(const int32_t* __restrict__ faces, uint32_t F, uint32_t V, HolesWs ws,
                                                                  uint32_t* __restrict__ info) {
  const uint32_t e = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  if (e >= 3u * F) return;
  const uint32_t f = e / 3u, k = e - 3u * f;
  const uint32_t a = (uint32_t)faces[3 * (size_t)f + k], b = (uint32_t)faces[3 * (size_t)f + (k == 2u ? 0u : k + 1u)];
  const uint32_t c = (uint32_t)faces[3 * (size_t)f + (k == 0u ? 2u : k - 1u)];
  if (a >= V || b >= V || c >= V) {                              // negative indices are >= 2^31 here: the whole face is out
    if (k == 0u) atomicOr(&info[DNS_HOLES_INFO_BAD_INDEX], 1u);
    return;
  }
  if (a == b) {
    atomicAdd(&info[DNS_HOLES_INFO_DEGENERATE], 1u);
    return;
  }
  const uint64_t key = ((uint64_t)min(a, b) << 32) | (uint64_t)max(a, b);
  uint32_t s = holes_slot(key, ws.cap);
  for (uint32_t probe = 0; probe < ws.cap; ++probe) {
    uint64_t cur = __hip_atomic_load(&ws.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == HOLES_EMPTY) cur = atomicCAS((unsigned long long*)&ws.keys[s], (unsigned long long)HOLES_EMPTY, (unsigned long long)key);
    if (cur == HOLES_EMPTY || cur == key) {
      if (atomicAdd(&ws.count[s], 1u) == 0u) ws.holder[s] = e;
      return;
    }
    s = s + 1u == ws.cap ? 0u : s + 1u;
  }
  atomicOr(&info[DNS_HOLES_INFO_TABLE_FULL], 1u);                // cannot happen with 4F slots; checked rather than assumed
}

__global__ __launch_bounds__(HOLES_BLOCK) void holes_boundary_kernel(const int32_t* __restrict__ faces, HolesWs ws,
                                                                     uint32_t* __restrict__ info) {
  const uint32_t s = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  if (s >= ws.cap) return;
  const uint32_t n = ws.count[s];
  if (n == 1u) {
    const uint32_t e = ws.holder[s];                             // 3 f + k of a face holes_edges found in range
    const uint32_t f = e / 3u, k = e - 3u * f;
    const uint32_t a = (uint32_t)faces[3 * (size_t)f + k], b = (uint32_t)faces[3 * (size_t)f + (k == 2u ? 0u : k + 1u)];
    atomicAdd(&ws.n_out[a], 1u);
    atomicAdd(&ws.n_in[b], 1u);
    ws.next[a] = b;
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

struct HolesCounts {
  uint32_t f, l;     // faces, loops
  __device__ HolesCounts& operator+=(const HolesCounts& o) { return f += o.f, l += o.l, *this; }
};

__global__ __launch_bounds__(HOLES_BLOCK) void holes_count_kernel(HolesWs ws, uint32_t V, uint32_t max_edges, uint32_t* __restrict__ info) {
  __shared__ HolesCounts s[HOLES_BLOCK];
  const uint32_t v = blockIdx.x * HOLES_BLOCK + threadIdx.x;
  HolesCounts own{0u, 0u};
  bool skipped = false;
  if (v < V) {
    const uint32_t L = holes_loop(ws, v, max_edges);
    own.f = L ? L - 2u : 0u, own.l = L ? 1u : 0u;
    ws.cnt[v] = own.f;
    skipped = ws.n_out[v] + ws.n_in[v] > 0u && !holes_simple(ws, v);
  }
  const uint64_t sk = __ballot(skipped);
  if (threadIdx.x % WAVE == 0 && sk) atomicAdd(&info[DNS_HOLES_INFO_VERTICES_SKIPPED], (uint32_t)__popcll(sk));
  const HolesCounts incl = block_scan_inclusive<HOLES_BLOCK>(s, own);
  if (threadIdx.x == HOLES_BLOCK - 1) ws.bcount[2 * blockIdx.x] = incl.f, ws.bcount[2 * blockIdx.x + 1] = incl.l;
}

// One workgroup of 1024: thread t sums a contiguous run of workgroup sums, an LDS scan of the 1024 run sums, then the run's prefixes.
__global__ __launch_bounds__(SCAN_THREADS) void holes_scan_kernel(HolesWs ws, uint32_t n_blocks, uint32_t* __restrict__ info) {
  __shared__ HolesCounts s[SCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n_blocks + SCAN_THREADS - 1) / SCAN_THREADS;
  const uint32_t b0 = (uint32_t)min((uint64_t)t * per, (uint64_t)n_blocks), b1 = min(b0 + per, n_blocks);
  HolesCounts own{0u, 0u};
  for (uint32_t b = b0; b < b1; ++b) own.f += ws.bcount[2 * b], own.l += ws.bcount[2 * b + 1];
  const HolesCounts incl = block_scan_inclusive<SCAN_THREADS>(s, own);
  uint32_t pf = incl.f - own.f, pl = incl.l - own.l;
  for (uint32_t b = b0; b < b1; ++b) {
    ws.bpre[2 * b] = pf, ws.bpre[2 * b + 1] = pl;
    pf += ws.bcount[2 * b], pl += ws.bcount[2 * b + 1];
  }
  if (t == SCAN_THREADS - 1) info[DNS_HOLES_INFO_FACES_ADDED] = incl.f, info[DNS_HOLES_INFO_LOOPS_FILLED] = incl.l;
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
