// The open-addressing table of 64-bit keys that mesh_cc (cc_edges), mesh_holes (holes_edges) and tsdf (tsdf_touch) build: linear
// probing that wraps, a slot claimed by a 64-bit compare-and-swap against the all-ones word, which no key equals (vertex indices
// are below 2^31, the frame in a TSDF key's low 16 bits is below 65535).  What a unit keeps beside a key -- holder counts, face
// ids, nothing -- stays in the unit.  Also the face-edge id e = 3 f + k of the two edge tables.
#pragma once
#include "common.hpp"
namespace dns {

constexpr uint64_t KEY_EMPTY = ~0ull;                            // a free slot
constexpr uint32_t KEY_NONE = ~0u;                               // key_claim: the probes ran out

__device__ __forceinline__ uint32_t key_slot(uint64_t key, uint32_t cap) {
  uint64_t h = key;                                              // murmur3's 64-bit finaliser
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return (uint32_t)(((h >> 32) * cap) >> 32);                    // [0, cap)
}

// The slot of keys [cap] that holds `key` after the call -- it was free and is now claimed, or it held the key already -- or
// KEY_NONE when `limit` (<= cap) probes met other keys only.  Several threads may claim the same key at once: all get its slot.
__device__ __forceinline__ uint32_t key_claim(uint64_t* keys, uint32_t cap, uint64_t key, uint32_t limit) {
  uint32_t s = key_slot(key, cap);
  for (uint32_t probe = 0; probe < limit; ++probe) {
    uint64_t cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == KEY_EMPTY) cur = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
    if (cur == KEY_EMPTY || cur == key) return s;
    s = s + 1u == cap ? 0u : s + 1u;
  }
  return KEY_NONE;
}

// The undirected edge of two vertex indices below 2^31: never KEY_EMPTY.
__device__ __forceinline__ uint64_t edge_key(uint32_t a, uint32_t b) { return ((uint64_t)min(a, b) << 32) | (uint64_t)max(a, b); }

// Face edge e = 3 f + k: the directed edge a -> b = faces[f][k] -> faces[f][(k + 1) % 3], as the face winds it.
struct FaceEdge {
  uint32_t f, k, a, b;
};
__device__ __forceinline__ FaceEdge face_edge(const int32_t* __restrict__ faces, uint32_t e) {
  FaceEdge q;
  q.f = e / 3u, q.k = e - 3u * q.f;
  q.a = (uint32_t)faces[3 * (size_t)q.f + q.k], q.b = (uint32_t)faces[3 * (size_t)q.f + (q.k == 2u ? 0u : q.k + 1u)];
  return q;
}
// false: one of the three indices of q's face is outside [0, V) -- negative ones are >= 2^31 here -- and the whole face is out.
__device__ __forceinline__ bool face_in_range(const int32_t* __restrict__ faces, const FaceEdge& q, uint32_t V) {
  const uint32_t c = (uint32_t)faces[3 * (size_t)q.f + (q.k == 0u ? 2u : q.k - 1u)];
  return q.a < V && q.b < V && c < V;
}

}  // namespace dns
