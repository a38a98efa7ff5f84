// Workspace layout and grid sizes of the mesh hole filling (mesh_holes.hip), free of HIP headers: tools/mesh_holes_plan_check.cpp
// walks it on the host under ASan + UBSan.
//
// The parts, in this order, each padded to a multiple of 256 bytes (ws_carve.hpp's align256):
//   n_out, n_in, next, cnt   [V] uint32 each: the per-vertex words
//   bcount, bpre             [v_blocks][2] uint32 each: (faces, loops) of a workgroup of HOLES_BLOCK vertices and their exclusive
//                            prefixes -- the scan's carries
//   keys [cap] uint64, count [cap] uint32, holder [cap] uint32: the edge table, cap = 4 F slots for at most 3 F keys
// The per-vertex parts and the carries come first, so that their offsets depend on V alone: dns_mesh_holes_emit is not told F.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ws_carve.hpp"

namespace dns {
namespace holesp {

constexpr uint32_t HOLES_BLOCK = 256;              // threads per workgroup of every kernel but the carry scan
using dns::SCAN_THREADS;                           // ws_carve.hpp: the one workgroup that scans the carries
constexpr uint32_t MAX_FACES = 1u << 29;           // refused from here on: 4 F slots and 3 F + 2 face-edge ids stay below 2^31
constexpr uint32_t MAX_VERTS = 1u << 31;           // vertex indices are non-negative int32
constexpr uint32_t MIN_EDGES = 3, MAX_EDGES = 32;  // bounds of max_edges
constexpr uint32_t INFO_WORDS = 8;                 // dns_hip.h: DNS_HOLES_INFO_*

struct Plan {
  uint32_t F, V;
  uint32_t cap;                                    // slots of the edge table
  uint32_t v_blocks;                               // workgroups over the vertices = entries of the carries
  uint64_t off_n_out, off_n_in, off_next, off_cnt, off_bcount, off_bpre, off_keys, off_count, off_holder;
  uint64_t vertex_bytes;                           // the parts whose layout depends on V alone: everything before off_keys
  uint64_t bytes;                                  // the whole workspace
  uint32_t grid_init, grid_edges, grid_slots, grid_verts;
};

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + HOLES_BLOCK - 1) / HOLES_BLOCK); }

// The per-vertex parts and the carries of V vertices (F plays no part).
inline void vertex_plan(uint32_t V, Plan* p) {
  p->V = V;
  p->v_blocks = blocks_for(V);
  uint64_t o = 0;
  const uint64_t words = (uint64_t)align256((size_t)V * sizeof(uint32_t));
  p->off_n_out = o, o += words;
  p->off_n_in = o, o += words;
  p->off_next = o, o += words;
  p->off_cnt = o, o += words;
  const uint64_t carries = (uint64_t)align256((size_t)p->v_blocks * 2 * sizeof(uint32_t));
  p->off_bcount = o, o += carries;
  p->off_bpre = o, o += carries;
  p->vertex_bytes = o;
  p->grid_verts = p->v_blocks;
}

// false: a refused size (F >= 2^29, V >= 2^31).  F = 0 gives a plan of the vertex parts alone, which nobody launches on.
inline bool make_plan(uint32_t F, uint32_t V, Plan* p) {
  if (F >= MAX_FACES || V >= MAX_VERTS) return false;
  vertex_plan(V, p);
  p->F = F;
  p->cap = 4u * F;
  uint64_t o = p->vertex_bytes;
  p->off_keys = o, o += (uint64_t)align256((size_t)p->cap * sizeof(uint64_t));
  p->off_count = o, o += (uint64_t)align256((size_t)p->cap * sizeof(uint32_t));
  p->off_holder = o, o += (uint64_t)align256((size_t)p->cap * sizeof(uint32_t));
  p->bytes = o;
  p->grid_edges = blocks_for(3ull * F);
  p->grid_slots = blocks_for(p->cap);
  p->grid_init = p->grid_slots > p->grid_verts ? p->grid_slots : p->grid_verts;
  return true;
}

}  // namespace holesp
}  // namespace dns
