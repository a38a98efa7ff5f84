// Host check of the hole filling's workspace plan (dns_slam_amd/csrc/mesh_holes_plan.hpp) under the address and
// undefined-behaviour sanitizers.  No GPU is involved and nothing is loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/mesh_holes_plan_check.cpp -o /tmp/mesh_holes_plan_check
//   /tmp/mesh_holes_plan_check
//
// F and V sweep 0, 1, the powers of two and their neighbours up to (and past) the refusal limits 2^29 and 2^31.  For every pair:
//   (a) a size at or past a limit is refused, every other one is planned;
//   (b) the nine parts lie in the order the header states, do not overlap, start on multiples of 256 bytes and end inside
//       `bytes`, which fits 64 bits with room to spare (below 2^40);
//   (c) the per-vertex parts and the carries are where vertex_plan(V) alone puts them, whatever F is: dns_mesh_holes_emit is
//       not told F;
//   (d) the grids cover 3F face edges, 4F slots and V vertices with fewer than 2^31 workgroups of 256, the initialising grid
//       covers slots, vertices and the info words, the carries hold one entry per workgroup of vertices, and the largest
//       face-edge id 3F - 1 and slot 4F - 1 fit 31 bits.
#include <stdio.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../dns_slam_amd/csrc/mesh_holes_plan.hpp"

using namespace dns::holesp;

static long g_fail = 0, g_plans = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++g_fail <= 40) {              \
        printf("FAIL %s: ", #cond);      \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

static std::vector<uint32_t> sizes(uint32_t limit_log2) {
  std::vector<uint32_t> s = {0u, 1u, 3u, 255u, 256u, 257u, 1000003u};
  for (uint32_t k = 1; k <= limit_log2; ++k) {
    const uint64_t p = 1ull << k;
    for (uint64_t x : {p - 1, p, p + 1})
      if (x <= 0xffffffffull) s.push_back((uint32_t)x);
  }
  s.push_back(0xffffffffu);
  return s;
}

static void check(uint32_t F, uint32_t V) {
  Plan p;
  const bool ok = make_plan(F, V, &p);
  CHECK(ok == (F < MAX_FACES && V < MAX_VERTS), "F %u V %u: planned %d", F, V, (int)ok);
  if (!ok) return;
  ++g_plans;
  const uint64_t cap = 4ull * F, nb = ((uint64_t)V + HOLES_BLOCK - 1) / HOLES_BLOCK;
  CHECK(p.F == F && p.V == V && p.cap == cap && p.v_blocks == nb, "F %u V %u: cap %u, v_blocks %u", F, V, p.cap, p.v_blocks);
  const uint64_t off[10] = {p.off_n_out, p.off_n_in, p.off_next, p.off_cnt, p.off_bcount, p.off_bpre,
                            p.off_keys,  p.off_count, p.off_holder, p.bytes};
  const uint64_t need[9] = {4ull * V, 4ull * V, 4ull * V, 4ull * V, 8 * nb, 8 * nb, 8 * cap, 4 * cap, 4 * cap};
  CHECK(off[0] == 0, "F %u V %u: first part at %llu", F, V, (unsigned long long)off[0]);
  for (int i = 0; i < 9; ++i) {
    CHECK(off[i] % 256 == 0, "F %u V %u: part %d at %llu", F, V, i, (unsigned long long)off[i]);
    CHECK(off[i + 1] >= off[i] && off[i + 1] - off[i] >= need[i], "F %u V %u: part %d of %llu bytes in [%llu, %llu)", F, V, i,
          (unsigned long long)need[i], (unsigned long long)off[i], (unsigned long long)off[i + 1]);
    CHECK(off[i + 1] - off[i] < need[i] + 256, "F %u V %u: part %d padded by 256 or more", F, V, i);
  }
  CHECK(p.vertex_bytes == p.off_keys && p.bytes < (1ull << 40), "F %u V %u: %llu bytes", F, V, (unsigned long long)p.bytes);
  Plan q;
  vertex_plan(V, &q);
  CHECK(q.off_n_out == p.off_n_out && q.off_n_in == p.off_n_in && q.off_next == p.off_next && q.off_cnt == p.off_cnt &&
            q.off_bcount == p.off_bcount && q.off_bpre == p.off_bpre && q.vertex_bytes == p.vertex_bytes &&
            q.v_blocks == p.v_blocks && q.grid_verts == p.grid_verts,
        "F %u V %u: the vertex parts depend on F", F, V);
  CHECK((uint64_t)p.grid_edges * HOLES_BLOCK >= 3ull * F && (uint64_t)p.grid_edges * HOLES_BLOCK < 3ull * F + HOLES_BLOCK,
        "F %u: %u workgroups for the face edges", F, p.grid_edges);
  CHECK((uint64_t)p.grid_slots * HOLES_BLOCK >= cap && (uint64_t)p.grid_verts * HOLES_BLOCK >= V, "F %u V %u: grids %u, %u", F, V,
        p.grid_slots, p.grid_verts);
  CHECK(p.grid_init >= p.grid_slots && p.grid_init >= p.grid_verts && (F == 0 || (uint64_t)p.grid_init * HOLES_BLOCK >= INFO_WORDS),
        "F %u V %u: initialising grid %u", F, V, p.grid_init);
  CHECK(p.grid_init < (1u << 31) && p.grid_edges < (1u << 31), "F %u V %u: grid limit", F, V);
  CHECK(F == 0 || (3ull * F - 1 < (1ull << 31) && cap - 1 < (1ull << 31)), "F %u: ids beyond 31 bits", F);
  CHECK(2 * nb <= 2ull * SCAN_THREADS * ((nb + SCAN_THREADS - 1) / SCAN_THREADS), "V %u: the carry scan's runs", V);
}

int main() {
  const std::vector<uint32_t> fs = sizes(29), vs = sizes(31);
  for (uint32_t F : fs)
    for (uint32_t V : vs) check(F, V);
  printf("mesh_holes_plan_check: %ld plans, %ld failed conditions\n", g_plans, g_fail);
  return g_fail ? 1 : 0;
}
