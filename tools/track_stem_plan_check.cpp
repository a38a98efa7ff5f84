// Host check of the fused tracker's stem-form workspace and LDS arithmetic (dns_slam_amd/csrc/track_stem_plan.hpp) under the
// address and undefined-behaviour sanitizers.  No GPU is involved and nothing is loaded into Python: plain loops walk the indices
// csrc/track_fused.inc computes through the same functions, into a buffer of exactly the planned size.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/track_stem_plan_check.cpp -o /tmp/track_stem_plan_check
//   /tmp/track_stem_plan_check
//
// For S = 1..64 samples per ray, R = 1..4 views (and the largest, 8), ray counts with full and partial last workgroups, both
// network shapes' LDS sizes and Cs in {16, 64} it checks:
//   (a) every element of the six row blocks that a workgroup touches -- the first and last element of each row (r, pl) -- lies
//       inside the workgroup's slice and its block, slices neither overlap nor leave the workspace (written through std::vector
//       under ASan, every float owned by at most one workgroup and block) and are 256-byte aligned;
//   (b) the staging passes (PE_ROWS rows at a time) visit every row once and the OneBlob tile fits below keep_off;
//   (c) keep_off covers the network phases, the persistent region and the views' poses follow it, the sum stays within 160 KiB;
//   (d) refused shapes are refused.
// It prints the slice layout for the Replica tracker shape (500 rays x 47 samples, two views) and for the parent's three test
// shapes; the NON-stem rows in front of `base` are laid out by track.hip's track_ws, which this change leaves as it was.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../dns_slam_amd/csrc/track_stem_plan.hpp"

using namespace dns::tfs;

static long g_fail = 0;
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

static uint32_t rays_per_wg(uint32_t S) { return S <= 32u ? 4u : 2u; }      // track.hip

int main() {
  const uint32_t hid = 32, keep_bytes = (4 * 224 + 4 * 64 * 3) * 4;         // TF_KEEP_BYTES (track_fused.hpp)
  const uint32_t mlp_lds[2] = {58112, 125696};                              // of the order of the 32 x 1 and 64 x 2 network phases
  long plans = 0;
  for (uint32_t li = 0; li < 2; ++li)
    for (uint32_t Cs : {16u, 64u})
      for (uint32_t S = 1; S <= 64; ++S)
        for (uint32_t R : {1u, 2u, 3u, 4u, 8u}) {
          const uint32_t rpw = rays_per_wg(S);
          const uint32_t n_pe = Cs == 16u ? 56u : 48u, ld = n_pe + Cs;      // Merge's input: 72 and 112 columns
          for (uint32_t N : {1u, rpw, rpw + 1u, 5u * rpw, 5u * rpw + rpw - 1u, 249u}) {
            const uint64_t base = 64ull * (1000u + S);
            const StemPlan p = stem_plan(N, S, rpw, R, n_pe, Cs, hid, mlp_lds[li], keep_bytes, base);
            CHECK(p.ok, "N %u S %u R %u refused", N, S, R);
            if (!p.ok) continue;
            ++plans;
            CHECK(p.cap == rpw * S && p.cap <= WG_POINTS && p.n_wg == (N + rpw - 1) / rpw, "cap %u, %u workgroups", p.cap, p.n_wg);
            CHECK(p.slice_floats % 64 == 0 && p.base == base && p.total_floats == base + (uint64_t)p.n_wg * p.slice_floats, "slice %u", p.slice_floats);
            for (uint32_t o : {p.rows, p.lat, p.dy, p.dpe, p.xm, p.drel}) CHECK(o % 64 == 0 && o < p.slice_floats, "block offset %u", o);
            // (c)
            CHECK(p.keep_off % 16 == 0 && p.keep_off >= mlp_lds[li] && p.keep_off >= p.tile_bytes && p.tile_bytes == PE_ROWS * (n_pe + 1) * 4,
                  "keep_off %u", p.keep_off);
            CHECK(p.views_off == p.keep_off + keep_bytes && p.lds_bytes == p.views_off + VIEWS_BYTES && p.lds_bytes <= LDS_LIMIT, "LDS %u", p.lds_bytes);
            CHECK(R * VIEW_FLOATS * 4 <= VIEWS_BYTES, "views");
            std::vector<uint8_t> ws(p.total_floats, 0);                     // one byte per float: its owner (workgroup, block)
            const uint32_t width[6] = {ld, hid, hid, n_pe, 3, 3};
            const uint32_t off[6] = {p.rows, p.lat, p.dy, p.dpe, p.xm, p.drel};
            for (uint32_t wg = 0; wg < p.n_wg; ++wg) {
              const uint32_t n0 = wg * rpw, n1 = n0 + rpw < N ? n0 + rpw : N, npts = (n1 - n0) * S, nrows = R * npts;
              CHECK(npts >= 1 && npts <= p.cap, "workgroup %u holds %u points", wg, npts);
              const uint64_t s0 = base + (uint64_t)wg * p.slice_floats;
              // (b)
              uint32_t staged = 0;
              for (uint32_t i0 = 0; i0 < nrows; i0 += PE_ROWS) staged += nrows - i0 < PE_ROWS ? nrows - i0 : PE_ROWS;
              CHECK(staged == nrows, "staging visits %u of %u rows", staged, nrows);
              // (a)
              for (uint32_t b = 0; b < 6; ++b) {
                const uint8_t tag = (uint8_t)(1 + (wg * 6 + b) % 250);
                const uint64_t b0 = s0 + off[b], b1 = b + 1 < 6 ? s0 + off[b + 1] : s0 + p.slice_floats;
                for (uint32_t r = 0; r < R; ++r)
                  for (uint32_t pl = 0; pl < npts; pl += (npts > 1 ? npts - 1 : 1)) {
                    const uint32_t row = pair_row(r, pl, npts);
                    CHECK(row < nrows, "row %u of %u", row, nrows);
                    const uint64_t e0 = b0 + (uint64_t)row * width[b], e1 = e0 + width[b] - 1;
                    CHECK(e1 < b1, "row %u of block %u leaves it", row, b);
                    CHECK(ws.at(e0) == 0 || ws.at(e0) == tag, "overlap at %llu", (unsigned long long)e0);
                    CHECK(ws.at(e1) == 0 || ws.at(e1) == tag, "overlap at %llu", (unsigned long long)e1);
                    ws.at(e0) = tag;
                    ws.at(e1) = tag;
                  }
              }
            }
            for (uint64_t i = 0; i < base; ++i) CHECK(ws[i] == 0, "a stem row in front of base");
          }
        }
  // (d)
  CHECK(!stem_plan(0, 47, 2, 2, 48, 64, 32, 125696, keep_bytes, 0).ok, "no rays");
  CHECK(!stem_plan(100, 65, 2, 2, 48, 64, 32, 125696, keep_bytes, 0).ok && !stem_plan(100, 33, 4, 2, 48, 64, 32, 125696, keep_bytes, 0).ok, "more than 128 points");
  CHECK(!stem_plan(100, 47, 2, 0, 48, 64, 32, 125696, keep_bytes, 0).ok && !stem_plan(100, 47, 2, 9, 48, 64, 32, 125696, keep_bytes, 0).ok, "view count");
  CHECK(!stem_plan(100, 47, 2, 2, 48, 6, 32, 125696, keep_bytes, 0).ok && !stem_plan(100, 47, 2, 2, 46, 64, 32, 125696, keep_bytes, 0).ok, "columns");
  CHECK(!stem_plan(100, 47, 2, 2, 96, 64, 32, 125696, keep_bytes, 0).ok, "more than 128 columns");
  CHECK(!stem_plan(100, 47, 2, 2, 48, 64, 30, 125696, keep_bytes, 0).ok, "outputs");
  CHECK(!stem_plan(100, 47, 2, 2, 48, 64, 32, 125697, keep_bytes, 0).ok && !stem_plan(100, 47, 2, 2, 48, 64, 32, 160 * 1024, keep_bytes, 0).ok, "LDS");
  CHECK(!stem_plan(100, 47, 2, 2, 48, 64, 32, 125696, keep_bytes, 32).ok, "unaligned base");
  // the layouts a reader compares
  const struct { uint32_t N, S, R; const char* what; } shown[] = {{500, 47, 2, "Replica tracker"}, {249, 47, 2, "test case 1"}, {249, 32, 3, "test case 2"}, {249, 64, 1, "test case 3"}};
  for (const auto& s : shown) {
    const StemPlan p = stem_plan(s.N, s.S, rays_per_wg(s.S), s.R, 48, 64, 32, 125696, keep_bytes, 0);
    printf("%-16s N %3u S %2u R %u: %3u workgroups x %6u floats (rows %u lat %u dy %u dpe %u xm %u drel %u) = %.1f MB; keep_off %u, LDS %u\n", s.what, s.N, s.S,
           s.R, p.n_wg, p.slice_floats, p.rows, p.lat, p.dy, p.dpe, p.xm, p.drel, (double)p.n_wg * p.slice_floats * 4 / 1e6, p.keep_off, p.lds_bytes);
  }
  printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}
