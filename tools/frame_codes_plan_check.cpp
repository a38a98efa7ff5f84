// Host check of dns_frame_codes' tiling and workspace arithmetic (dns_slam_amd/csrc/frame_codes_plan.hpp) under the address and
// undefined-behaviour sanitizers.  No GPU is involved and nothing is loaded into Python: plain loops walk the indices
// csrc/frame_codes.hip computes through the same functions, into buffers of exactly the planned sizes.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/frame_codes_plan_check.cpp -o /tmp/frame_codes_plan_check
//   /tmp/frame_codes_plan_check
//
// For point counts around the tile and grid boundaries, 1..64 views, the two network shapes' LDS sizes and every tile size it checks:
//   (a) the tiles a workgroup walks (b, b + blocks, ...) cover every point exactly once;
//   (b) every row and latent slot a tile writes lies inside the workgroup's slice, slices do not overlap and are 16-byte aligned,
//       and the workspace holds them all (written through std::vector under ASan);
//   (c) the OneBlob tile lies behind the MLP area and the whole fits 160 KiB; the staging pass (PE_ROWS pairs at a time) visits
//       every pair once;
//   (d) refused shapes are refused.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../dns_slam_amd/csrc/frame_codes_plan.hpp"

using namespace dns::fc;

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

int main() {
  const uint32_t n_pe = 48, C = 64, hid = 32, ld = n_pe + C;
  const uint32_t mlp_lds[2] = {38400, 73728};                       // of the order of the 32 x 1 and 64 x 2 forward areas
  long plans = 0;
  const uint64_t sizes[] = {1, 37, 127, 128, 129, 677, 128 * 255, 128 * 256, 128 * 256 + 1, 128 * 512 + 5, 47000, 128 * 1300 + 77, 64 * 4 * 512, 128 * 4 * 512 + 3};
  for (uint32_t li = 0; li < 2; ++li)
    for (uint64_t P : sizes)
      for (uint32_t R : {1u, 2u, 3u, 7u, 64u})
      for (uint32_t tile : {0u, 32u, 64u, 128u}) {
        const Plan p = plan(P, R, n_pe, C, hid, mlp_lds[li], tile);
        const uint32_t TP = p.tile_pts;
        CHECK(TP == 32 || TP == 64 || TP == 128, "tile of %u points", TP);
        CHECK(tile == 0 || TP == tile, "tile %u asked, %u planned", tile, TP);
        if (tile == 0) {
          const uint32_t cap = N_CU * (LDS_LIMIT / p.lds_bytes >= 2u ? 2u : 1u);
          const bool large = P >= (uint64_t)TILE_PTS * TILE_FILL * cap;
          const bool fits = R * TP <= TILE_ROWS || TP == 32, largest = TP == 128 || R * 2 * TP > TILE_ROWS;
          CHECK(large ? TP == 128 : (fits && largest), "tile %u for %llu points, %u views", TP, (unsigned long long)P, R);
        }
        CHECK(p.ok, "P %llu R %u refused", (unsigned long long)P, R);
        if (!p.ok) continue;
        ++plans;
        CHECK(p.tile_off == mlp_lds[li] && p.tile_off % 16 == 0, "tile offset %u", p.tile_off);
        CHECK((uint64_t)p.tile_off + (uint64_t)PE_ROWS * (n_pe + 1) * 4 <= p.lds_bytes && p.lds_bytes <= LDS_LIMIT, "LDS %u", p.lds_bytes);
        CHECK(p.blocks >= 1 && p.blocks <= p.n_tiles && p.blocks <= 2 * N_CU, "blocks %u of %u tiles", p.blocks, p.n_tiles);
        CHECK((uint64_t)p.n_tiles * TP >= P && (uint64_t)(p.n_tiles - 1) * TP < P, "tiles %u for %llu", p.n_tiles, (unsigned long long)P);
        CHECK(p.slice_floats % 4 == 0 && p.rows_floats % 4 == 0 && p.ws_floats == p.slice_floats * p.blocks, "slice %llu", (unsigned long long)p.slice_floats);
        CHECK(p.slice_floats <= 0xffffffffull, "slice does not fit 32 bits");
        std::vector<uint8_t> seen(P, 0);
        std::vector<uint8_t> ws(p.ws_floats, 0);                    // one byte per float: which workgroup wrote it (+1)
        for (uint32_t b = 0; b < p.blocks; ++b) {
          const uint64_t rows0 = (uint64_t)b * p.slice_floats, lat0 = rows0 + p.rows_floats;
          for (uint32_t t = b; t < p.n_tiles; t += p.blocks) {
            const uint64_t p0 = tile_first(t, TP);
            const uint32_t npts = tile_points(P, t, TP), nrows = R * npts;
            CHECK(npts >= 1 && npts <= TP, "tile %u holds %u", t, npts);
            for (uint32_t pl = 0; pl < npts; ++pl) ++seen[p0 + pl];
            uint32_t staged = 0;
            for (uint32_t i0 = 0; i0 < nrows; i0 += PE_ROWS) staged += nrows - i0 < PE_ROWS ? nrows - i0 : PE_ROWS;
            CHECK(staged == nrows, "staging visits %u of %u pairs", staged, nrows);
            if (t != b && t + p.blocks < p.n_tiles) continue;      // the writes: a workgroup's first and last tile
            for (uint32_t r = 0; r < R; ++r)
              for (uint32_t pl = 0; pl < npts; ++pl) {
                const uint32_t s = pair_slot(r, pl, npts);
                CHECK(s < nrows, "slot %u of %u", s, nrows);
                ws.at(rows0 + (uint64_t)s * ld) = (uint8_t)(b % 255 + 1);
                ws.at(rows0 + (uint64_t)s * ld + ld - 1) = (uint8_t)(b % 255 + 1);
                ws.at(lat0 + (uint64_t)s * hid) = (uint8_t)(b % 255 + 1);
                ws.at(lat0 + (uint64_t)s * hid + hid - 1) = (uint8_t)(b % 255 + 1);
                CHECK(rows0 + (uint64_t)s * ld + ld <= lat0 && lat0 + (uint64_t)s * hid + hid <= rows0 + p.slice_floats, "slot %u leaves its block", s);
              }
          }
        }
        long bad = 0;
        for (uint8_t v : seen) bad += v != 1;
        CHECK(bad == 0, "P %llu R %u: %ld points not covered exactly once", (unsigned long long)P, R, bad);
      }
  // (d)
  CHECK(!plan(0, 3, 48, 64, 32, 38400).ok, "no points");
  CHECK(!plan(1ull << 31, 3, 48, 64, 32, 38400).ok, "2^31 points");
  CHECK(!plan(100, 0, 48, 64, 32, 38400).ok && !plan(100, 65, 48, 64, 32, 38400).ok, "view count");
  CHECK(!plan(100, 3, 48, 62, 32, 38400).ok && !plan(100, 3, 46, 64, 32, 38400).ok && !plan(100, 3, 96, 64, 32, 38400).ok, "columns");
  CHECK(!plan(100, 3, 48, 64, 30, 38400).ok && !plan(100, 3, 48, 64, 68, 38400).ok, "outputs");
  CHECK(!plan(100, 3, 48, 64, 32, 0).ok && !plan(100, 3, 48, 64, 32, 160 * 1024).ok && !plan(100, 3, 48, 64, 32, 38401).ok, "LDS");
  CHECK(plan((1ull << 31) - 1, 64, 48, 64, 32, 73728).ok, "largest accepted size");
  CHECK(!plan(100, 3, 48, 64, 32, 38400, 16).ok && !plan(100, 3, 48, 64, 32, 38400, 96).ok, "tile size");
  printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}
