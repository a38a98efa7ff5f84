// Host check of the image stem's tile geometry (dns_slam_amd/csrc/stem_tile.hpp) under the address and undefined-behaviour
// sanitizers.  No GPU is involved and nothing is loaded into Python: plain loops walk the addresses csrc/stem.hip computes through
// the same functions.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/stem_tile_check.cpp -o /tmp/stem_tile_check
//   /tmp/stem_tile_check
//
// For every H in 1..80, W in 1..160 (n = 2, so that the image index of a workgroup is exercised) it checks:
//   (a) every staged item comes from inside the image -- and then from the input pixel and channel its LDS slot stands for -- or is
//       a zero pad, exactly where that pixel lies outside the image;
//   (b) every staged LDS slot lies inside the input tile, no slot is staged twice, and every A-operand address of every in-image
//       output pixel and every k < 147 is a staged slot holding the tap (2 oy + ky - 3, 2 ox + kx - 3, c);
//   (c) the accumulator map writes every output element [n,h,w,64] exactly once;
//   (d) the LDS plan fits 160 KiB (and the statistics scratch fits the input tile it overlays);
//   (e) the partial rows and the two-level reduction cover every row once.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../dns_slam_amd/csrc/stem_tile.hpp"

using namespace dns::stem;

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
  CHECK(LDS_BYTES <= LDS_LIMIT_BYTES, "LDS plan %d bytes", LDS_BYTES);
  CHECK(STAT_DOUBLES * 8 <= IN_FLOATS * 4, "statistics scratch %d bytes over a %d-byte tile", STAT_DOUBLES * 8, IN_FLOATS * 4);
  CHECK(LDS_IN_OFF >= LDS_W_OFF + LDS_W_FLOATS && LDS_FLOATS == LDS_IN_OFF + IN_FLOATS, "LDS regions overlap");
  CHECK(K_PAD % 2 == 0 && K_PAD >= K_REAL && K_PAD - K_REAL < 2, "K padding");
  for (int k = 0; k < K_REAL; ++k) {
    int ky, kx, c;
    k_tap(k, &ky, &kx, &c);
    CHECK(ky >= 0 && ky < KH && kx >= 0 && kx < KW && c >= 0 && c < CIN && (ky * KW + kx) * CIN + c == k, "k %d -> (%d, %d, %d)", k, ky, kx, c);
    CHECK(k_offset(k) == ky * IN_ROW_STRIDE + kx * CIN + c, "k_offset(%d) = %d", k, k_offset(k));
  }
  const uint32_t n = 2;
  long shapes = 0;
  for (int H = 1; H <= 80; ++H)
    for (int W = 1; W <= 160; ++W) {
      const int h = out_extent(H), w = out_extent(W);
      CHECK(h == (H + 2 * PAD - KH) / STRIDE + 1 && w == (W + 2 * PAD - KW) / STRIDE + 1, "output extent of %d x %d", H, W);
      const uint64_t grid = grid_size(n, H, W);
      CHECK(grid == partial_rows(n, H, W) && grid >= n, "grid %llu", (unsigned long long)grid);
      std::vector<uint8_t> written((size_t)n * h * w * COUT, 0);
      const int64_t img_floats = (int64_t)H * W * CIN;
      for (uint64_t b = 0; b < grid; ++b) {
        const Tile t = tile_of(b, H, W);
        CHECK(t.img < n && t.oy0 < h && t.ox0 < w && t.oy0 % TILE_H == 0 && t.ox0 % TILE_W == 0, "tile %llu of %d x %d", (unsigned long long)b, H, W);
        if (b >= grid / n) continue;                 // the tiles of image 1 repeat image 0's: walk the addresses once
        // (a), (b): the staging
        std::vector<int64_t> slot(IN_FLOATS, -2);    // -2 = never staged, -1 = zero pad, else the image float
        for (int i = 0; i < STAGE_ITEMS; ++i) {
          const int d = stage_lds(i);
          CHECK(d >= 0 && d < IN_FLOATS, "H %d W %d: item %d staged to %d", H, W, i, d);
          if (d < 0 || d >= IN_FLOATS) continue;
          CHECK(slot[d] == -2, "H %d W %d: slot %d staged twice", H, W, d);
          const int64_t s = stage_src(t, i, H, W);
          CHECK(s >= -1 && s < img_floats, "H %d W %d: item %d read from %lld of %lld", H, W, i, (long long)s, (long long)img_floats);
          slot[d] = s;
          const int r = d / IN_ROW_STRIDE, f = d % IN_ROW_STRIDE;
          const int iy = t.iy0 + r, ix = t.ix0 + f / CIN, c = f % CIN;
          const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
          CHECK(s == (inside ? ((int64_t)iy * W + ix) * CIN + c : -1), "H %d W %d: slot %d holds %lld", H, W, d, (long long)s);
        }
        // (b), (c): operands and stores of every accumulator element
        for (int wave = 0; wave < WAVES; ++wave)
          for (int mt = 0; mt < ROWS_PER_WAVE; ++mt)
            for (int lane = 0; lane < 64; ++lane)
              for (int r = 0; r < 16; ++r) {
                const int ly = row_of(wave, mt), lx = acc_pixel(r, lane);
                CHECK(ly >= 0 && ly < TILE_H && lx >= 0 && lx < TILE_W, "accumulator (%d, %d, %d, %d) -> (%d, %d)", wave, mt, lane, r, ly, lx);
                const int oy = t.oy0 + ly, ox = t.ox0 + lx;
                if (oy >= h || ox >= w) continue;
                for (int nb = 0; nb < 2; ++nb)
                  for (uint32_t img = 0; img < n; ++img) {
                    const int ch = acc_channel(lane) + 32 * nb;
                    uint8_t& cnt = written[(((size_t)img * h + oy) * w + ox) * COUT + ch];
                    if (cnt < 255) ++cnt;
                  }
                if (acc_channel(lane) != 0) continue;              // the operand walk: once per pixel
                for (int k = 0; k < K_REAL; ++k) {
                  const int a = pixel_base(ly, lx) + k_offset(k);
                  CHECK(a >= 0 && a < IN_FLOATS, "H %d W %d: operand address %d", H, W, a);
                  if (a < 0 || a >= IN_FLOATS) continue;
                  int ky, kx, c;
                  k_tap(k, &ky, &kx, &c);
                  const int iy = STRIDE * oy + ky - PAD, ix = STRIDE * ox + kx - PAD;
                  const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
                  CHECK(slot[a] == (inside ? ((int64_t)iy * W + ix) * CIN + c : -1), "H %d W %d: pixel (%d, %d) k %d reads slot %d = %lld", H, W,
                        oy, ox, k, a, (long long)slot[a]);
                }
              }
      }
      long bad = 0;
      for (uint8_t v : written) bad += v != 1;
      CHECK(bad == 0, "H %d W %d: %ld output elements not written exactly once", H, W, bad);
      // (e)
      const uint32_t chunk = reduce_chunk(grid), r1 = reduce_rows(grid);
      CHECK(chunk >= 1 && r1 >= 1 && r1 <= REDUCE_ROWS && (uint64_t)r1 * chunk >= grid && (uint64_t)(r1 - 1) * chunk < grid,
            "reduction of %llu rows: %u rows of %u", (unsigned long long)grid, r1, chunk);
      ++shapes;
    }
  // the reduction at sizes the sweep does not reach
  for (uint64_t rows : {1ull, 255ull, 256ull, 257ull, 9804ull, 65536ull, 65537ull, (1ull << 31) - 1}) {
    const uint32_t chunk = reduce_chunk(rows), r1 = reduce_rows(rows);
    CHECK(chunk >= 1 && r1 >= 1 && r1 <= REDUCE_ROWS && (uint64_t)r1 * chunk >= rows && (uint64_t)(r1 - 1) * chunk < rows,
          "reduction of %llu rows: %u rows of %u", (unsigned long long)rows, r1, chunk);
  }
  printf("%ld shapes, LDS %d bytes, %ld failures\n", shapes, LDS_BYTES, g_fail);
  return g_fail ? 1 : 0;
}
