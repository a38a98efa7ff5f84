// Host check of the channels-last convolution's plan (dns_slam_amd/csrc/conv_plan.hpp) under the address and undefined-behaviour
// sanitizers.  No GPU is involved and nothing is loaded into Python: plain loops walk the addresses csrc/lpips.hip computes through
// the same functions.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/conv_plan_check.cpp -o /tmp/conv_plan_check
//   /tmp/conv_plan_check
//
// The five AlexNet layers of LPIPS are taken at the input sizes an S x (1331 - S) image gives them, for every S in 31..1300 (both
// sides sweep the whole range, odd sizes included; n = 2, so that the image index of a workgroup is exercised).  For every such
// layer shape it checks:
//   (a) the plan: output extent, chunking (CK divides Cin, K padded to even by less than 2), the LDS regions do not overlap and
//       fit the 60 KB the kernel declares, twice that fits 160 KiB, the staging loads of a chunk fit the registers that hold them,
//       the grid is below 2^31 and the packed weight image's chunk offsets are 16-byte aligned and inside it;
//   (b) the tiles cover every output element [n,h,w,Cout/64 blocks] exactly once, and the accumulator map covers a tile once;
//   (c) the pool extents keep every window inside its input, and the head's workgroups cover every pixel once.
// For the sizes S in 31..130 and a list of large ones, on the corner, edge and one interior tile and for the first and last channel
// slice of every kernel row, it walks the addresses:
//   (d) every staged item comes from inside the image -- and then from the input pixel and channel its LDS slot stands for -- or is
//       a zero pad, exactly where that pixel lies outside the image; the `vec` floats of an item stay inside one pixel;
//   (e) every staged LDS slot lies inside the input rows, no slot is staged twice, and the A-operand address of every in-image
//       output pixel and every k of the chunk is a staged slot holding the tap (s oy + ky - pad, s ox + kx - pad, cs CK + c).
#include <stdio.h>
#include <stdint.h>
#include <set>
#include <vector>
#include "../dns_slam_amd/csrc/conv_plan.hpp"

using namespace dns::convp;

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

struct Layer {
  int Cin, Cout, ks, stride, pad;
  bool pooled;
};
static const Layer LAYERS[5] = {{3, 64, 11, 4, 2, false}, {64, 192, 5, 1, 2, true}, {192, 384, 3, 1, 1, true},
                                {384, 256, 3, 1, 1, false}, {256, 256, 3, 1, 1, false}};

static void check_plan(const Plan& p, const Layer& L, int H, int W, uint32_t n) {
  CHECK(p.h == (H + 2 * L.pad - L.ks) / L.stride + 1 && p.w == (W + 2 * L.pad - L.ks) / L.stride + 1, "output extent of %d x %d", H, W);
  CHECK(p.CK >= 1 && L.Cin % p.CK == 0 && p.n_cslices * p.CK == L.Cin && p.n_chunks == L.ks * p.n_cslices, "chunking of Cin %d: CK %d", L.Cin, p.CK);
  CHECK(p.vec == 1 || (p.vec == 4 && p.CK % 4 == 0 && L.Cin % 4 == 0), "vec %d with CK %d", p.vec, p.CK);
  CHECK(p.KC == L.ks * p.CK && p.KC_PAD % 2 == 0 && p.KC_PAD >= p.KC && p.KC_PAD - p.KC < 2, "K padding %d -> %d", p.KC, p.KC_PAD);
  CHECK(p.CKP >= p.CK && p.ROW_STRIDE == p.IN_COLS * p.CKP && p.IN_FLOATS == TILE_H * p.ROW_STRIDE, "row layout");
  CHECK(p.W_FLOATS == p.KC_PAD * NB && p.W_FLOATS % 4 == 0 && p.IN_OFF >= p.W_FLOATS, "weight slice of %d floats, rows at %d", p.W_FLOATS, p.IN_OFF);
  CHECK(p.IN_OFF + p.IN_FLOATS <= LDS_FLOATS, "LDS plan of %d floats", p.IN_OFF + p.IN_FLOATS);
  CHECK(2 * LDS_BYTES <= LDS_LIMIT_BYTES, "two workgroups of %d bytes", LDS_BYTES);
  const uint64_t grid = grid_size(p, n);
  CHECK(grid >= n && grid < (1ull << 31), "grid %llu", (unsigned long long)grid);
  CHECK(p.stage_items == TILE_H * p.IN_COLS * (p.CK / p.vec), "stage items %d", p.stage_items);
  CHECK(p.stage_items <= in_iters(p.vec) * THREADS && p.W_FLOATS / 4 <= W_ITERS * THREADS, "%d items and %d weight loads over the registers that hold them",
        p.stage_items, p.W_FLOATS / 4);
  CHECK((int64_t)H * W * L.Cin < (1ll << 31) && (int64_t)(p.W - 1) * L.Cin + L.Cin - 1 < (1ll << 31), "offsets inside an image of %d x %d x %d", H, W, L.Cin);
  for (uint32_t cb = 0; cb < p.cout_blocks; ++cb)
    for (int ch = 0; ch < p.n_chunks; ++ch) {
      const uint64_t o = pack_offset(p, cb, ch);
      CHECK(o % 4 == 0 && o + p.W_FLOATS <= pack_floats(p), "chunk (%u, %d) of the weight image at %llu", cb, ch, (unsigned long long)o);
    }
}

static void check_cover(const Plan& p, int H, int W, uint32_t n) {
  std::vector<uint8_t> written((size_t)n * p.h * p.w * p.cout_blocks, 0);
  const uint64_t grid = grid_size(p, n);
  for (uint64_t b = 0; b < grid; ++b) {
    const Tile t = tile_of(b, p);
    CHECK(t.img < n && t.cb < p.cout_blocks && t.oy0 < p.h && t.ox0 < p.w && t.oy0 % TILE_H == 0 && t.ox0 % TILE_W == 0, "tile %llu of %d x %d",
          (unsigned long long)b, H, W);
    if (!(t.img < n && t.cb < p.cout_blocks)) continue;
    for (int ly = 0; ly < TILE_H; ++ly)
      for (int lx = 0; lx < TILE_W; ++lx) {
        const int oy = t.oy0 + ly, ox = t.ox0 + lx;
        if (oy < 0 || ox < 0 || oy >= p.h || ox >= p.w) continue;
        uint8_t& c = written[(((size_t)t.img * p.h + oy) * p.w + ox) * p.cout_blocks + t.cb];
        if (c < 255) ++c;
      }
  }
  long bad = 0;
  for (uint8_t v : written) bad += v != 1;
  CHECK(bad == 0, "%d x %d: %ld output elements not written exactly once", H, W, bad);
}

static void walk_tile(const Plan& p, const Layer& L, const Tile& t, int H, int W) {
  const int64_t img_floats = (int64_t)H * W * L.Cin;
  for (int ky = 0; ky < L.ks; ++ky)
    for (int cs : {0, p.n_cslices - 1}) {
      std::vector<int64_t> slot(p.IN_FLOATS, -2);      // -2 = never staged, -1 = zero pad, else the image float
      for (int i = 0; i < p.stage_items; ++i) {
        const int d = stage_lds(p, i);
        CHECK(d >= 0 && d + p.vec <= p.IN_FLOATS, "H %d W %d: item %d staged to %d", H, W, i, d);
        if (d < 0 || d + p.vec > p.IN_FLOATS) continue;
        const int64_t s = stage_src(p, t, ky, cs, i);
        const Item it = stage_item(p, t, i);
        CHECK(it.lds == d && (it.r_cv & 15) == d / p.ROW_STRIDE && (it.r_cv >> 4) == (d % p.ROW_STRIDE) % p.CKP && item_src(p, t, it, ky, cs) == s,
              "H %d W %d: item %d = (%d, %d, %d)", H, W, i, it.r_cv, it.col, it.lds);
        CHECK(s >= -1 && s + p.vec <= img_floats && (s < 0 || s % p.vec == 0), "H %d W %d: item %d read from %lld of %lld", H, W, i, (long long)s,
              (long long)img_floats);
        const int r = d / p.ROW_STRIDE, xc = (d % p.ROW_STRIDE) / p.CKP, c = (d % p.ROW_STRIDE) % p.CKP;
        CHECK(r < TILE_H && xc < p.IN_COLS && c + p.vec <= p.CK, "H %d W %d: slot %d = (%d, %d, %d)", H, W, d, r, xc, c);
        const int iy = L.stride * (t.oy0 + r) + ky - L.pad, ix = L.stride * t.ox0 - L.pad + xc;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        CHECK(s == (inside ? ((int64_t)iy * W + ix) * L.Cin + cs * p.CK + c : -1), "H %d W %d: slot %d holds %lld", H, W, d, (long long)s);
        for (int e = 0; e < p.vec; ++e) {
          CHECK(slot[d + e] == -2, "H %d W %d: slot %d staged twice", H, W, d + e);
          slot[d + e] = s < 0 ? -1 : s + e;
        }
      }
      for (int ly = 0; ly < TILE_H; ++ly)
        for (int lx = 0; lx < TILE_W; ++lx) {
          const int oy = t.oy0 + ly, ox = t.ox0 + lx;
          if (oy >= p.h || ox >= p.w) continue;
          // the kernel's walk over k: (kx, c) advanced by two per step from k = hk, per lane; where the staging loads are
          // float4 (CK even, no pad row) the kernel keeps (ukx, uc) for the whole wave and a lane reads c = uc + hk
          for (int hk = 0; hk < 2; ++hk) {
            int kk = hk, kx = 0, c = hk;
            if (c >= p.CK) c -= p.CK, ++kx;
            int ukx = 0, uc = 0;
            for (int s = 0; s < p.KC_PAD / 2; ++s) {
              if (p.vec == 4) {
                CHECK(p.CK % 2 == 0 && p.KC_PAD == p.KC && ukx == kx && uc + hk == c && 2 * s + hk == kk, "uniform walk: step %d -> (%d, %d), lane (%d, %d)", s,
                      ukx, uc, kx, c);
                uc += 2;
                if (uc >= p.CK) uc = 0, ++ukx;
              }
              if (kk < p.KC) {
                CHECK(kx < L.ks && c < p.CK && kx * p.CK + c == kk, "k %d -> (%d, %d)", kk, kx, c);
                const int a = pixel_base(p, ly, lx) + k_offset(p, kx, c);
                CHECK(a >= 0 && a < p.IN_FLOATS, "H %d W %d: operand address %d", H, W, a);
                if (a >= 0 && a < p.IN_FLOATS) {
                  const int iy = L.stride * oy + ky - L.pad, ix = L.stride * ox + kx - L.pad;
                  const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
                  CHECK(slot[a] == (inside ? ((int64_t)iy * W + ix) * L.Cin + cs * p.CK + c : -1), "H %d W %d: pixel (%d, %d) ky %d k %d reads slot %d = %lld",
                        H, W, oy, ox, ky, kk, a, (long long)slot[a]);
                }
              }
              kk += 2, c += 2;
              if (c >= p.CK) c -= p.CK, ++kx;
              if (c >= p.CK) c -= p.CK, ++kx;
            }
          }
        }
    }
}

int main() {
  // the accumulator map covers a tile's 8 x 32 pixels x 64 channels once
  {
    std::vector<int> cnt(TILE_H * TILE_W * NB, 0);
    for (int wave = 0; wave < WAVES; ++wave)
      for (int mt = 0; mt < ROWS_PER_WAVE; ++mt)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 16; ++r)
            for (int nb = 0; nb < 2; ++nb) {
              const int ly = row_of(wave, mt), lx = acc_pixel(r, lane), ch = acc_channel(lane) + 32 * nb;
              CHECK(ly >= 0 && ly < TILE_H && lx >= 0 && lx < TILE_W && ch >= 0 && ch < NB, "accumulator (%d, %d, %d, %d)", wave, mt, lane, r);
              if (ly >= 0 && ly < TILE_H && lx >= 0 && lx < TILE_W && ch >= 0 && ch < NB) ++cnt[(ly * TILE_W + lx) * NB + ch];
            }
    long bad = 0;
    for (int v : cnt) bad += v != 1;
    CHECK(bad == 0, "accumulator map: %ld elements of a tile not covered once", bad);
  }
  std::set<int> walk;
  for (int s = 31; s <= 130; ++s) walk.insert(s);
  for (int s : {131, 255, 256, 257, 479, 480, 511, 640, 679, 680, 681, 1023, 1024, 1199, 1200, 1201, 1299, 1300}) walk.insert(s);
  const uint32_t n = 2;
  long shapes = 0, tiles_walked = 0;
  int max_lds = 0;
  for (int S = 31; S <= 1300; ++S) {
    int H = S, W = 1331 - S;
    for (int l = 0; l < 5; ++l) {
      const Layer& L = LAYERS[l];
      if (L.pooled) {
        const int ph = pool_extent(H), pw = pool_extent(W);
        CHECK(ph >= 1 && pw >= 1 && 2 * (ph - 1) + 2 <= H - 1 && 2 * (pw - 1) + 2 <= W - 1 && 2 * ph + 2 > H - 1 && 2 * pw + 2 > W - 1,
              "pool of %d x %d -> %d x %d", H, W, ph, pw);
        H = ph, W = pw;
      }
      Plan p;
      const bool ok = make_plan(H, W, L.Cin, L.Cout, L.ks, L.stride, L.pad, &p);
      CHECK(ok, "layer %d at %d x %d is refused", l, H, W);
      if (!ok) break;
      check_plan(p, L, H, W, n);
      check_cover(p, H, W, n);
      max_lds = (p.IN_OFF + p.IN_FLOATS) * 4 > max_lds ? (p.IN_OFF + p.IN_FLOATS) * 4 : max_lds;
      const uint64_t hw = (uint64_t)p.h * p.w;
      const uint32_t hb = head_blocks(hw);
      CHECK(hb >= 1 && (uint64_t)hb * HEAD_PIXELS >= hw && (uint64_t)(hb - 1) * HEAD_PIXELS < hw && L.Cout % 64 == 0 && L.Cout <= HEAD_MAX_C,
            "head of %d x %d x %d: %u workgroups", p.h, p.w, L.Cout, hb);
      if (walk.count(S)) {
        std::set<uint64_t> blocks;
        const uint32_t tx = p.tiles_x, ty = p.tiles_y;
        for (uint32_t y : {0u, ty / 2, ty - 1})
          for (uint32_t x : {0u, tx / 2, tx - 1})
            blocks.insert(((uint64_t)(n - 1) * ty * tx + (uint64_t)y * tx + x) * p.cout_blocks + (p.cout_blocks - 1));
        for (uint64_t b : blocks) {
          walk_tile(p, L, tile_of(b, p), H, W);
          ++tiles_walked;
        }
      }
      H = p.h, W = p.w;
      ++shapes;
    }
  }
  // refused shapes stay refused
  Plan q;
  CHECK(!make_plan(8, 8, 64, 100, 3, 1, 1, &q), "Cout 100 accepted");
  CHECK(!make_plan(8, 8, 64, 64, 13, 1, 1, &q), "kernel 13 accepted");
  CHECK(!make_plan(2, 2, 64, 64, 5, 1, 0, &q), "an image smaller than the kernel accepted");
  CHECK(!make_plan(8, 8, 64, 64, 3, 1, 3, &q), "pad 3 of a 3 x 3 kernel accepted");
  CHECK(!make_plan(40000, 8, 64, 64, 3, 1, 1, &q), "a side of 40000 accepted");
  CHECK(!make_plan(64, 64, 10, 64, 11, 4, 2, &q) || q.IN_OFF + q.IN_FLOATS <= LDS_FLOATS, "Cin 10, kernel 11 over the LDS budget");
  printf("%ld layer shapes, %ld tiles walked, LDS up to %d of %d bytes, %ld failures\n", shapes, tiles_walked, max_lds, LDS_BYTES, g_fail);
  return g_fail ? 1 : 0;
}
