// Tile geometry of the image stem (stem.hip: conv 7x7 stride 2 pad 3, 3 -> 64 channels, on [n,H,W,3] images), free of HIP headers:
// the output tile of a workgroup, the input tile with its halo, the LDS layout, the K -> (ky, kx, c) map of the implicit GEMM, which
// accumulator element is which output pixel, the grid and the number of partial-sum rows.  stem.hip computes every address through
// these functions, and tools/stem_tile_check.cpp holds them to the conditions the kernel relies on (staged addresses inside the image
// or zero pads and inside the LDS tile, every output written once, LDS within the budget), under sanitizers, on a machine without a GPU.
//
// The GEMM: M = output pixels, N = output channels, K = (ky, kx, c) -- so the 21 floats (kx, c) of one kernel row are 21 CONSECUTIVE
// floats of one row of the channels-last input tile, and an A operand is input_tile[pixel_base + k_offset(k)].  K is padded 147 -> 148
// (v_mfma_f32_32x32x2_f32 takes two k per instruction) with a zero weight row; the A operand of k = 147 is the constant 0, never a load
// (0 * NaN would not be 0).
#pragma once
#include <stdint.h>
#include "conv_tile.hpp"

#if defined(__HIPCC__)
#define DNS_STEM_HD __host__ __device__ inline
#else
#define DNS_STEM_HD inline
#endif

namespace dns {
namespace stem {

constexpr int KH = 7, KW = 7, CIN = 3, COUT = 64, STRIDE = 2, PAD = 3;
constexpr int K_REAL = KH * KW * CIN;              // 147
constexpr int K_PAD = 148;                         // two k per matrix instruction
constexpr int K_ROW = KW * CIN;                    // 21 consecutive floats of an input row per kernel row

// the workgroup shape and the accumulator map: conv_tile.hpp's, shared with the general convolution (conv_plan.hpp)
using convt::THREADS; using convt::WAVES; using convt::TILE_W; using convt::ROWS_PER_WAVE; using convt::TILE_H;
using convt::row_of; using convt::acc_pixel; using convt::acc_channel;
#if defined(__HIPCC__)
using convt::f32x16; using convt::relu;
#endif

constexpr int IN_ROWS = STRIDE * (TILE_H - 1) + KH;        // 21 input rows, halo included
constexpr int IN_COLS = STRIDE * (TILE_W - 1) + KW;        // 69 input columns
constexpr int IN_ROW_FLOATS = IN_COLS * CIN;               // 207 floats staged per row
constexpr int IN_ROW_STRIDE = 208;                         // LDS row stride in floats
constexpr int IN_FLOATS = IN_ROWS * IN_ROW_STRIDE;         // 4368
constexpr int STAGE_ITEMS = IN_ROWS * IN_ROW_FLOATS;       // 4347 floats staged per tile

// LDS layout, in floats: the weight image [K_PAD][COUT], then the input tile; the statistics' float64 scratch [WAVES][64 lanes][4]
// overlays the input tile once the products are done
constexpr int LDS_W_OFF = 0;
constexpr int LDS_W_FLOATS = K_PAD * COUT;                 // 9472
constexpr int LDS_IN_OFF = LDS_W_OFF + LDS_W_FLOATS;
constexpr int LDS_FLOATS = LDS_IN_OFF + IN_FLOATS;         // 13840 floats = 55360 bytes: two workgroups per CU
constexpr int LDS_BYTES = LDS_FLOATS * 4;
constexpr int STAT_DOUBLES = WAVES * 64 * 4;               // 1024 doubles = 2048 floats <= IN_FLOATS
constexpr int LDS_LIMIT_BYTES = 160 * 1024;
static_assert(STAT_DOUBLES * 2 <= IN_FLOATS, "statistics scratch overlays the input tile");
static_assert((LDS_IN_OFF * 4) % 8 == 0, "float64 scratch alignment");
static_assert(LDS_BYTES <= 64 * 1024, "static LDS");

DNS_STEM_HD int out_extent(int in_extent) { return (in_extent - 1) / STRIDE + 1; }
DNS_STEM_HD uint32_t tiles_x(int W) { return (uint32_t)((out_extent(W) + TILE_W - 1) / TILE_W); }
DNS_STEM_HD uint32_t tiles_y(int H) { return (uint32_t)((out_extent(H) + TILE_H - 1) / TILE_H); }
// workgroups of a call = rows of float64 partial sums (one row of 2 * COUT doubles per workgroup); 0 = too many for one grid
DNS_STEM_HD uint64_t grid_size(uint32_t n, int H, int W) { return (uint64_t)n * tiles_y(H) * tiles_x(W); }
DNS_STEM_HD uint64_t partial_rows(uint32_t n, int H, int W) { return grid_size(n, H, W); }
// the partial rows are added in two levels, each in index order: level 1 sums runs of reduce_chunk rows into <= REDUCE_ROWS rows
constexpr uint32_t REDUCE_ROWS = 256;
DNS_STEM_HD uint32_t reduce_chunk(uint64_t rows) { return (uint32_t)((rows + REDUCE_ROWS - 1) / REDUCE_ROWS); }
DNS_STEM_HD uint32_t reduce_rows(uint64_t rows) {
  const uint32_t c = reduce_chunk(rows);
  return c ? (uint32_t)((rows + c - 1) / c) : 0u;
}

struct Tile {
  uint32_t img;          // image of the batch
  int oy0, ox0;          // first output pixel
  int iy0, ix0;          // input pixel at LDS (row 0, column 0): may be negative (zero padding)
};
DNS_STEM_HD Tile tile_of(uint64_t block, int H, int W) {
  const uint32_t tx = tiles_x(W), ty = tiles_y(H);
  Tile t;
  t.img = (uint32_t)(block / ((uint64_t)tx * ty));
  const uint32_t r = (uint32_t)(block % ((uint64_t)tx * ty));
  t.oy0 = (int)(r / tx) * TILE_H;
  t.ox0 = (int)(r % tx) * TILE_W;
  t.iy0 = t.oy0 * STRIDE - PAD;
  t.ix0 = t.ox0 * STRIDE - PAD;
  return t;
}

// Staging item i in [0, STAGE_ITEMS): LDS float offset inside the input tile, and the float offset inside the IMAGE it is loaded
// from (-1 = zero pad).  A tile row is one contiguous run of the channels-last image row.
DNS_STEM_HD int stage_lds(int i) { return (i / IN_ROW_FLOATS) * IN_ROW_STRIDE + i % IN_ROW_FLOATS; }
DNS_STEM_HD int64_t stage_src(const Tile& t, int i, int H, int W) {
  const int r = i / IN_ROW_FLOATS, f = i % IN_ROW_FLOATS;
  const int iy = t.iy0 + r;
  const int64_t x3 = (int64_t)t.ix0 * CIN + f;             // float index inside the image row
  if (iy < 0 || iy >= H || x3 < 0 || x3 >= (int64_t)W * CIN) return -1;
  return (int64_t)iy * W * CIN + x3;
}

// A operand: input_tile[pixel_base(ly, lx) + k_offset(k)] for the output pixel (ly, lx) of the tile and k < K_REAL
DNS_STEM_HD int pixel_base(int ly, int lx) { return (STRIDE * ly) * IN_ROW_STRIDE + (STRIDE * lx) * CIN; }
DNS_STEM_HD int k_offset(int k) {
  const int ky = k / K_ROW;
  return ky * IN_ROW_STRIDE + (k - ky * K_ROW);
}
DNS_STEM_HD void k_tap(int k, int* ky, int* kx, int* c) {
  *ky = k / K_ROW;
  *kx = (k % K_ROW) / CIN;
  *c = k % CIN;
}

}  // namespace stem
}  // namespace dns
