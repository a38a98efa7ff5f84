// Tile and grid arithmetic of the channels-last convolution, the 3x3/2 max pool and the LPIPS head (lpips.hip), free of HIP headers:
// the plan of a layer (K chunking, LDS layout, grid), the staging map of a chunk, the A-operand addresses of the implicit GEMM and
// which accumulator element is which output.  lpips.hip computes every address through these functions, and
// tools/conv_plan_check.cpp holds them to the conditions the kernels rely on (staged addresses inside the image or zero pads and
// inside the LDS tile, every output written once, LDS within the budget, grids within the limits), under sanitizers, on a machine
// without a GPU.
//
// The GEMM: M = output pixels (32 consecutive pixels of one output row per matrix tile), N = 64 output channels per workgroup,
// K = (ky, channel slice, kx, channel in slice).  K is reduced CHUNK by chunk, a chunk = one kernel row ky and one slice of CK input
// channels: the workgroup stages, for its 8 output rows, the ONE input row each of them reads under ky (IN_COLS pixels x CK channels,
// pixel pitch CKP floats: odd where CK is even, so that the 32 pixels of a matrix tile fall into different LDS banks) and the chunk's
// [KC_PAD][64] slice of the packed weight image.  Inside a chunk k = kx CK + c, and an A operand is
// tile[pixel_base(ly, lx) + k_offset(k)].  KC = ks CK is padded to even (v_mfma_f32_32x32x2_f32 takes two k per instruction) with a
// zero weight row whose A operand is the constant 0, never a load (0 * NaN would not be 0).
//
// Packed weight image of a layer: [Cout / 64][n_chunks][KC_PAD][64] floats, chunk = ky n_cslices + cs,
// element (cb, chunk, kx CK + c, o) = weight[cb 64 + o][cs CK + c][ky][kx].
#pragma once
#include <stdint.h>
#include "conv_tile.hpp"

#if defined(__HIPCC__)
#define DNS_CONV_HD __host__ __device__ inline
#else
#define DNS_CONV_HD inline
#endif

namespace dns {
namespace convp {

// the workgroup shape and the accumulator map: conv_tile.hpp's, shared with the image stem (stem_tile.hpp)
using convt::THREADS; using convt::WAVES; using convt::TILE_W; using convt::ROWS_PER_WAVE; using convt::TILE_H;
using convt::row_of; using convt::acc_pixel; using convt::acc_channel;
#if defined(__HIPCC__)
using convt::f32x16; using convt::relu;
#endif
constexpr int NB = 64;                             // output channels per workgroup: two N blocks of 32
constexpr int LDS_FLOATS = 15360;                  // 60 KB of static LDS: two workgroups per CU
constexpr int LDS_BYTES = LDS_FLOATS * 4;
constexpr int LDS_LIMIT_BYTES = 160 * 1024;
constexpr int MAX_SIDE = 32768, MAX_KS = 11, MAX_CIN = 4096, MAX_COUT = 4096;
// the staging loads of a chunk are held in registers while the previous chunk is multiplied: at most this many per thread
constexpr int W_ITERS = 6;                         // float4 loads of the weight slice: KC_PAD <= 96
constexpr int IN_ITERS_V4 = 9, IN_ITERS_V1 = 13;   // loads of the input rows, float4 / scalar
DNS_CONV_HD constexpr int in_iters(int vec) { return vec == 4 ? IN_ITERS_V4 : IN_ITERS_V1; }
static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
static_assert(2 * LDS_BYTES <= LDS_LIMIT_BYTES, "two workgroups per CU");

struct Plan {
  int H, W, Cin, Cout, ks, stride, pad;            // the layer
  int h, w;                                        // output extent
  int vec;                                         // floats per staging load: 4 where Cin % 4 == 0, else 1
  int CK, CKP;                                     // channels per chunk, pixel pitch of the staged rows in floats
  int n_cslices, n_chunks;                         // Cin / CK, ks * n_cslices
  int KC, KC_PAD;                                  // k per chunk (ks CK), padded to even
  int IN_COLS, ROW_STRIDE, IN_FLOATS;              // staged pixels per row, floats per staged row, floats of the 8 rows
  int W_FLOATS, IN_OFF;                            // weight slice (at LDS offset 0), offset of the input rows
  int stage_items;                                 // staging loads of the input rows per chunk (vec floats each)
  uint32_t tiles_x, tiles_y, cout_blocks;
};

DNS_CONV_HD int out_extent(int in_extent, int ks, int stride, int pad) {
  const int span = in_extent + 2 * pad - ks;
  return span < 0 ? 0 : span / stride + 1;
}

// channels per chunk: the whole of Cin where it is no multiple of 4 (the 3-channel image), else the largest of 32, 16, 8, 4 that
// divides Cin and fits LDS; 0 = no fit.  Depends on (Cin, ks, stride) alone, so a weight image serves every image size.
DNS_CONV_HD int lds_floats_for(int CK, int ks, int stride) {
  const int CKP = (CK % 2 == 0) ? CK + 1 : CK;
  const int in_cols = stride * (TILE_W - 1) + ks;
  const int kc_pad = (ks * CK + 1) / 2 * 2;
  return kc_pad * NB + TILE_H * in_cols * CKP;
}
DNS_CONV_HD int chunk_channels(int Cin, int ks, int stride) {
  if (Cin % 4 != 0) return lds_floats_for(Cin, ks, stride) <= LDS_FLOATS ? Cin : 0;
  for (int ck = 32; ck >= 4; ck /= 2)
    if (Cin % ck == 0 && lds_floats_for(ck, ks, stride) <= LDS_FLOATS) return ck;
  return 0;
}

// false: a refused layer or image size
DNS_CONV_HD bool make_plan(int H, int W, int Cin, int Cout, int ks, int stride, int pad, Plan* p) {
  if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || Cin < 1 || Cin > MAX_CIN || Cout < NB || Cout > MAX_COUT || Cout % NB != 0)
    return false;
  if (ks < 1 || ks > MAX_KS || stride < 1 || stride > 4 || pad < 0 || pad >= ks) return false;
  p->H = H, p->W = W, p->Cin = Cin, p->Cout = Cout, p->ks = ks, p->stride = stride, p->pad = pad;
  p->h = out_extent(H, ks, stride, pad), p->w = out_extent(W, ks, stride, pad);
  if (p->h < 1 || p->w < 1) return false;
  p->CK = chunk_channels(Cin, ks, stride);
  if (p->CK < 1) return false;
  p->vec = (Cin % 4 == 0) ? 4 : 1;
  p->CKP = (p->CK % 2 == 0) ? p->CK + 1 : p->CK;
  p->n_cslices = Cin / p->CK;
  p->n_chunks = ks * p->n_cslices;
  p->KC = ks * p->CK;
  p->KC_PAD = (p->KC + 1) / 2 * 2;
  p->IN_COLS = stride * (TILE_W - 1) + ks;
  p->ROW_STRIDE = p->IN_COLS * p->CKP;
  p->IN_FLOATS = TILE_H * p->ROW_STRIDE;
  p->W_FLOATS = p->KC_PAD * NB;
  p->IN_OFF = p->W_FLOATS;
  p->stage_items = TILE_H * p->IN_COLS * (p->CK / p->vec);
  p->tiles_x = (uint32_t)((p->w + TILE_W - 1) / TILE_W);
  p->tiles_y = (uint32_t)((p->h + TILE_H - 1) / TILE_H);
  p->cout_blocks = (uint32_t)(Cout / NB);
  if ((int64_t)H * W * Cin >= (1ll << 31)) return false;                   // a row offset inside an image is an int
  if (p->W_FLOATS / 4 > W_ITERS * THREADS || p->stage_items > in_iters(p->vec) * THREADS) return false;
  return p->IN_OFF + p->IN_FLOATS <= LDS_FLOATS;
}

// workgroups of a call; the caller refuses >= 2^31
DNS_CONV_HD uint64_t grid_size(const Plan& p, uint32_t n) { return (uint64_t)n * p.tiles_y * p.tiles_x * p.cout_blocks; }
// floats of the packed weight image
DNS_CONV_HD uint64_t pack_floats(const Plan& p) { return (uint64_t)p.cout_blocks * p.n_chunks * p.W_FLOATS; }
DNS_CONV_HD uint64_t pack_offset(const Plan& p, uint32_t cb, int chunk) { return ((uint64_t)cb * p.n_chunks + chunk) * p.W_FLOATS; }

struct Tile {
  uint32_t img, cb;      // image of the batch, block of 64 output channels
  int oy0, ox0;          // first output pixel
};
DNS_CONV_HD Tile tile_of(uint64_t block, const Plan& p) {
  Tile t;
  t.cb = (uint32_t)(block % p.cout_blocks);
  const uint64_t rest = block / p.cout_blocks;
  const uint32_t per = p.tiles_x * p.tiles_y;
  t.img = (uint32_t)(rest / per);
  const uint32_t r = (uint32_t)(rest % per);
  t.oy0 = (int)(r / p.tiles_x) * TILE_H;
  t.ox0 = (int)(r % p.tiles_x) * TILE_W;
  return t;
}

// Staging item i in [0, stage_items) of chunk (ky, cs): the LDS float offset inside the input rows, and the float offset inside the
// IMAGE its `vec` floats are loaded from (-1 = zero pad).  Row r of the tile holds the input row that output row oy0 + r reads
// under ky.  What does not depend on the chunk is an Item, which a thread works out once: the tile row (with the first channel of
// the item inside the slice in the bits above), the float offset inside an image row (-1: left or right of the image) and the LDS
// offset.
struct Item {
  int r_cv;              // r | cv vec << 4
  int col;               // ix Cin + cv vec, or -1
  int lds;
};
DNS_CONV_HD int stage_lds(const Plan& p, int i) {
  const int cvs = p.CK / p.vec;
  const int cv = i % cvs, px = i / cvs;
  return (px / p.IN_COLS) * p.ROW_STRIDE + (px % p.IN_COLS) * p.CKP + cv * p.vec;
}
DNS_CONV_HD Item stage_item(const Plan& p, const Tile& t, int i) {
  const int cvs = p.CK / p.vec;
  const int cv = i % cvs, px = i / cvs;
  const int r = px / p.IN_COLS, xc = px % p.IN_COLS;
  const int ix = p.stride * t.ox0 - p.pad + xc;
  Item it;
  it.r_cv = r | ((cv * p.vec) << 4);
  it.col = (ix < 0 || ix >= p.W) ? -1 : ix * p.Cin + cv * p.vec;
  it.lds = r * p.ROW_STRIDE + xc * p.CKP + cv * p.vec;
  return it;
}
DNS_CONV_HD int64_t item_src(const Plan& p, const Tile& t, const Item& it, int ky, int cs) {
  const int iy = p.stride * (t.oy0 + (it.r_cv & 15)) + ky - p.pad;
  if (iy < 0 || iy >= p.H || it.col < 0) return -1;
  return (int64_t)iy * (p.W * p.Cin) + it.col + cs * p.CK;
}
DNS_CONV_HD int64_t stage_src(const Plan& p, const Tile& t, int ky, int cs, int i) { return item_src(p, t, stage_item(p, t, i), ky, cs); }

// A operand: rows[pixel_base(ly, lx) + k_offset(kx, c)] for the output pixel (ly, lx) of the tile, kx < ks, c < CK
DNS_CONV_HD int pixel_base(const Plan& p, int ly, int lx) { return ly * p.ROW_STRIDE + p.stride * lx * p.CKP; }
DNS_CONV_HD int k_offset(const Plan& p, int kx, int c) { return kx * p.CKP + c; }

// ---- max pool 3x3 stride 2, no padding, floor mode
DNS_CONV_HD int pool_extent(int e) { return e < 3 ? 0 : (e - 3) / 2 + 1; }

// ---- LPIPS head: a workgroup of 4 waves takes HEAD_PIXELS consecutive pixels of one pair (a wave HEAD_PIXELS / 4 consecutive ones)
// and leaves one float64 partial; the number of workgroups per pair depends on h w alone
constexpr int HEAD_PIXELS = 64;
constexpr int HEAD_BATCH = 4;                      // pixels a wave has in flight
constexpr int HEAD_MAX_C = 512;
constexpr int LPIPS_LAYERS = 5;
DNS_CONV_HD uint32_t head_blocks(uint64_t hw) { return (uint32_t)((hw + HEAD_PIXELS - 1) / HEAD_PIXELS); }

}  // namespace convp
}  // namespace dns
