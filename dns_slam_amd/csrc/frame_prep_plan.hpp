// Host plan of dns_prepare_frames (frame_prep.hip): the sizes of the stages, the layout of the table blob and the tables themselves.
// No HIP in here: tools/frame_prep_plan_check.cpp walks it on the host under ASan + UBSan, and dns_frame_prep_tables exports it, so
// a C caller needs no Python.
//
// A frame goes through the stages of BaseDataset.__getitem__ (datas/slam_datasets.py:85-149).  Each stage is separable, so one table
// per stage and axis says, for every destination coordinate, which source coordinate(s) it reads and with which fp32 weights, by the
// resampling rule of the library that runs the stage:
//   cv   linear  colour [Hc,Wc] -> [Hd,Wd]   cv2.resize(color, (Wd, Hd)): index, index + 1 (clamped), weights (1 - f, f)
//   cv   nearest labels [Hl,Wl] -> [Hd,Wd]   cv2.resize(..., INTER_NEAREST): index
//   torch linear colour [Hd,Wd] -> [Hs,Ws]   F.interpolate(mode='bilinear', align_corners=True): index, index + 1 (clamped), weights
//   torch nearest depth, labels [Hd,Wd] -> [Hs,Ws]   F.interpolate(mode='nearest'): index
// and the crop_edge crop reads [edge, Hs - edge) x [edge, Ws - edge) of the last one.  Without crop_size Hs, Ws = Hd, Wd: both torch
// rules are the identity at equal sizes, as both cv rules are, so a stage the reference skips and a stage of equal sizes are one case.
//
// The blob, in 32-bit words (int32 indices, fp32 weights as their bits), in this order:
//   cv_x_idx [Wd], cv_x_w [Wd][2], cv_y_idx [Hd], cv_y_w [Hd][2]           the cv linear stage
//   tb_x_idx [Ws], tb_x_w [Ws][2], tb_y_idx [Hs], tb_y_w [Hs][2]           the torch linear stage
//   tn_x [Ws], tn_y [Hs]                                                   the torch nearest stage
//   cn_x [Wd], cn_y [Hd]                                                   the cv nearest stage (built for Hl, Wl = 0 too: all 0)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/dns_hip.h"

namespace dns {
namespace fprep {

constexpr uint32_t MAX_SIDE = 32768;               // every image side; keeps a frame's pixel count below 2^30
constexpr uint32_t MAX_FRAMES = 65535;             // gridDim.y
constexpr uint32_t FP_BLOCK = 256;                 // threads per workgroup, one output pixel each
constexpr uint32_t IDENT_CV = 1u, IDENT_TORCH = 2u, IDENT_CVN = 4u;   // Plan::ident: stages whose source and destination sizes are equal

struct Plan {
  uint32_t H, W;                                   // the output: Hs - 2 edge, Ws - 2 edge
  uint32_t ident;
  bool labels;
  uint64_t cv_x_idx, cv_x_w, cv_y_idx, cv_y_w, tb_x_idx, tb_x_w, tb_y_idx, tb_y_w, tn_x, tn_y, cn_x, cn_y;   // word offsets
  uint64_t words;
  uint32_t grid_x;                                 // workgroups over one frame's output pixels
};

inline bool side_ok(uint32_t s) { return s >= 1 && s <= MAX_SIDE; }

// false: refused sizes (a side of 0 or beyond MAX_SIDE, labels with one side 0, a crop that leaves nothing).
inline bool make_plan(const DnsFramePrepDims& d, Plan* p) {
  if (!side_ok(d.Hc) || !side_ok(d.Wc) || !side_ok(d.Hd) || !side_ok(d.Wd) || !side_ok(d.Hs) || !side_ok(d.Ws)) return false;
  const bool labels = d.Hl != 0 || d.Wl != 0;
  if (labels && (!side_ok(d.Hl) || !side_ok(d.Wl))) return false;
  if (d.edge >= MAX_SIDE || 2 * d.edge >= d.Hs || 2 * d.edge >= d.Ws) return false;
  p->H = d.Hs - 2 * d.edge, p->W = d.Ws - 2 * d.edge;
  p->labels = labels;
  p->ident = (d.Hc == d.Hd && d.Wc == d.Wd ? IDENT_CV : 0u) | (d.Hs == d.Hd && d.Ws == d.Wd ? IDENT_TORCH : 0u) |
             (labels && d.Hl == d.Hd && d.Wl == d.Wd ? IDENT_CVN : 0u);
  uint64_t o = 0;
  p->cv_x_idx = o, o += d.Wd;
  p->cv_x_w = o, o += 2ull * d.Wd;
  p->cv_y_idx = o, o += d.Hd;
  p->cv_y_w = o, o += 2ull * d.Hd;
  p->tb_x_idx = o, o += d.Ws;
  p->tb_x_w = o, o += 2ull * d.Ws;
  p->tb_y_idx = o, o += d.Hs;
  p->tb_y_w = o, o += 2ull * d.Hs;
  p->tn_x = o, o += d.Ws;
  p->tn_y = o, o += d.Hs;
  p->cn_x = o, o += d.Wd;
  p->cn_y = o, o += d.Hd;
  p->words = o;
  p->grid_x = (uint32_t)(((uint64_t)p->H * p->W + FP_BLOCK - 1) / FP_BLOCK);
  return true;
}

// ---- the four rules: destination coordinate dd of `dst` -> source index in [0, src) (and the weights of index, index + 1) -----------

// cv2 resize, INTER_LINEAR, float32 (the published rule: the coordinate is ROUNDED TO fp32 before the floor, which moves a weight by
// up to 2^-14 at ScanNet's widths against the exact one)
inline void cv_linear(uint32_t dd, uint32_t src, uint32_t dst, int32_t* idx, float* w) {
  const double scale = 1.0 / ((double)dst / (double)src);
  float f = (float)(((double)dd + 0.5) * scale - 0.5);
  int32_t s = (int32_t)floorf(f);
  f -= (float)s;
  if (s < 0) s = 0, f = 0.0f;
  if (s >= (int32_t)src - 1) s = (int32_t)src - 1, f = 0.0f;
  *idx = s, w[0] = 1.0f - f, w[1] = f;
}

// cv2 resize, INTER_NEAREST
inline int32_t cv_nearest(uint32_t dd, uint32_t src, uint32_t dst) {
  const double scale = 1.0 / ((double)dst / (double)src);
  const int32_t s = (int32_t)floor((double)dd * scale);
  return s < (int32_t)src - 1 ? s : (int32_t)src - 1;
}

// F.interpolate(mode='nearest'): nearest_neighbor_compute_source_index with the fp32 scale src / dst
inline int32_t torch_nearest(uint32_t dd, uint32_t src, uint32_t dst) {
  const float scale = (float)src / (float)dst;
  const int32_t s = (int32_t)floorf((float)dd * scale);
  return s < (int32_t)src - 1 ? s : (int32_t)src - 1;
}

// F.interpolate(mode='bilinear', align_corners=True), fp32: area_pixel_compute_scale = (src - 1) / (dst - 1) (0 for dst = 1),
// the source coordinate scale * dd, guard_index_and_lambda
inline void torch_linear(uint32_t dd, uint32_t src, uint32_t dst, int32_t* idx, float* w) {
  const float scale = dst > 1 ? (float)(src - 1) / (float)(dst - 1) : 0.0f;
  const float real = scale * (float)dd;
  int32_t s = (int32_t)floorf(real);
  if (s > (int32_t)src - 1) s = (int32_t)src - 1;
  float lam = real - (float)s;
  lam = lam < 0.0f ? 0.0f : (lam > 1.0f ? 1.0f : lam);
  *idx = s, w[0] = 1.0f - lam, w[1] = lam;
}

inline void put_f(int32_t* words, uint64_t at, float v) { memcpy(words + at, &v, sizeof v); }

// Fills words[0 .. p.words) for the plan p of d.
inline void fill_tables(const DnsFramePrepDims& d, const Plan& p, int32_t* words) {
  float w[2];
  for (uint32_t x = 0; x < d.Wd; ++x) {
    cv_linear(x, d.Wc, d.Wd, words + p.cv_x_idx + x, w);
    put_f(words, p.cv_x_w + 2ull * x, w[0]), put_f(words, p.cv_x_w + 2ull * x + 1, w[1]);
    words[p.cn_x + x] = p.labels ? cv_nearest(x, d.Wl, d.Wd) : 0;
  }
  for (uint32_t y = 0; y < d.Hd; ++y) {
    cv_linear(y, d.Hc, d.Hd, words + p.cv_y_idx + y, w);
    put_f(words, p.cv_y_w + 2ull * y, w[0]), put_f(words, p.cv_y_w + 2ull * y + 1, w[1]);
    words[p.cn_y + y] = p.labels ? cv_nearest(y, d.Hl, d.Hd) : 0;
  }
  for (uint32_t x = 0; x < d.Ws; ++x) {
    torch_linear(x, d.Wd, d.Ws, words + p.tb_x_idx + x, w);
    put_f(words, p.tb_x_w + 2ull * x, w[0]), put_f(words, p.tb_x_w + 2ull * x + 1, w[1]);
    words[p.tn_x + x] = torch_nearest(x, d.Wd, d.Ws);
  }
  for (uint32_t y = 0; y < d.Hs; ++y) {
    torch_linear(y, d.Hd, d.Hs, words + p.tb_y_idx + y, w);
    put_f(words, p.tb_y_w + 2ull * y, w[0]), put_f(words, p.tb_y_w + 2ull * y + 1, w[1]);
    words[p.tn_y + y] = torch_nearest(y, d.Hd, d.Hs);
  }
}

}  // namespace fprep
}  // namespace dns
