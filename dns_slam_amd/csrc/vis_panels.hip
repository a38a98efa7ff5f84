// frame_vis's sheet on the device (include/dns_hip.h, "visualisation panels"): fig_plot's 3 x 3 panels (utils/common.py:682-745) --
// rows depth, colour, label; columns input, generated, |difference| -- at native resolution as one uint8 image, in place of six
// full-image host reads and a matplotlib figure.
//
// depth_vmax_kernel: vmax = the largest finite positive gt depth, as an integer atomic maximum over the floats' bits (for positive
// finite floats the order of the bits is the order of the values), one atomic per wave after a wave maximum: the same word on every call.
// vis_panels_kernel: one thread per pixel of the SHEET; it finds its panel, reads at most two source values per channel and stores
// three bytes.  The plasma table (plasma_lut.hpp, generated from matplotlib) is staged in LDS once per workgroup.
// Bounds: a thread past the sheet returns; a source pixel is read only inside a panel (y < H, x < W); the label table is read at
// 0 <= label < n_lut only; the plasma index is clamped to 0..255 before the table read.
#include "common.hpp"
#include "dev_reduce.hpp"
#define PLASMA_LUT_SPACE __constant__
#include "plasma_lut.hpp"

namespace dns {
namespace {

constexpr uint32_t VIS_BLOCK = 256;

struct VisArgs {
  const float *gt_color, *est_color, *gt_depth, *est_depth;   // [H,W,3] x 2, [H,W] x 2
  const int32_t *gt_label, *est_label, *label_lut;            // [H,W] x 2, [n_lut] or NULL
  const uint32_t* vmax_bits;                                  // the depth row's vmax (depth_vmax_kernel)
  uint8_t* out;                                               // [3H + 2 gap, 3W + 2 gap, 3]
  uint32_t H, W, gap, n_lut;
  float max_label;
  uint32_t background;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for NaN and +-inf

// plasma(Normalize(0, vmax)(x), bytes=True)'s table index: trunc(fl32(fl32(x / vmax) * 256)), below 0 -> 0, 256 and above -> 255;
// vmax == 0 -> 0 (Normalize returns zeros when vmin == vmax)
__device__ __forceinline__ uint32_t plasma_index(float x, float vmax) {
#pragma clang fp contract(off)
  if (vmax == 0.0f) return 0u;
  const float t = (x / vmax) * 256.0f;
  if (!(t >= 0.0f)) return 0u;
  return t >= 256.0f ? 255u : (uint32_t)t;
}

// trunc(fl32(clip(x, 0, 1) * 255)); a NaN is taken as 0
__device__ __forceinline__ uint8_t colour_byte(float x) {
  const float c = x >= 0.0f ? (x <= 1.0f ? x : 1.0f) : 0.0f;
  return (uint8_t)(c * 255.0f);
}

__device__ __forceinline__ int32_t map_label(const VisArgs& a, int32_t v) {
  return (a.label_lut && v >= 0 && (uint32_t)v < a.n_lut) ? a.label_lut[v] : v;
}

__global__ __launch_bounds__(VIS_BLOCK) void depth_vmax_kernel(const float* __restrict__ depth, uint32_t n, uint32_t* __restrict__ vmax_bits) {
  uint32_t best = 0;
  for (uint32_t i = blockIdx.x * VIS_BLOCK + threadIdx.x; i < n; i += gridDim.x * VIS_BLOCK) {
    const float d = depth[i];
    if (d > 0.0f && finite_f(d)) {
      const uint32_t b = __float_as_uint(d);
      best = b > best ? b : best;
    }
  }
  best = wave_max(best);
  if ((threadIdx.x & (WAVE - 1)) == 0 && best) atomicMax(vmax_bits, best);
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_panels_kernel(const VisArgs a) {
  static_assert(VIS_BLOCK == PLASMA_N, "one thread per table entry stages the plasma table");
  __shared__ uint8_t lut[PLASMA_N * 3];
  lut[3u * threadIdx.x] = plasma_lut[3u * threadIdx.x];
  lut[3u * threadIdx.x + 1u] = plasma_lut[3u * threadIdx.x + 1u];
  lut[3u * threadIdx.x + 2u] = plasma_lut[3u * threadIdx.x + 2u];
  __syncthreads();
  const uint32_t SH = 3u * a.H + 2u * a.gap, SW = 3u * a.W + 2u * a.gap;
  const uint64_t gid = (uint64_t)blockIdx.x * VIS_BLOCK + threadIdx.x;
  if (gid >= (uint64_t)SH * SW) return;
  const uint32_t Y = (uint32_t)(gid / SW), X = (uint32_t)(gid - (uint64_t)Y * SW);
  const uint32_t row = Y / (a.H + a.gap), y = Y - row * (a.H + a.gap);
  const uint32_t col = X / (a.W + a.gap), x = X - col * (a.W + a.gap);
  const uint8_t bg = (uint8_t)a.background;
  uint8_t r = bg, g = bg, b = bg;
  if (y < a.H && x < a.W) {                                    // inside a panel (row, col <= 2 follows from Y < SH, X < SW)
    const size_t p = (size_t)y * a.W + x;
    if (row == 1u) {                                           // colour
      float c[3];
#pragma unroll
      for (uint32_t ch = 0; ch < 3u; ++ch) {
        const float gt = a.gt_color[p * 3u + ch], est = a.est_color[p * 3u + ch];
        c[ch] = col == 0u ? gt : (col == 1u ? est : fabsf(gt - est));
      }
      r = colour_byte(c[0]), g = colour_byte(c[1]), b = colour_byte(c[2]);
    } else {
      float v, vmax;
      if (row == 0u) {                                         // depth
        const float gt = a.gt_depth[p], est = a.est_depth[p];
        v = col == 0u ? gt : (col == 1u ? est : fabsf(gt - est));
        vmax = __uint_as_float(*a.vmax_bits);
      } else {                                                 // label: through the class -> label table, then as numbers
        const int32_t gt = map_label(a, a.gt_label[p]), est = map_label(a, a.est_label[p]);
        const int64_t d = (int64_t)gt - (int64_t)est;
        v = col == 0u ? (float)gt : (col == 1u ? (float)est : (float)(d < 0 ? -d : d));
        vmax = a.max_label;
      }
      if (finite_f(v)) {                                       // a non-finite scalar pixel keeps the background colour
        const uint32_t idx = plasma_index(v, vmax);
        r = lut[3u * idx], g = lut[3u * idx + 1u], b = lut[3u * idx + 2u];
      }
    }
  }
  uint8_t* o = a.out + gid * 3u;
  o[0] = r, o[1] = g, o[2] = b;
}

}  // namespace
}  // namespace dns

using namespace dns;

extern "C" int dns_vis_panels(const float* gt_color, const float* est_color, const float* gt_depth, const float* est_depth,
                              const int32_t* gt_label, const int32_t* est_label, const int32_t* label_lut, uint32_t n_lut, uint32_t H,
                              uint32_t W, float max_label, uint32_t gap, uint32_t background, uint8_t* out, uint32_t* vmax_bits,
                              void* stream) {
  DNS_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "dns_vis_panels: image %u x %u (sides 1..16384)", H, W);
  DNS_REQUIRE(gap <= 4096, "dns_vis_panels: gap %u (must be <= 4096)", gap);
  DNS_REQUIRE(background <= 255, "dns_vis_panels: background %u (a byte)", background);
  DNS_REQUIRE(max_label >= 0.0f && max_label <= 3.402823466e38f, "dns_vis_panels: max_label must be finite and >= 0");
  DNS_REQUIRE(gt_color && est_color && gt_depth && est_depth && gt_label && est_label && out && vmax_bits,
              "dns_vis_panels: NULL argument");
  DNS_REQUIRE(!label_lut || n_lut > 0, "dns_vis_panels: a label table of 0 entries");
  hipStream_t st = (hipStream_t)stream;
  const int rc = fill_words(vmax_bits, 0u, 1, st, "dns_vis_panels");
  if (rc != DNS_OK) return rc;
  const uint32_t n = H * W, rb = (n + VIS_BLOCK - 1) / VIS_BLOCK;
  DNS_LAUNCH(depth_vmax_kernel, dim3(rb < 1024u ? rb : 1024u), dim3(VIS_BLOCK), 0, st, gt_depth, n, vmax_bits);
  VisArgs a;
  a.gt_color = gt_color, a.est_color = est_color, a.gt_depth = gt_depth, a.est_depth = est_depth;
  a.gt_label = gt_label, a.est_label = est_label, a.label_lut = label_lut, a.vmax_bits = vmax_bits, a.out = out;
  a.H = H, a.W = W, a.gap = gap, a.n_lut = label_lut ? n_lut : 0u, a.max_label = max_label, a.background = background;
  const uint64_t pixels = (uint64_t)(3u * H + 2u * gap) * (3u * W + 2u * gap);
  DNS_LAUNCH(vis_panels_kernel, dim3((uint32_t)((pixels + VIS_BLOCK - 1) / VIS_BLOCK)), dim3(VIS_BLOCK), 0, st, a);
  return check_launch("dns_vis_panels");
}
