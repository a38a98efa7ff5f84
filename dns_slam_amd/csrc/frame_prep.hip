// Frame preparation (include/dns_hip.h, "frame preparation"): BaseDataset.__getitem__ (datas/slam_datasets.py:85-149) on the raw
// 8/16-bit images of n frames in one launch, and the first occurrences of the label values that cal_class_n's numbering follows.
//
// prepare_frames_kernel: one thread per output pixel (frame = blockIdx.y), a gather of at most 16 colour taps, one depth and one
// label read, through the tables frame_prep_plan.hpp builds on the host.  The order of operations IS the specification, so the unit
// is compiled with -ffp-contract=off (Makefile): every product and every sum below rounds once, to fp32.
//   colour tap:        fl32(u8) / 255.0f               (IEEE division: hipcc's default for fp32 '/' is the correctly rounded one);
//                      a workgroup divides each of the 256 byte values once, into LDS, and a tap is a read of that table
//   cv2 linear:        h = a w0 + b w1 along x for the rows sy, sy + 1; then h0 v0 + h1 v1
//   torch linear:      the same shape on the cv2 stage's results
// An identity stage (equal sizes) is skipped: its weights are (1, 0), and a 1 + b 0 = a for the finite non-negative values here, so
// skipping changes no bit and saves the taps (the Replica case reads one tap, not sixteen).
// Every index read from a table is clamped into its image (umin), so a blob that does not belong to the dims cannot make the kernel
// read outside the images; the tables themselves are sized by the same plan and checked by the entry point.
#include "common.hpp"
#include "frame_prep_plan.hpp"

namespace dns {
namespace {

using namespace fprep;

struct FpArgs {
  const uint8_t* color;
  const uint16_t* depth;
  const void* label;
  const int32_t* lut;
  const int32_t *cv_x_idx, *cv_y_idx, *tb_x_idx, *tb_y_idx, *tn_x, *tn_y, *cn_x, *cn_y;
  const float *cv_x_w, *cv_y_w, *tb_x_w, *tb_y_w;
  uint32_t Hc, Wc, Hd, Wd, Hl, Wl, edge, H, W;
  uint32_t ident, bgr, label_bytes;
  float png_depth_scale, scale;
  float* out_color;
  float* out_depth;
  int64_t* out_label;
};

__device__ __forceinline__ uint32_t clampi(int32_t i, uint32_t n) { return min((uint32_t)max(i, 0), n - 1u); }

// colour channel c of the pixel (y, x) of frame image `img` [Hc,Wc,3] as the reference's float: astype(float32) / 255, read from
// the workgroup's table unit[v] = fl32(v) / 255.0f
__device__ __forceinline__ float tap(const float* unit, const uint8_t* img, uint32_t Wc, uint32_t y, uint32_t x, uint32_t c) {
  return unit[img[((size_t)y * Wc + x) * 3u + c]];
}

// the cv2 stage at (y1, x1) of the depth-sized image
__device__ __forceinline__ float cv_pixel(const FpArgs& a, const float* unit, const uint8_t* img, uint32_t y1, uint32_t x1, uint32_t c) {
  if (a.ident & IDENT_CV) return tap(unit, img, a.Wc, y1, x1, c);
  const uint32_t sx0 = clampi(a.cv_x_idx[x1], a.Wc), sx1 = min(sx0 + 1u, a.Wc - 1u);
  const uint32_t sy0 = clampi(a.cv_y_idx[y1], a.Hc), sy1 = min(sy0 + 1u, a.Hc - 1u);
  const float a0 = a.cv_x_w[2u * x1], a1 = a.cv_x_w[2u * x1 + 1u], b0 = a.cv_y_w[2u * y1], b1 = a.cv_y_w[2u * y1 + 1u];
  const float h0 = tap(unit, img, a.Wc, sy0, sx0, c) * a0 + tap(unit, img, a.Wc, sy0, sx1, c) * a1;
  const float h1 = tap(unit, img, a.Wc, sy1, sx0, c) * a0 + tap(unit, img, a.Wc, sy1, sx1, c) * a1;
  return h0 * b0 + h1 * b1;
}

__global__ __launch_bounds__(FP_BLOCK) void prepare_frames_kernel(const FpArgs a) {
  static_assert(FP_BLOCK == 256, "one thread per byte value fills the table");
  __shared__ float unit[256];
  unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
  const uint32_t pix = blockIdx.x * FP_BLOCK + threadIdx.x;
  if (pix >= a.H * a.W) return;
  const uint32_t f = blockIdx.y;
  const uint32_t y = pix / a.W, x = pix - y * a.W;
  const uint32_t y2 = y + a.edge, x2 = x + a.edge;                 // in the crop_size image
  const size_t out = (size_t)f * a.H * a.W + pix;
  const bool ident_t = (a.ident & IDENT_TORCH) != 0u;

  // depth and label: nearest, from the depth-sized image
  const uint32_t yd = ident_t ? y2 : clampi(a.tn_y[y2], a.Hd), xd = ident_t ? x2 : clampi(a.tn_x[x2], a.Wd);
  const float dv = (float)a.depth[((size_t)f * a.Hd + yd) * a.Wd + xd];
  a.out_depth[out] = (dv / a.png_depth_scale) * a.scale;
  if (a.label_bytes) {
    const bool ident_n = (a.ident & IDENT_CVN) != 0u;
    const uint32_t yl = ident_n ? yd : clampi(a.cn_y[yd], a.Hl), xl = ident_n ? xd : clampi(a.cn_x[xd], a.Wl);
    const size_t at = ((size_t)f * a.Hl + yl) * a.Wl + xl;
    const uint32_t v = a.label_bytes == 1u ? (uint32_t)((const uint8_t*)a.label)[at] : (uint32_t)((const uint16_t*)a.label)[at];
    a.out_label[out] = (int64_t)a.lut[v];
  }

  // colour
  const uint8_t* img = a.color + (size_t)f * a.Hc * a.Wc * 3u;
  float rgb[3];
  if (ident_t) {
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) rgb[c] = cv_pixel(a, unit, img, y2, x2, a.bgr ? 2u - c : c);
  } else {
    const uint32_t x0 = clampi(a.tb_x_idx[x2], a.Wd), x1 = min(x0 + 1u, a.Wd - 1u);
    const uint32_t y0 = clampi(a.tb_y_idx[y2], a.Hd), y1 = min(y0 + 1u, a.Hd - 1u);
    const float wx0 = a.tb_x_w[2u * x2], wx1 = a.tb_x_w[2u * x2 + 1u], wy0 = a.tb_y_w[2u * y2], wy1 = a.tb_y_w[2u * y2 + 1u];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
      const uint32_t cs = a.bgr ? 2u - c : c;
      const float t0 = cv_pixel(a, unit, img, y0, x0, cs) * wx0 + cv_pixel(a, unit, img, y0, x1, cs) * wx1;
      const float t1 = cv_pixel(a, unit, img, y1, x0, cs) * wx0 + cv_pixel(a, unit, img, y1, x1, cs) * wx1;
      rgb[c] = t0 * wy0 + t1 * wy1;
    }
  }
  float* oc = a.out_color + out * 3u;
  oc[0] = rgb[0], oc[1] = rgb[1], oc[2] = rgb[2];
}

// first[v] = min over the pixels i with label[i] == v of i, as an UNSIGNED minimum over words that start at 0xffffffff: a value that
// never occurs keeps 0xffffffff = -1.  Only the first pixel of a run of equal values can be a first occurrence, so only it issues an
// atomic: label images are made of large constant regions.
template <typename T>
__global__ __launch_bounds__(FP_BLOCK) void label_first_seen_kernel(const T* __restrict__ label, uint32_t n, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * FP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = (uint32_t)label[i];
  if (i == 0u || (uint32_t)label[i - 1u] != v) atomicMin(first + v, i);
}

}  // namespace
}  // namespace dns

using namespace dns;
using namespace dns::fprep;

extern "C" uint64_t dns_frame_prep_table_words(const DnsFramePrepDims* d) {
  Plan p;
  return d && make_plan(*d, &p) ? p.words : 0;
}

extern "C" int dns_frame_prep_tables(const DnsFramePrepDims* d, int32_t* words, uint64_t n_words) {
  DNS_REQUIRE(d && words, "dns_frame_prep_tables: NULL argument");
  Plan p;
  DNS_REQUIRE(make_plan(*d, &p), "dns_frame_prep_tables: sizes refused (sides 1..%u, labels with both sides or none, 2 edge < Hs, Ws)",
              MAX_SIDE);
  DNS_REQUIRE(n_words == p.words, "dns_frame_prep_tables: %llu words given, the plan has %llu", (unsigned long long)n_words,
              (unsigned long long)p.words);
  fill_tables(*d, p, words);
  return DNS_OK;
}

extern "C" int dns_prepare_frames(const uint8_t* color, int bgr, const uint16_t* depth, const void* label, int label_bytes,
                                  const int32_t* lut, const DnsFramePrepDims* d, const int32_t* tables, uint64_t table_words, uint32_t n,
                                  float png_depth_scale, float scale, float* out_color, float* out_depth, int64_t* out_label,
                                  void* stream) {
  DNS_REQUIRE(d, "dns_prepare_frames: NULL dims");
  Plan p;
  DNS_REQUIRE(make_plan(*d, &p), "dns_prepare_frames: sizes refused (sides 1..%u, labels with both sides or none, 2 edge < Hs, Ws)",
              MAX_SIDE);
  DNS_REQUIRE(table_words == p.words, "dns_prepare_frames: a table blob of %llu words, the sizes plan %llu",
              (unsigned long long)table_words, (unsigned long long)p.words);
  DNS_REQUIRE(label_bytes == 0 || label_bytes == 1 || label_bytes == 2, "dns_prepare_frames: label_bytes %d (0, 1 or 2)", label_bytes);
  DNS_REQUIRE((label_bytes != 0) == p.labels, "dns_prepare_frames: label_bytes %d with a label image of %u x %u", label_bytes, d->Hl,
              d->Wl);
  DNS_REQUIRE(n <= MAX_FRAMES, "dns_prepare_frames: %u frames (must be <= %u)", n, MAX_FRAMES);
  DNS_REQUIRE(png_depth_scale != 0.0f, "dns_prepare_frames: png_depth_scale 0");
  if (n == 0) return DNS_OK;
  DNS_REQUIRE(color && depth && tables && out_color && out_depth, "dns_prepare_frames: NULL argument");
  DNS_REQUIRE(!p.labels || (label && lut && out_label), "dns_prepare_frames: NULL label argument");
  hipStream_t st = (hipStream_t)stream;
  FpArgs a;
  a.color = color, a.depth = depth, a.label = label, a.lut = lut;
  a.cv_x_idx = tables + p.cv_x_idx, a.cv_y_idx = tables + p.cv_y_idx, a.tb_x_idx = tables + p.tb_x_idx, a.tb_y_idx = tables + p.tb_y_idx;
  a.tn_x = tables + p.tn_x, a.tn_y = tables + p.tn_y, a.cn_x = tables + p.cn_x, a.cn_y = tables + p.cn_y;
  a.cv_x_w = (const float*)(tables + p.cv_x_w), a.cv_y_w = (const float*)(tables + p.cv_y_w);
  a.tb_x_w = (const float*)(tables + p.tb_x_w), a.tb_y_w = (const float*)(tables + p.tb_y_w);
  a.Hc = d->Hc, a.Wc = d->Wc, a.Hd = d->Hd, a.Wd = d->Wd, a.Hl = d->Hl, a.Wl = d->Wl, a.edge = d->edge, a.H = p.H, a.W = p.W;
  a.ident = p.ident, a.bgr = bgr ? 1u : 0u, a.label_bytes = (uint32_t)label_bytes;
  a.png_depth_scale = png_depth_scale, a.scale = scale;
  a.out_color = out_color, a.out_depth = out_depth, a.out_label = out_label;
  DNS_LAUNCH(prepare_frames_kernel, dim3(p.grid_x, n), dim3(FP_BLOCK), 0, st, a);
  return check_launch("dns_prepare_frames");
}

extern "C" int dns_label_first_seen(const void* label, int label_bytes, uint64_t n_pixels, int32_t* first, void* stream) {
  DNS_REQUIRE(label_bytes == 1 || label_bytes == 2, "dns_label_first_seen: label_bytes %d (1 or 2)", label_bytes);
  DNS_REQUIRE(n_pixels < (1ull << 31), "dns_label_first_seen: %llu pixels (must be < 2^31)", (unsigned long long)n_pixels);
  DNS_REQUIRE(first && (n_pixels == 0 || label), "dns_label_first_seen: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int rc = fill_words(first, 0xffffffffu, 65536, st, "dns_label_first_seen");
  if (rc != DNS_OK || n_pixels == 0) return rc;
  const uint32_t n = (uint32_t)n_pixels, blocks = (n + FP_BLOCK - 1) / FP_BLOCK;
  if (label_bytes == 1)
    DNS_LAUNCH(label_first_seen_kernel<uint8_t>, dim3(blocks), dim3(FP_BLOCK), 0, st, (const uint8_t*)label, n, (uint32_t*)first);
  else
    DNS_LAUNCH(label_first_seen_kernel<uint16_t>, dim3(blocks), dim3(FP_BLOCK), 0, st, (const uint16_t*)label, n, (uint32_t*)first);
  return check_launch("dns_label_first_seen");
}
