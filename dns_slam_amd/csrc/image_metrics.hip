// 2-D evaluation metrics (eval_2d.py of the reference; include/dns_hip.h, ABI v17): MS-SSIM + masked MSE of F image pairs as one
// fixed launch sequence, and the confusion matrices of F label-image pairs.
//
// MS-SSIM, per level l = 0..4 (sizes h_l x w_l, level 0 = the caller's images, levels 1..4 pooled into the workspace):
//   ms_level_kernel   grid (tiles_x, tiles_y, F), 256 threads, one tile of MS_TH x MS_TW output pixels of the valid 11-tap
//                     convolution.  The workgroup stages the (MS_TH+10) x (MS_TW+10) x 3 patch of X and of Y in LDS (one coalesced
//                     read of the interleaved [h,w,3] rows), then per channel: the horizontal pass of the five quantities X, Y,
//                     XX, YY, XY into LDS (float64), the vertical pass in registers, cs and ssim of each output pixel, and at the
//                     end ONE row of six float64 sums (cs, ssim per channel) per workgroup.  No filtered map goes to memory.
//   ms_pool_kernel    the 2x2 average pool (zero padding of size % 2, divisor 4) of X and Y into the next level; the launch that
//                     reads level 0 also sums the squared differences of the pixels with depth > 0 (one row per workgroup).
//   ms_final_kernel   grid F: adds the rows of each level in a fixed order in float64, forms the means, relu, powers, product, and
//                     the MSE.
// 5 + 4 + 1 = 10 launches for any F.  Every sum is a fixed tree: the outputs are the same bits for every call.
//
// Arithmetic: the window is eleven fp32 constants (the bits pytorch_msssim's fp32 window has); everything after the fp32 pixels
// (and the fp32 pooled pixels) is float64 -- products of two fp32 values are exact in float64, so G*(X X) - (G*X)^2 does not lose the
// digits an fp32 evaluation loses to cancellation (1.5e-5 on constant images).  gfx950 runs float64 FMAs at half the fp32 rate and
// the kernels are bound by LDS traffic and launch latency, not by the FMAs.
#include "common.hpp"
#include <algorithm>

namespace dns {
namespace {

constexpr int MS_LEVELS = 5;
constexpr int MS_WIN = 11, MS_R = MS_WIN - 1;
constexpr int MS_TH = 32, MS_TW = 16;                        // output pixels per workgroup
constexpr int MS_IH = MS_TH + MS_R, MS_IW = MS_TW + MS_R;    // staged patch: 42 x 26 pixels
constexpr int MS_BLOCK = 256;
constexpr int MS_PITCH = MS_IW * 3;                          // floats per staged row (channels interleaved)
static_assert(MS_TW * (MS_TH / 2) == MS_BLOCK, "vertical pass: one column and two rows (r, r + MS_TH/2) per thread");
// LDS: 2 x 42 x 78 x 4 = 26208 B (X, Y patches) + 5 x 42 x 16 x 8 = 26880 B (horizontal pass) = 53088 B: three workgroups per CU
static_assert(2 * MS_IH * MS_PITCH * 4 + 5 * MS_IH * MS_TW * 8 <= 64 * 1024, "static LDS");
static_assert(6 * MS_BLOCK <= 5 * MS_IH * MS_TW, "the block reduction reuses the horizontal-pass buffer");

// exp(-(k-5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1, in fp32: the bits of pytorch_msssim's _fspecial_gauss_1d(11, 1.5)
// (tests/test_image_metrics_ref.py compares them with torch's evaluation of that expression)
constexpr float MS_WINDOW[MS_WIN] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                     0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};
constexpr double MS_WEIGHTS[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
constexpr double MS_C1 = 0.01 * 0.01, MS_C2 = 0.03 * 0.03;

struct MsWindow {
  double g[MS_WIN];
};

struct MsDims {
  uint32_t h[MS_LEVELS], w[MS_LEVELS];         // level sizes
  uint32_t tiles[MS_LEVELS];                   // workgroups (rows of partial sums) of ms_level_kernel per frame
  uint32_t pool_blocks;                        // workgroups of the level 0 -> 1 pool per frame (rows of the MSE partials)
};

inline uint32_t pooled(uint32_t s) { return (s + 2 * (s % 2) - 2) / 2 + 1; }

inline MsDims ms_dims(uint32_t H, uint32_t W) {
  MsDims d;
  d.h[0] = H, d.w[0] = W;
  for (int l = 0; l < MS_LEVELS; ++l) {
    if (l) d.h[l] = pooled(d.h[l - 1]), d.w[l] = pooled(d.w[l - 1]);
    d.tiles[l] = ((d.h[l] - MS_R + MS_TH - 1) / MS_TH) * ((d.w[l] - MS_R + MS_TW - 1) / MS_TW);
  }
  d.pool_blocks = (uint32_t)(((uint64_t)d.h[1] * d.w[1] + MS_BLOCK - 1) / MS_BLOCK);
  return d;
}

// workspace: [float64 level partials: sum_l F tiles_l 6][float64 MSE partials: F pool_blocks 2][fp32 X, Y of levels 1..4]
struct MsWs {
  double* part[MS_LEVELS];
  double* mse_part;
  float* x[MS_LEVELS];
  float* y[MS_LEVELS];
};

inline uint64_t ms_layout(void* ws, uint32_t F, const MsDims& d, MsWs* out) {
  uint64_t off = 0;
  char* base = (char*)ws;
  for (int l = 0; l < MS_LEVELS; ++l) {
    if (out) out->part[l] = (double*)(base + off);
    off += (uint64_t)F * d.tiles[l] * 6 * sizeof(double);
  }
  if (out) out->mse_part = (double*)(base + off);
  off += (uint64_t)F * d.pool_blocks * 2 * sizeof(double);
  for (int l = 1; l < MS_LEVELS; ++l) {
    const uint64_t n = (uint64_t)F * d.h[l] * d.w[l] * 3 * sizeof(float);
    if (out) out->x[l] = (float*)(base + off);
    off += n;
    if (out) out->y[l] = (float*)(base + off);
    off += n;
  }
  return off;
}

// sums v[0..N) over the workgroup in a fixed tree; the totals are valid in thread 0.  red: N * MS_BLOCK doubles of LDS.
template <int N>
__device__ inline void block_sum(double* v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) red[q * MS_BLOCK + t] = v[q];
  for (int s = MS_BLOCK / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
#pragma unroll
      for (int q = 0; q < N; ++q) red[q * MS_BLOCK + t] += red[q * MS_BLOCK + t + s];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = red[q * MS_BLOCK];
}

__global__ __launch_bounds__(MS_BLOCK) void ms_level_kernel(const float* __restrict__ X, const float* __restrict__ Y, uint32_t h,
                                                            uint32_t w, MsWindow win, double* __restrict__ part) {
  __shared__ float sx[MS_IH * MS_PITCH];
  __shared__ float sy[MS_IH * MS_PITCH];
  __shared__ double hb[5 * MS_IH * MS_TW];
  const int t = threadIdx.x;
  const uint32_t r0 = blockIdx.y * MS_TH, c0 = blockIdx.x * MS_TW;      // first output (= first input) row / column of the tile
  const uint32_t oh = h - MS_R, ow = w - MS_R;
  const size_t frame = (size_t)blockIdx.z * h * w * 3;
  // stage the patch: rows r0 .. r0+41, columns c0 .. c0+25, zeros beyond the image (those feed masked outputs only)
  const uint32_t rows_in = min((uint32_t)MS_IH, h - r0), cols_in = min((uint32_t)MS_IW, w - c0);
  for (int i = t; i < MS_IH * MS_PITCH; i += MS_BLOCK) {
    const uint32_t r = i / MS_PITCH, e = i % MS_PITCH;
    float a = 0.f, b = 0.f;
    if (r < rows_in && e < cols_in * 3) {
      const size_t g = frame + ((size_t)(r0 + r) * w + c0) * 3 + e;
      a = X[g], b = Y[g];
    }
    sx[i] = a, sy[i] = b;
  }
  const int vj = t % MS_TW, vr = t / MS_TW;                            // vertical pass: column vj, rows vr and vr + 16
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                      // cs[3], ssim[3]
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                                   // patch staged / previous channel's vertical pass done
    for (int i = t; i < MS_IH * MS_TW; i += MS_BLOCK) {
      const int r = i / MS_TW, j = i % MS_TW;
      const float* px = sx + r * MS_PITCH + j * 3 + c;
      const float* py = sy + r * MS_PITCH + j * 3 + c;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
      for (int k = 0; k < MS_WIN; ++k) {
        const double x = (double)px[3 * k], y = (double)py[3 * k], g = win.g[k];
        a0 += g * x, a1 += g * y, a2 += g * (x * x), a3 += g * (y * y), a4 += g * (x * y);
      }
      hb[0 * MS_IH * MS_TW + i] = a0, hb[1 * MS_IH * MS_TW + i] = a1, hb[2 * MS_IH * MS_TW + i] = a2;
      hb[3 * MS_IH * MS_TW + i] = a3, hb[4 * MS_IH * MS_TW + i] = a4;
    }
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = vr + half * (MS_TH / 2);
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MS_WIN; ++k) {
        const double g = win.g[k];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] += g * hb[q * MS_IH * MS_TW + (r + k) * MS_TW + vj];
      }
      if (r0 + r < oh && c0 + vj < ow) {
        const double mx = v[0], my = v[1];
        const double sxx = v[2] - mx * mx, syy = v[3] - my * my, sxy = v[4] - mx * my;
        const double cs = (2.0 * sxy + MS_C2) / (sxx + syy + MS_C2);
        acc[c] += cs;
        acc[3 + c] += (2.0 * mx * my + MS_C1) / (mx * mx + my * my + MS_C1) * cs;
      }
    }
  }
  block_sum<6>(acc, hb);
  if (t == 0) {
    double* row = part + ((size_t)blockIdx.z * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
#pragma unroll
    for (int q = 0; q < 6; ++q) row[q] = acc[q];
  }
}

// one pooled pixel per thread; grid (blocks, F).  MSE: every source pixel lies in exactly one 2x2 window, so the same threads
// also sum the squared fp32 differences of the pixels with depth > 0 (all pixels without depth).
template <bool MSE>
__global__ __launch_bounds__(MS_BLOCK) void ms_pool_kernel(const float* __restrict__ X, const float* __restrict__ Y, uint32_t h, uint32_t w,
                                                           uint32_t h2, uint32_t w2, float* __restrict__ X2, float* __restrict__ Y2,
                                                           const float* __restrict__ depth, double* __restrict__ mse_part) {
  __shared__ double red[2 * MS_BLOCK];
  const uint32_t f = blockIdx.y;
  const uint64_t o = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  const int ph = h % 2, pw = w % 2;
  double v[2] = {0.0, 0.0};                                            // sum of squared differences, number of valid pixels
  if (o < (uint64_t)h2 * w2) {
    const uint32_t i = (uint32_t)(o / w2), j = (uint32_t)(o % w2);
    float ax[3] = {0.f, 0.f, 0.f}, ay[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int di = 0; di < 2; ++di) {
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const int64_t r = 2 * (int64_t)i - ph + di, c = 2 * (int64_t)j - pw + dj;
        if (r < 0 || c < 0 || r >= (int64_t)h || c >= (int64_t)w) continue;       // zero padding
        const size_t px = (size_t)f * h * w + (size_t)r * w + (size_t)c;
        bool valid = true;
        if (MSE && depth) valid = depth[px] > 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float x = X[px * 3 + ch], y = Y[px * 3 + ch];
          ax[ch] += x, ay[ch] += y;
          if (MSE && valid) {
            const double d = (double)(x - y);
            v[0] += d * d;
          }
        }
        if (MSE && valid) v[1] += 1.0;
      }
    }
    const size_t q = ((size_t)f * h2 * w2 + (size_t)o) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) X2[q + ch] = ax[ch] * 0.25f, Y2[q + ch] = ay[ch] * 0.25f;
  }
  if (MSE) {
    block_sum<2>(v, red);
    if (threadIdx.x == 0) {
      double* row = mse_part + ((size_t)f * gridDim.x + blockIdx.x) * 2;
      row[0] = v[0], row[1] = v[1];
    }
  }
}

struct MsFinalArgs {
  const double* part[MS_LEVELS];
  uint32_t tiles[MS_LEVELS];
  double n_out[MS_LEVELS];                     // output pixels of the level's valid convolution
  const double* mse_part;
  uint32_t pool_blocks;
};

__global__ __launch_bounds__(MS_BLOCK) void ms_final_kernel(MsFinalArgs a, double* __restrict__ ms_ssim, double* __restrict__ mse,
                                                            int64_t* __restrict__ n_valid, double* __restrict__ levels) {
  __shared__ double red[6 * MS_BLOCK];
  const uint32_t f = blockIdx.x;
  const int t = threadIdx.x;
  double prod[3] = {1.0, 1.0, 1.0};
  for (int l = 0; l < MS_LEVELS; ++l) {
    const double* p = a.part[l] + (size_t)f * a.tiles[l] * 6;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = t; i < a.tiles[l]; i += MS_BLOCK) {
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] += p[(size_t)i * 6 + q];
    }
    block_sum<6>(v, red);
    if (t == 0) {
      for (int c = 0; c < 3; ++c) {
        const double term = (l < MS_LEVELS - 1 ? v[c] : v[3 + c]) / a.n_out[l];
        levels[((size_t)f * MS_LEVELS + l) * 3 + c] = term;
        prod[c] *= pow(term > 0.0 ? term : 0.0, MS_WEIGHTS[l]);
      }
    }
  }
  double m[2] = {0.0, 0.0};
  const double* p = a.mse_part + (size_t)f * a.pool_blocks * 2;
  for (uint32_t i = t; i < a.pool_blocks; i += MS_BLOCK) m[0] += p[(size_t)i * 2], m[1] += p[(size_t)i * 2 + 1];
  block_sum<2>(m, red);
  if (t == 0) {
    ms_ssim[f] = (prod[0] + prod[1] + prod[2]) / 3.0;
    mse[f] = m[0] / (3.0 * m[1]);                                      // no valid pixel: 0 / 0 = NaN, as an empty mse_loss
    n_valid[f] = (int64_t)m[1];
  }
}

// ---- confusion matrices ------------------------------------------------------------------------------------------------------
constexpr int CF_BLOCK = 256, CF_PER_THREAD = 16;
constexpr uint32_t CF_CHUNK = CF_BLOCK * CF_PER_THREAD;               // pixels per workgroup: a 32-bit LDS counter cannot overflow
static_assert(DNS_CONFUSION_LDS_CLASSES * DNS_CONFUSION_LDS_CLASSES * 4 <= 16 * 1024, "LDS histogram budget: 16 KiB per workgroup");

template <bool LDS>
__global__ __launch_bounds__(CF_BLOCK) void confusion_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, uint64_t N,
                                                             uint32_t nc, unsigned long long* __restrict__ conf,
                                                             unsigned long long* __restrict__ n_invalid) {
  __shared__ uint32_t hist[LDS ? DNS_CONFUSION_LDS_CLASSES * DNS_CONFUSION_LDS_CLASSES : 1];
  __shared__ uint32_t bad;
  const uint32_t f = blockIdx.y;
  const uint32_t cells = nc * nc;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < cells; i += CF_BLOCK) hist[i] = 0;
  }
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const uint64_t start = (uint64_t)blockIdx.x * CF_CHUNK;
  const uint64_t end = min(start + CF_CHUNK, N);
  unsigned long long* cf = conf + (size_t)f * cells;
  uint32_t my_bad = 0;
  for (uint64_t i = start + threadIdx.x; i < end; i += CF_BLOCK) {
    const int32_t g = gt[(size_t)f * N + i], p = pred[(size_t)f * N + i];
    if ((uint32_t)g >= nc || (uint32_t)p >= nc) {
      ++my_bad;
      continue;
    }
    const uint32_t cell = (uint32_t)g * nc + (uint32_t)p;
    if (LDS) atomicAdd(&hist[cell], 1u);
    else atomicAdd(&cf[cell], 1ull);
  }
  if (my_bad) atomicAdd(&bad, my_bad);
  __syncthreads();
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < cells; i += CF_BLOCK) {
      const uint32_t n = hist[i];
      if (n) atomicAdd(&cf[i], (unsigned long long)n);
    }
  }
  if (threadIdx.x == 0 && bad) atomicAdd(&n_invalid[f], (unsigned long long)bad);
}

}  // namespace
}  // namespace dns

using namespace dns;

extern "C" void dns_ms_ssim_window(float* window) {
  for (int k = 0; k < MS_WIN; ++k) window[k] = MS_WINDOW[k];
}

static bool ms_size_ok(uint32_t F, uint32_t H, uint32_t W) {
  return F > 0 && F <= 65535u && std::min(H, W) > DNS_MS_SSIM_MIN_SIDE && H <= (1u << 15) && W <= (1u << 15);
}

extern "C" uint64_t dns_ms_ssim_ws_bytes(uint32_t F, uint32_t H, uint32_t W) {
  if (!ms_size_ok(F, H, W)) return 0;
  return ms_layout(nullptr, F, ms_dims(H, W), nullptr);
}

extern "C" int dns_ms_ssim(const float* pred, const float* gt, const float* depth, uint32_t F, uint32_t H, uint32_t W, void* ws,
                           double* ms_ssim, double* mse, int64_t* n_valid, double* levels, void* stream) {
  DNS_REQUIRE(std::min(H, W) > DNS_MS_SSIM_MIN_SIDE, "dns_ms_ssim: images of %u x %u: the smaller side must be larger than %u "
              "(four 2x poolings ahead of an 11-tap window)", H, W, DNS_MS_SSIM_MIN_SIDE);
  DNS_REQUIRE(ms_size_ok(F, H, W), "dns_ms_ssim: %u frames of %u x %u (1..65535 frames, sides <= 32768)", F, H, W);
  DNS_REQUIRE(pred && gt && ws && ms_ssim && mse && n_valid && levels, "dns_ms_ssim: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const MsDims d = ms_dims(H, W);
  MsWs w;
  ms_layout(ws, F, d, &w);
  MsWindow win;
  for (int k = 0; k < MS_WIN; ++k) win.g[k] = (double)MS_WINDOW[k];
  MsFinalArgs fa;
  const float *x = pred, *y = gt;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const uint32_t oh = d.h[l] - MS_R, ow = d.w[l] - MS_R;
    const dim3 grid((ow + MS_TW - 1) / MS_TW, (oh + MS_TH - 1) / MS_TH, F);
    DNS_LAUNCH(ms_level_kernel, grid, dim3(MS_BLOCK), 0, st, x, y, d.h[l], d.w[l], win, w.part[l]);
    fa.part[l] = w.part[l], fa.tiles[l] = d.tiles[l], fa.n_out[l] = (double)oh * (double)ow;
    if (l == MS_LEVELS - 1) break;
    const uint32_t blocks = (uint32_t)(((uint64_t)d.h[l + 1] * d.w[l + 1] + MS_BLOCK - 1) / MS_BLOCK);
    if (l == 0)
      DNS_LAUNCH(ms_pool_kernel<true>, dim3(blocks, F), dim3(MS_BLOCK), 0, st, x, y, d.h[0], d.w[0], d.h[1], d.w[1], w.x[1], w.y[1],
                 depth, w.mse_part);
    else
      DNS_LAUNCH(ms_pool_kernel<false>, dim3(blocks, F), dim3(MS_BLOCK), 0, st, x, y, d.h[l], d.w[l], d.h[l + 1], d.w[l + 1],
                 w.x[l + 1], w.y[l + 1], (const float*)nullptr, (double*)nullptr);
    x = w.x[l + 1], y = w.y[l + 1];
  }
  fa.mse_part = w.mse_part, fa.pool_blocks = d.pool_blocks;
  DNS_LAUNCH(ms_final_kernel, dim3(F), dim3(MS_BLOCK), 0, st, fa, ms_ssim, mse, n_valid, levels);
  return check_launch("dns_ms_ssim");
}

extern "C" int dns_label_confusion(const int32_t* gt, const int32_t* pred, uint32_t F, uint64_t N, uint32_t n_class, int64_t* conf,
                                   int64_t* n_invalid, void* stream) {
  DNS_REQUIRE(n_class >= 1 && n_class <= DNS_CONFUSION_MAX_CLASSES, "dns_label_confusion: n_class %u (must be 1..%u)", n_class,
              DNS_CONFUSION_MAX_CLASSES);
  DNS_REQUIRE(F <= 65535u, "dns_label_confusion: %u frames (must be <= 65535)", F);
  DNS_REQUIRE(N < ((uint64_t)1 << 31) * CF_CHUNK, "dns_label_confusion: %llu pixels per frame are too many", (unsigned long long)N);
  if (F == 0) return DNS_OK;
  DNS_REQUIRE(conf && n_invalid && (N == 0 || (gt && pred)), "dns_label_confusion: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int rc = fill_words2(conf, 0u, (size_t)F * n_class * n_class * 2, n_invalid, 0u, (size_t)F * 2, st, "dns_label_confusion");
  if (rc != DNS_OK || N == 0) return rc;
  const dim3 grid((uint32_t)((N + CF_CHUNK - 1) / CF_CHUNK), F);
  if (n_class <= DNS_CONFUSION_LDS_CLASSES)
    DNS_LAUNCH(confusion_kernel<true>, grid, dim3(CF_BLOCK), 0, st, gt, pred, N, n_class, (unsigned long long*)conf,
               (unsigned long long*)n_invalid);
  else
    DNS_LAUNCH(confusion_kernel<false>, grid, dim3(CF_BLOCK), 0, st, gt, pred, N, n_class, (unsigned long long*)conf,
               (unsigned long long*)n_invalid);
  return check_launch("dns_label_confusion");
}
