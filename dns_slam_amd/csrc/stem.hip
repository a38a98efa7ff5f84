// The frozen image stem (reference models/layers.py:56-58,95-98: conv 7x7 stride 2 pad 3, 3 -> 64 channels, batch-norm, ReLU) on
// channels-last images [n,H,W,3] -> channels-last maps [n,h,w,64], the layout dns_feature_gather and dns_kf_pair_rows read.
//
// An implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output element, so an image's map does not
// depend on its batch, its position or the call): M = 32 output pixels of one row, N = 2 x 32 channels, K = (ky, kx, c) padded
// 147 -> 148.  A workgroup of 4 waves owns 8 rows x 32 pixels; its input tile with the halo (21 x 69 x 3 floats) and the packed
// [148][64] weight image sit in LDS (55 KB: two workgroups per CU); a wave holds 2 rows x 64 channels in 64 accumulator registers.
// All geometry is stem_tile.hpp's (checked on the host by tools/stem_tile_check.cpp); f32x16 and the NaN-keeping relu come
// through it from conv_tile.hpp.  A store instruction writes, per half wave,
// the 32 consecutive channels of one pixel: two whole 128-byte lines.  No atomics.
//
// Batch statistics (nn.BatchNorm2d in train mode, which is what the reference's never-eval()-ed stem computes): the forward kernel
// leaves one row of float64 sums of conv and conv^2 per workgroup and channel, taken from the fp32 conv values; stem_reduce_kernel
// and stem_finish_kernel add the rows in index order and form s = gamma / sqrt(var + eps), t = beta - mean s in float64; then the
// maps are normalised in place (stem_normalise_kernel) or the convolution runs again with the epilogue.
#include "common.hpp"
#include "stem_tile.hpp"

namespace dns {
namespace {
using namespace stem;

template <bool STATS, bool EPI, bool STORE>
__global__ __launch_bounds__(THREADS, 2) void stem_fwd_kernel(const float* __restrict__ images, int H, int W,
                                                              const float* __restrict__ wpack, const float* __restrict__ st,
                                                              float* __restrict__ out, double* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Tile t = tile_of(blockIdx.x, H, W);
  const int h = out_extent(H), w = out_extent(W);
  const float* __restrict__ im = images + (size_t)t.img * H * W * CIN;

  // Staging: every load of the thread is issued before the first is waited for (a loop of load -> LDS store pays one memory round
  // trip per iteration: 27 of them).  A zero pad, or an item past the end, loads element 0 -- always there -- and drops it.
  constexpr int W_VECS = LDS_W_FLOATS / 4, W_ITERS = (W_VECS + THREADS - 1) / THREADS;
  constexpr int IN_ITERS = (STAGE_ITEMS + THREADS - 1) / THREADS;
  float4 wv[W_ITERS];
  float xv[IN_ITERS];
#pragma unroll
  for (int j = 0; j < W_ITERS; ++j) {
    const int i = tid + j * THREADS;
    wv[j] = reinterpret_cast<const float4*>(wpack)[i < W_VECS ? i : 0];
  }
#pragma unroll
  for (int j = 0; j < IN_ITERS; ++j) {
    const int i = tid + j * THREADS;
    const int64_t s = i < STAGE_ITEMS ? stage_src(t, i, H, W) : -1;
    const float v = im[s >= 0 ? s : 0];
    xv[j] = s >= 0 ? v : 0.f;
  }
  float* tin = lds + LDS_IN_OFF;
#pragma unroll
  for (int j = 0; j < W_ITERS; ++j) {
    const int i = tid + j * THREADS;
    if (i < W_VECS) reinterpret_cast<float4*>(lds + LDS_W_OFF)[i] = wv[j];
  }
#pragma unroll
  for (int j = 0; j < IN_ITERS; ++j) {
    const int i = tid + j * THREADS;
    if (i < STAGE_ITEMS) tin[stage_lds(i)] = xv[j];
  }
  __syncthreads();

  const int hk = lane >> 5;
  int base[ROWS_PER_WAVE];
#pragma unroll
  for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) base[mt] = pixel_base(row_of(wave, mt), lane & 31);
  const float* wl = lds + LDS_W_OFF + (lane & 31);
  f32x16 acc[ROWS_PER_WAVE][2];
#pragma unroll
  for (int mt = 0; mt < ROWS_PER_WAVE; ++mt)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nb][r] = 0.f;

  // the operands of step s (k = 2 s + hk): k = 147 is a zero weight row, and its A operand is the constant 0
  auto operands = [&](int s, float* a, float* b) {
    const int k = 2 * s + hk;
    const bool real = k < K_REAL;
    const int ko = real ? k_offset(k) : 0;
#pragma unroll
    for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) {
      const float v = tin[base[mt] + ko];
      a[mt] = real ? v : 0.f;
    }
    b[0] = wl[k * COUT];
    b[1] = wl[k * COUT + 32];
  };
  // fully unrolled, the next step's LDS reads issued ahead of this step's four matrix instructions
  float a_cur[ROWS_PER_WAVE], b_cur[2];
  operands(0, a_cur, b_cur);
#pragma unroll
  for (int s = 0; s < K_PAD / 2; ++s) {
    float a_nxt[ROWS_PER_WAVE] = {0.f, 0.f}, b_nxt[2] = {0.f, 0.f};
    if (s + 1 < K_PAD / 2) operands(s + 1, a_nxt, b_nxt);
#pragma unroll
    for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) {
      acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[mt], b_cur[0], acc[mt][0], 0, 0, 0);
      acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[mt], b_cur[1], acc[mt][1], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) a_cur[mt] = a_nxt[mt];
    b_cur[0] = b_nxt[0];
    b_cur[1] = b_nxt[1];
  }

  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int ch = acc_channel(lane) + 32 * nb;
    float sc = 1.f, sh = 0.f;
    if (EPI) {
      sc = st[ch];
      sh = st[COUT + ch];
    }
#pragma unroll
    for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) {
      const int oy = t.oy0 + row_of(wave, mt);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ox = t.ox0 + acc_pixel(r, lane);
        if (oy < h && ox < w) {
          const float v = acc[mt][nb][r];
          if (STATS) {
            s1[nb] += (double)v;
            s2[nb] += (double)v * (double)v;
          }
          if (STORE) out[(((size_t)t.img * h + oy) * w + ox) * COUT + ch] = EPI ? relu(fmaf(v, sc, sh)) : v;
        }
      }
    }
  }

  if (STATS) {
    // one row per workgroup: lanes l and l + 32 of the 4 waves hold the same channel; added in (wave, half) order
    double* red = reinterpret_cast<double*>(lds + LDS_IN_OFF);
    __syncthreads();                                 // every wave is done with the input tile
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      red[(wave * 64 + lane) * 4 + nb * 2 + 0] = s1[nb];
      red[(wave * 64 + lane) * 4 + nb * 2 + 1] = s2[nb];
    }
    __syncthreads();
    if (tid < 2 * COUT) {
      const int ch = tid & 63, q = tid >> 6;
      double tot = 0.0;
      for (int wv = 0; wv < WAVES; ++wv)
        for (int half = 0; half < 2; ++half) tot += red[(wv * 64 + half * 32 + (ch & 31)) * 4 + (ch >> 5) * 2 + q];
      partials[(size_t)blockIdx.x * (2 * COUT) + q * COUT + ch] = tot;
    }
  }
}

// rows [b * chunk, (b + 1) * chunk) of the [rows][2 * COUT] partial sums -> row b of `out`, in index order
__global__ __launch_bounds__(2 * COUT) void stem_reduce_kernel(const double* __restrict__ partials, uint64_t rows, uint32_t chunk,
                                                               double* __restrict__ out) {
  const uint64_t r0 = (uint64_t)blockIdx.x * chunk;
  const uint64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
  double tot = 0.0;
  for (uint64_t r = r0; r < r1; ++r) tot += partials[r * (2 * COUT) + threadIdx.x];
  out[(size_t)blockIdx.x * (2 * COUT) + threadIdx.x] = tot;
}

// the level-1 rows in index order -> s_c = gamma / sqrt(var + eps), t_c = beta - mean s_c (biased variance over `count` values)
__global__ __launch_bounds__(COUT) void stem_finish_kernel(const double* __restrict__ level1, uint32_t rows, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           double eps, float* __restrict__ st) {
  const int c = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (uint32_t r = 0; r < rows; ++r) {
    a += level1[(size_t)r * (2 * COUT) + c];
    b += level1[(size_t)r * (2 * COUT) + COUT + c];
  }
  const double mean = a / count;
  double var = b / count - mean * mean;
  var = var < 0.0 ? 0.0 : var;                       // (a NaN stays one)
  const double s = (double)gamma[c] / sqrt(var + eps);
  st[c] = (float)s;
  st[COUT + c] = (float)((double)beta[c] - mean * s);
}

// y = relu(fma(conv, s_c, t_c)) in place over [n_pixels][COUT]; the grid stride is a multiple of 16 float4, so a thread keeps
// its four channels
__global__ __launch_bounds__(256) void stem_normalise_kernel(float* __restrict__ out, uint64_t n_vec, const float* __restrict__ st) {
  const int c0 = (threadIdx.x & 15) * 4;
  float sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sc[j] = st[c0 + j];
    sh[j] = st[COUT + c0 + j];
  }
  float4* o = reinterpret_cast<float4*>(out);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (uint64_t)gridDim.x * 256) {
    float4 v = o[i];
    v.x = relu(fmaf(v.x, sc[0], sh[0]));
    v.y = relu(fmaf(v.y, sc[1], sh[1]));
    v.z = relu(fmaf(v.z, sc[2], sh[2]));
    v.w = relu(fmaf(v.w, sc[3], sh[3]));
    o[i] = v;
  }
}

bool shape_ok(uint32_t n, uint32_t H, uint32_t W) {
  if (n < 1 || H < 1 || W < 1 || H > 32768 || W > 32768) return false;
  const uint64_t g = grid_size(n, (int)H, (int)W);
  return g >= 1 && g < (1ull << 31);
}
}  // namespace
}  // namespace dns

extern "C" uint64_t dns_stem_partial_rows(uint32_t n, uint32_t H, uint32_t W) {
  return dns::shape_ok(n, H, W) ? dns::stem::partial_rows(n, (int)H, (int)W) : 0;
}

extern "C" int dns_stem_forward(const float* images, uint32_t n, uint32_t H, uint32_t W, const float* wpack, const float* st,
                                float* out, uint32_t flags, double* partials, void* stream) {
  using namespace dns;
  using namespace dns::stem;
  DNS_REQUIRE(shape_ok(n, H, W), "dns_stem_forward: n %u, H %u, W %u out of range", n, H, W);
  DNS_REQUIRE(images != nullptr && wpack != nullptr, "dns_stem_forward: NULL images or weight image");
  DNS_REQUIRE(((uintptr_t)wpack & 15) == 0, "dns_stem_forward: the weight image must be 16-byte aligned");
  const bool stats = flags & DNS_STEM_STATS, epi = flags & DNS_STEM_EPILOGUE, store = flags & DNS_STEM_STORE;
  DNS_REQUIRE((flags & ~7u) == 0 && stats != epi && (stats || store),
              "dns_stem_forward: flags %#x are none of STORE | EPILOGUE, STATS | STORE, STATS", flags);
  DNS_REQUIRE(!store || (out != nullptr && ((uintptr_t)out & 127) == 0), "dns_stem_forward: out must be 128-byte aligned");
  DNS_REQUIRE(!epi || st != nullptr, "dns_stem_forward: the epilogue needs st");
  DNS_REQUIRE(!stats || partials != nullptr, "dns_stem_forward: the statistics need the partial rows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_stem_forward");
  if (rc != DNS_OK) return rc;
  const dim3 grid((uint32_t)grid_size(n, (int)H, (int)W)), block(THREADS);
  if (epi) DNS_LAUNCH((stem_fwd_kernel<false, true, true>), grid, block, 0, s, images, (int)H, (int)W, wpack, st, out, partials);
  else if (stats && store) DNS_LAUNCH((stem_fwd_kernel<true, false, true>), grid, block, 0, s, images, (int)H, (int)W, wpack, st, out, partials);
  else DNS_LAUNCH((stem_fwd_kernel<true, false, false>), grid, block, 0, s, images, (int)H, (int)W, wpack, st, out, partials);
  return check_launch("dns_stem_forward");
}

extern "C" int dns_stem_batch_stats(const double* partials, uint32_t n, uint32_t H, uint32_t W, const float* gamma, const float* beta,
                                    double eps, double* level1, float* st, void* stream) {
  using namespace dns;
  using namespace dns::stem;
  DNS_REQUIRE(shape_ok(n, H, W), "dns_stem_batch_stats: n %u, H %u, W %u out of range", n, H, W);
  DNS_REQUIRE(partials && gamma && beta && level1 && st, "dns_stem_batch_stats: NULL argument");
  const uint64_t count = (uint64_t)n * out_extent((int)H) * out_extent((int)W);
  DNS_REQUIRE(count > 1, "dns_stem_batch_stats: batch statistics need more than one value per channel");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_stem_batch_stats");
  if (rc != DNS_OK) return rc;
  const uint64_t rows = partial_rows(n, (int)H, (int)W);
  const uint32_t chunk = reduce_chunk(rows), r1 = reduce_rows(rows);
  DNS_LAUNCH(stem_reduce_kernel, dim3(r1), dim3(2 * COUT), 0, s, partials, rows, chunk, level1);
  DNS_LAUNCH(stem_finish_kernel, dim3(1), dim3(COUT), 0, s, (const double*)level1, r1, (double)count, gamma, beta, eps, st);
  return check_launch("dns_stem_batch_stats");
}

extern "C" int dns_stem_normalise(float* out, uint64_t n_pixels, const float* st, void* stream) {
  using namespace dns;
  DNS_REQUIRE(out != nullptr && st != nullptr && ((uintptr_t)out & 15) == 0, "dns_stem_normalise: NULL or unaligned argument");
  if (n_pixels == 0) return DNS_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_stem_normalise");
  if (rc != DNS_OK) return rc;
  const uint64_t n_vec = n_pixels * (stem::COUT / 4);
  const uint64_t want = (n_vec + 255) / 256;
  const uint32_t blocks = (uint32_t)(want < 4096 ? want : 4096);
  DNS_LAUNCH(stem_normalise_kernel, dim3(blocks), dim3(256), 0, s, out, n_vec, st);
  return check_launch("dns_stem_normalise");
}
