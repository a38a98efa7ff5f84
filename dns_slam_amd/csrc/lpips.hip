// LPIPS (AlexNet tower + distance head; include/dns_hip.h, ABI v24) on channels-last maps.
//
// conv_cl_kernel   a channels-last convolution + bias + optional ReLU, [n,H,W,Cin] -> [n,h,w,Cout], as an implicit GEMM on
//                  v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output element, so an image's map does not depend
//                  on its batch, its position or the call).  A workgroup of 4 waves owns 8 output rows x 32 pixels x 64 channels; a
//                  wave holds 2 rows x 64 channels in 64 accumulator registers.  K = (ky, channel slice, kx, c) is reduced chunk by
//                  chunk (conv_plan.hpp): per chunk the input rows the tile reads under one ky, CK channels of them, and the matching
//                  [KC_PAD][64] slice of the packed weight image are staged in LDS (at most 60 KB: two workgroups per CU); the
//                  loads of the next chunk are in flight, into registers, while this one is multiplied.  One kernel serves all five AlexNet layers.  DNS_CONV_SCALE_INPUT folds the
//                  LPIPS input scaling into the staging: the zero padding is zero AFTER the scaling.  A store instruction writes,
//                  per half wave, the 32 consecutive channels of one pixel: whole 128-byte lines.  No atomics.
// max_pool_kernel  3x3 stride 2, no padding, floor mode, four channels per thread, keeping a NaN.
// lpips_head_kernel  per pixel of a pair the two channel norms and sum_c lin_c (f_c / (|f| + 1e-10) - g_c / (|g| + 1e-10))^2 in
//                  float64 (the quotient as a product with the reciprocal), a wave per pixel; one float64 partial per workgroup,
//                  added in a fixed order.
// lpips_finish_kernel  adds the partials of each layer in index order, divides by h w, adds the layers.
// All geometry is conv_plan.hpp's (checked on the host by tools/conv_plan_check.cpp); f32x16 and the NaN-keeping relu come
// through it from conv_tile.hpp.
#include "common.hpp"
#include "conv_plan.hpp"

namespace dns {
namespace {
using namespace convp;

typedef float f32x4 __attribute__((ext_vector_type(4)));      // (arrays of HIP's float4 class kept across the chunk loop end up in scratch)

// max that keeps a NaN of either side
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// LPIPS input scaling of channel c: clamp to [0,1] (a NaN fails both comparisons and stays), 2x - 1, (. - shift) / scale
__device__ __forceinline__ float scale_input(float x, int c) {
  const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
  const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
  x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  x = 2.f * x - 1.f;
  return (x - shift) / scale;
}

template <int VEC, bool SCALE>
__global__ __launch_bounds__(THREADS, 2) void conv_cl_kernel(const float* __restrict__ x, const float* __restrict__ wpack,
                                                             const float* __restrict__ bias, float* __restrict__ out, Plan p,
                                                             int do_relu) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Tile t = tile_of(blockIdx.x, p);
  const float* __restrict__ im = x + (size_t)t.img * p.H * p.W * p.Cin;
  float* tin = lds + p.IN_OFF;
  const int hk = lane >> 5, lx = lane & 31;
  int base[ROWS_PER_WAVE];
#pragma unroll
  for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) base[mt] = pixel_base(p, row_of(wave, mt), lx);
  const float* wl = lds + lx;
  f32x16 acc[ROWS_PER_WAVE][2];
#pragma unroll
  for (int mt = 0; mt < ROWS_PER_WAVE; ++mt)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nb][r] = 0.f;

  // Staging.  What of an item does not depend on the chunk is worked out once; the loads of chunk n + 1 are issued before chunk n
  // is multiplied and stay in registers until it is done, so their round trip to memory hides behind the matrix instructions.
  // A zero pad, or an item past the end, loads element 0 -- always there -- and drops it.
  constexpr int IN_ITERS = in_iters(VEC);
  const int w_vecs = p.W_FLOATS / 4;
  Item item[IN_ITERS];
#pragma unroll
  for (int j = 0; j < IN_ITERS; ++j) {
    const int i = tid + j * THREADS;
    item[j] = stage_item(p, t, i < p.stage_items ? i : 0);
    if (i >= p.stage_items) item[j].col = -1, item[j].lds = -1;
  }
  f32x4 wv[W_ITERS];
  float xv[IN_ITERS][VEC];
  uint32_t live = 0;                                 // bit j: item j of the chunk in flight is inside the image
  // (the loaded values are first touched by `store`: a select here would wait for them before the chunk is multiplied)
  auto load = [&](int chunk, int ky, int cs) __attribute__((always_inline)) {
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(wpack + pack_offset(p, t.cb, chunk));
#pragma unroll
    for (int j = 0; j < W_ITERS; ++j) {
      const int i = tid + j * THREADS;
      wv[j] = wsrc[i < w_vecs ? i : 0];
    }
    live = 0;
#pragma unroll
    for (int j = 0; j < IN_ITERS; ++j) {
      const int64_t s = item_src(p, t, item[j], ky, cs);
      live |= (s >= 0 ? 1u : 0u) << j;
      if constexpr (VEC == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(im + (s >= 0 ? s : 0));
        xv[j][0] = q.x, xv[j][1] = q.y, xv[j][2] = q.z, xv[j][3] = q.w;
      } else {
        xv[j][0] = im[s >= 0 ? s : 0];
      }
    }
  };
  auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < W_ITERS; ++j) {
      const int i = tid + j * THREADS;
      if (i < w_vecs) reinterpret_cast<f32x4*>(lds)[i] = wv[j];
    }
#pragma unroll
    for (int j = 0; j < IN_ITERS; ++j) {
      if (item[j].lds >= 0) {
        const bool in = (live >> j) & 1u;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float q = xv[j][e];
          if (SCALE) q = scale_input(q, item[j].r_cv >> 4);
          tin[item[j].lds + e] = in ? q : 0.f;
        }
      }
    }
  };
  int ky = 0, cs = 0;
  load(0, 0, 0);
  for (int chunk = 0; chunk < p.n_chunks; ++chunk) {
    if (chunk) __syncthreads();                      // every wave is done with the previous chunk
    store();
    __syncthreads();
    if (++cs == p.n_cslices) cs = 0, ++ky;
    if (chunk + 1 < p.n_chunks) load(chunk + 1, ky, cs);

    // step s takes k = 2 s + hk of the chunk = (kx, c).  Where CK is even (every VEC = 4 layer) the two k of a step share kx and
    // there is no pad row: kx and c - hk are the same for the whole wave.  Else (the 3-channel image) every lane keeps its own
    // (kx, c); the pad row k = KC is a zero weight row, and its A operand is the constant 0.
    const int steps = p.KC_PAD / 2;
    int kk = hk, kx = 0, c = hk;                     // VEC = 1: per lane
    if (c >= p.CK) c -= p.CK, ++kx;
    int ukx = 0, uc = 0;                             // VEC = 4: wave-uniform
    auto operands = [&](float* a, float* b, int s) __attribute__((always_inline)) {
      if constexpr (VEC == 4) {
        const int ko = k_offset(p, ukx, uc) + hk;
#pragma unroll
        for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) a[mt] = tin[base[mt] + ko];
        b[0] = wl[(2 * s + hk) * NB];
        b[1] = wl[(2 * s + hk) * NB + 32];
        uc += 2;
        if (uc >= p.CK) uc = 0, ++ukx;
      } else {
        const bool real = kk < p.KC;
        const int ko = real ? k_offset(p, kx, c) : 0;
#pragma unroll
        for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) {
          const float v = tin[base[mt] + ko];
          a[mt] = real ? v : 0.f;
        }
        b[0] = wl[kk * NB];
        b[1] = wl[kk * NB + 32];
        kk += 2, c += 2;                               // CK >= 2 wraps once, CK = 1 twice
        if (c >= p.CK) c -= p.CK, ++kx;
        if (c >= p.CK) c -= p.CK, ++kx;
      }
    };
    float a_cur[ROWS_PER_WAVE], b_cur[2];
    operands(a_cur, b_cur, 0);
    for (int s = 0; s < steps; ++s) {
      float a_nxt[ROWS_PER_WAVE] = {0.f, 0.f}, b_nxt[2] = {0.f, 0.f};
      if (s + 1 < steps) operands(a_nxt, b_nxt, s + 1);   // the next step's LDS reads ahead of this step's four matrix instructions
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
  }

#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int ch = (int)t.cb * NB + acc_channel(lane) + 32 * nb;
    const float b = bias ? bias[ch] : 0.f;
#pragma unroll
    for (int mt = 0; mt < ROWS_PER_WAVE; ++mt) {
      const int oy = t.oy0 + row_of(wave, mt);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ox = t.ox0 + acc_pixel(r, lane);
        if (oy < p.h && ox < p.w) {
          const float v = acc[mt][nb][r] + b;
          out[(((size_t)t.img * p.h + oy) * p.w + ox) * p.Cout + ch] = do_relu ? relu(v) : v;
        }
      }
    }
  }
}

// one thread per output pixel and four channels
__global__ __launch_bounds__(256) void max_pool_kernel(const float* __restrict__ x, uint64_t n_items, int h, int w, int C, int ph,
                                                       int pw, float* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const int c4 = C / 4;
  const int cv = (int)(i % c4);
  uint64_t px = i / c4;
  const int ox = (int)(px % pw);
  px /= pw;
  const int oy = (int)(px % ph);
  const uint64_t img = px / ph;
  const float4* src = reinterpret_cast<const float4*>(x) + ((img * h + 2 * oy) * w + 2 * ox) * c4 + cv;
  float4 m = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const float4 v = src[((size_t)dy * w + dx) * c4];
      m.x = nan_max(m.x, v.x), m.y = nan_max(m.y, v.y), m.z = nan_max(m.z, v.z), m.w = nan_max(m.w, v.w);
    }
  reinterpret_cast<float4*>(out)[i] = m;
}

// the sum over the 64 lanes in a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// grid (head_blocks(h w), F): fa, fb [F][hw][C]; a wave takes HEAD_PIXELS / 4 consecutive pixels, HEAD_BATCH at a time (their
// reductions are independent chains), lane l the channels l, l + 64, ...  A lane adds up its own share of the weighted squared
// differences over the wave's pixels; the 64 shares are added once, at the end.  A pixel past the end is read as zeros: 0.
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                         const float* __restrict__ lin, uint64_t hw, int C,
                                                         double* __restrict__ partials) {
  __shared__ double red[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = C / 64;                            // <= HEAD_MAX_C / 64
  constexpr int MAXP = HEAD_MAX_C / 64, PER_WAVE = HEAD_PIXELS / WAVES;
  static_assert(PER_WAVE % HEAD_BATCH == 0, "whole batches");
  double lw[MAXP];
#pragma unroll
  for (int j = 0; j < MAXP; ++j) lw[j] = j < per ? (double)lin[lane + 64 * j] : 0.0;
  const uint64_t p0 = (uint64_t)blockIdx.x * HEAD_PIXELS + (uint64_t)wave * PER_WAVE;
  double dacc = 0.0;
  for (int q0 = 0; q0 < PER_WAVE; q0 += HEAD_BATCH) {
    if (p0 + q0 >= hw) break;                        // wave-uniform
    float a[HEAD_BATCH][MAXP], b[HEAD_BATCH][MAXP];
    double sa[HEAD_BATCH], sb[HEAD_BATCH];
#pragma unroll
    for (int u = 0; u < HEAD_BATCH; ++u) {
      const uint64_t px = p0 + q0 + u;
      const bool in = px < hw;
      const size_t o = ((size_t)blockIdx.y * hw + (in ? px : 0)) * C + lane;
      sa[u] = 0.0, sb[u] = 0.0;
#pragma unroll
      for (int j = 0; j < MAXP; ++j) {
        a[u][j] = (in && j < per) ? fa[o + 64 * j] : 0.f;
        b[u][j] = (in && j < per) ? fb[o + 64 * j] : 0.f;
        sa[u] += (double)a[u][j] * (double)a[u][j], sb[u] += (double)b[u][j] * (double)b[u][j];
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
      for (int u = 0; u < HEAD_BATCH; ++u) sa[u] += __shfl_xor(sa[u], m, 64), sb[u] += __shfl_xor(sb[u], m, 64);
    }
#pragma unroll
    for (int u = 0; u < HEAD_BATCH; ++u) {
      const double ra = 1.0 / (sqrt(sa[u]) + 1e-10), rb = 1.0 / (sqrt(sb[u]) + 1e-10);
#pragma unroll
      for (int j = 0; j < MAXP; ++j) {
        const double e = (double)a[u][j] * ra - (double)b[u][j] * rb;
        dacc += lw[j] * (e * e);
      }
    }
  }
  const double tot = wave_sum(dacc);
  if (lane == 0) red[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct FinishArgs {
  const double* part[LPIPS_LAYERS];
  uint32_t blocks[LPIPS_LAYERS];
  double hw[LPIPS_LAYERS];
  uint32_t n_layers;
};

// grid F, 64 threads: thread l < n_layers adds layer l's partials in index order; thread 0 then adds the layers in order
__global__ __launch_bounds__(64) void lpips_finish_kernel(FinishArgs a, double* __restrict__ lpips, double* __restrict__ layers) {
  __shared__ double d[LPIPS_LAYERS];
  const uint32_t f = blockIdx.x, l = threadIdx.x;
  if (l < a.n_layers) {
    const double* p = a.part[l] + (size_t)f * a.blocks[l];
    double tot = 0.0;
    for (uint32_t i = 0; i < a.blocks[l]; ++i) tot += p[i];
    d[l] = tot / a.hw[l];
    layers[(size_t)f * a.n_layers + l] = d[l];
  }
  __syncthreads();
  if (l == 0) {
    double tot = 0.0;
    for (uint32_t j = 0; j < a.n_layers; ++j) tot += d[j];
    lpips[f] = tot;
  }
}

}  // namespace
}  // namespace dns

using namespace dns;
using namespace dns::convp;

extern "C" int dns_conv_pack_shape(uint32_t Cin, uint32_t Cout, uint32_t ks, uint32_t stride, uint32_t pad, uint32_t* shape) {
  Plan p;
  DNS_REQUIRE(shape != nullptr, "dns_conv_pack_shape: NULL shape");
  // the chunking depends on (Cin, ks, stride) alone; the image size below is the smallest the layer takes
  const int side = (int)ks > (int)pad ? (int)ks : 1;
  DNS_REQUIRE(Cin <= (uint32_t)MAX_CIN && Cout <= (uint32_t)MAX_COUT && ks <= (uint32_t)MAX_KS && stride <= 4 && pad <= (uint32_t)MAX_KS &&
                  make_plan(side, side, (int)Cin, (int)Cout, (int)ks, (int)stride, (int)pad, &p),
              "dns_conv_pack_shape: Cin %u, Cout %u, kernel %u, stride %u, pad %u are refused (Cout a multiple of 64, kernel <= 11, "
              "stride <= 4, pad < kernel, a chunk within 60 KB of LDS)", Cin, Cout, ks, stride, pad);
  shape[0] = p.cout_blocks, shape[1] = (uint32_t)p.n_chunks, shape[2] = (uint32_t)p.KC_PAD, shape[3] = (uint32_t)p.CK;
  return DNS_OK;
}

extern "C" int dns_conv_cl(const float* x, uint32_t n, uint32_t H, uint32_t W, uint32_t Cin, const float* wpack, const float* bias,
                           uint32_t Cout, uint32_t ks, uint32_t stride, uint32_t pad, uint32_t flags, float* out, void* stream) {
  Plan p;
  DNS_REQUIRE(n >= 1 && H <= (uint32_t)MAX_SIDE && W <= (uint32_t)MAX_SIDE && Cin <= (uint32_t)MAX_CIN && Cout <= (uint32_t)MAX_COUT &&
                  ks <= (uint32_t)MAX_KS && stride <= 4 && pad <= (uint32_t)MAX_KS &&
                  make_plan((int)H, (int)W, (int)Cin, (int)Cout, (int)ks, (int)stride, (int)pad, &p),
              "dns_conv_cl: n %u, H %u, W %u, Cin %u, Cout %u, kernel %u, stride %u, pad %u are refused", n, H, W, Cin, Cout, ks,
              stride, pad);
  const uint64_t grid = grid_size(p, n);
  DNS_REQUIRE(grid >= 1 && grid < (1ull << 31), "dns_conv_cl: %llu workgroups are too many for one call", (unsigned long long)grid);
  DNS_REQUIRE((flags & ~(DNS_CONV_RELU | DNS_CONV_SCALE_INPUT)) == 0, "dns_conv_cl: flags %#x", flags);
  const bool scale = flags & DNS_CONV_SCALE_INPUT;
  DNS_REQUIRE(!scale || Cin == 3, "dns_conv_cl: DNS_CONV_SCALE_INPUT is the scaling of a 3-channel image, Cin is %u", Cin);
  DNS_REQUIRE(x != nullptr && wpack != nullptr && out != nullptr, "dns_conv_cl: NULL argument");
  DNS_REQUIRE(((uintptr_t)wpack & 15) == 0 && ((uintptr_t)out & 127) == 0 && (p.vec == 1 || ((uintptr_t)x & 15) == 0),
              "dns_conv_cl: x and wpack must be 16-byte aligned, out 128-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_conv_cl");
  if (rc != DNS_OK) return rc;
  const dim3 g((uint32_t)grid), b(THREADS);
  const int do_relu = (flags & DNS_CONV_RELU) ? 1 : 0;
  if (p.vec == 4) DNS_LAUNCH((conv_cl_kernel<4, false>), g, b, 0, s, x, wpack, bias, out, p, do_relu);
  else if (scale) DNS_LAUNCH((conv_cl_kernel<1, true>), g, b, 0, s, x, wpack, bias, out, p, do_relu);
  else DNS_LAUNCH((conv_cl_kernel<1, false>), g, b, 0, s, x, wpack, bias, out, p, do_relu);
  return check_launch("dns_conv_cl");
}

extern "C" int dns_max_pool_cl(const float* x, uint32_t n, uint32_t h, uint32_t w, uint32_t C, float* out, void* stream) {
  DNS_REQUIRE(n >= 1 && h >= 3 && w >= 3 && h <= (uint32_t)MAX_SIDE && w <= (uint32_t)MAX_SIDE && C >= 4 && C % 4 == 0 &&
                  C <= (uint32_t)MAX_COUT,
              "dns_max_pool_cl: n %u, h %u, w %u, C %u are refused (sides 3..32768, C a multiple of 4)", n, h, w, C);
  DNS_REQUIRE(x != nullptr && out != nullptr && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0,
              "dns_max_pool_cl: NULL or unaligned argument");
  const int ph = pool_extent((int)h), pw = pool_extent((int)w);
  const uint64_t items = (uint64_t)n * ph * pw * (C / 4);
  const uint64_t blocks = (items + 255) / 256;
  DNS_REQUIRE(blocks < (1ull << 31), "dns_max_pool_cl: %llu workgroups are too many for one call", (unsigned long long)blocks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_max_pool_cl");
  if (rc != DNS_OK) return rc;
  DNS_LAUNCH(max_pool_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, x, items, (int)h, (int)w, (int)C, ph, pw, out);
  return check_launch("dns_max_pool_cl");
}

extern "C" uint32_t dns_lpips_head_blocks(uint32_t h, uint32_t w) {
  if (h < 1 || w < 1 || h > (uint32_t)MAX_SIDE || w > (uint32_t)MAX_SIDE) return 0;
  return head_blocks((uint64_t)h * w);
}

extern "C" int dns_lpips_head(const float* fa, const float* fb, const float* lin, uint32_t F, uint32_t h, uint32_t w, uint32_t C,
                              double* partials, void* stream) {
  DNS_REQUIRE(F >= 1 && F <= 65535u && dns_lpips_head_blocks(h, w) != 0 && C >= 64 && C % 64 == 0 && C <= (uint32_t)HEAD_MAX_C,
              "dns_lpips_head: F %u, h %u, w %u, C %u are refused (1..65535 pairs, C a multiple of 64 up to %d)", F, h, w, C, HEAD_MAX_C);
  DNS_REQUIRE(fa && fb && lin && partials, "dns_lpips_head: NULL argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_lpips_head");
  if (rc != DNS_OK) return rc;
  DNS_LAUNCH(lpips_head_kernel, dim3(dns_lpips_head_blocks(h, w), F), dim3(256), 0, s, fa, fb, lin, (uint64_t)h * w, (int)C, partials);
  return check_launch("dns_lpips_head");
}

extern "C" int dns_lpips_finish(const double* const* partials, const uint32_t* h, const uint32_t* w, uint32_t n_layers, uint32_t F,
                                double* lpips, double* layers, void* stream) {
  DNS_REQUIRE(n_layers >= 1 && n_layers <= (uint32_t)LPIPS_LAYERS && F >= 1 && F <= 65535u, "dns_lpips_finish: %u layers, %u pairs",
              n_layers, F);
  DNS_REQUIRE(partials && h && w && lpips && layers, "dns_lpips_finish: NULL argument");
  FinishArgs a;
  a.n_layers = n_layers;
  for (uint32_t l = 0; l < (uint32_t)LPIPS_LAYERS; ++l) a.part[l] = nullptr, a.blocks[l] = 0, a.hw[l] = 1.0;
  for (uint32_t l = 0; l < n_layers; ++l) {
    const uint32_t b = dns_lpips_head_blocks(h[l], w[l]);
    DNS_REQUIRE(b != 0 && partials[l] != nullptr, "dns_lpips_finish: layer %u: %u x %u or NULL partials", l, h[l], w[l]);
    a.part[l] = partials[l], a.blocks[l] = b, a.hw[l] = (double)h[l] * (double)w[l];
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ensure_ready(s, "dns_lpips_finish");
  if (rc != DNS_OK) return rc;
  DNS_LAUNCH(lpips_finish_kernel, dim3(F), dim3(64), 0, s, a, lpips, layers);
  return check_launch("dns_lpips_finish");
}
