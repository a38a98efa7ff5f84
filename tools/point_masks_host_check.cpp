// Host check of the kernels of dns_slam_amd/csrc/mesh_masks.hip under the address and undefined-behaviour sanitizers: the kernel
// source itself is compiled for the host (one std::thread per lane of a workgroup, a barrier for __syncthreads, a barrier per
// wave for the cross-lane operations) and driven through its C entry points over 1500 points x 300 poses (two LDS tiles) with
// exactly-sized buffers, in every mode and with chunk lengths below, at and above the workgroup size, not a multiple of it, and
// beyond P.  Checked against plain loops over a [P,K] table of samples: no access outside a buffer, the chunk maxima (also of
// all-negative samples), the classes, every refusal.  No GPU is involved.  From the repository root:
//
//   mkdir -p /tmp/pm_check && for f in dev_project.hpp dev_reduce.hpp mesh_masks.hip; do \
//     sed -e 's/#include "common.hpp"//' -e 's/extern "C" //' dns_slam_amd/csrc/$f > /tmp/pm_check/$f; done
//   g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       -Wno-unused-value -I/tmp/pm_check tools/point_masks_host_check.cpp -o /tmp/pm_check/check && /tmp/pm_check/check
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float3 { float x, y, z; };
inline float3 make_float3(float a, float b, float c) { return {a, b, c}; }
constexpr int WAVE = 64;
inline thread_local dim3 threadIdx, blockIdx;
inline std::barrier<>* g_bar;
inline std::barrier<>* g_wbar[16];
inline int64_t g_lane[16][WAVE];
inline int g_pred[1024];
inline unsigned g_block;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline int __syncthreads_and(int p) {
  g_pred[threadIdx.x] = p;
  __syncthreads();
  int all = 1;
  for (unsigned t = 0; t < g_block; ++t) all &= g_pred[t] != 0;
  __syncthreads();
  return all;
}
template <class T>
T __shfl_xor(T x, int o) {
  const unsigned w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
  g_lane[w][l] = (int64_t)x;
  g_wbar[w]->arrive_and_wait();
  const T y = (T)g_lane[w][l ^ (unsigned)o];
  g_wbar[w]->arrive_and_wait();
  return y;
}
inline uint64_t __ballot(int p) {
  const unsigned w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
  g_lane[w][l] = p != 0;
  g_wbar[w]->arrive_and_wait();
  uint64_t m = 0;
  for (int i = 0; i < WAVE; ++i) m |= (uint64_t)g_lane[w][i] << i;
  g_wbar[w]->arrive_and_wait();
  return m;
}
inline int atomicMax(int* a, int v) {
  int old = __atomic_load_n(a, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(a, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
using std::max; using std::min;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
typedef void* hipStream_t;
#define DNS_OK 0
#define DNS_E_ARG (-1)
inline int g_refused;
#define DNS_REQUIRE(cond, ...) do { if (!(cond)) { ++g_refused; return DNS_E_ARG; } } while (0)
inline int check_launch(const char*) { return 0; }
inline int fill_words(void* dst, uint32_t value, size_t n, hipStream_t, const char*) {
  for (size_t i = 0; i < n; ++i) ((uint32_t*)dst)[i] = value;
  return 0;
}
template <class F, class... A>
void launch(F kern, dim3 grid, dim3 block, A... args) {
  g_block = block.x;
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bar(block.x);
    g_bar = &bar;
    std::vector<std::unique_ptr<std::barrier<>>> wb;
    for (unsigned w = 0; w < block.x / WAVE; ++w) wb.emplace_back(new std::barrier<>(WAVE)), g_wbar[w] = wb.back().get();
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
      th.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); kern(args...); });
    for (auto& x : th) x.join();
  }
}
#define DNS_LAUNCH(kern, grid, block, lds, st, ...) launch(kern, grid, block, __VA_ARGS__)

#include "mesh_masks.hip"
#include <random>

static const int H = 12, W = 16;
static const float intr[4] = {12.f, 12.f, 7.5f, 5.5f};

// the sample of depth image d at (u, v) in float64: pixel i at coordinate i, zeros outside
static double sample_ref(const float* d, double u, double v) {
  if (!std::isfinite(u) || !std::isfinite(v)) return 0.0;
  const double x0 = std::floor(u), y0 = std::floor(v);
  double s = 0;
  for (int dy = 0; dy < 2; ++dy)
    for (int dx = 0; dx < 2; ++dx) {
      const double x = x0 + dx, y = y0 + dy;
      if (x < 0 || x > W - 1 || y < 0 || y > H - 1) continue;
      s += d[(size_t)y * W + (size_t)x] * (dx ? u - x0 : x0 + 1 - u) * (dy ? v - y0 : y0 + 1 - v);
    }
  return s;
}

int main() {
  std::mt19937 g(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const uint32_t P = 1500, K = 300;
  std::vector<float> pts(3 * P), w2c(16 * K, 0.f), depth((size_t)K * H * W), md(K);
  for (uint32_t p = 0; p < P; ++p) pts[3 * p] = U(g) * 400.f, pts[3 * p + 1] = U(g) * 400.f, pts[3 * p + 2] = U(g) * 3.f;
  for (uint32_t p = 0; p < P; p += 3) pts[3 * p] *= 0.005f, pts[3 * p + 1] *= 0.005f;          // a third of them near the axis
  for (uint32_t k = 0; k < K; ++k) {
    float* m = &w2c[16 * k];
    m[0] = m[5] = m[10] = m[15] = 1.f;
    m[3] = U(g) * 0.3f, m[7] = U(g) * 0.3f, m[11] = -2.5f + U(g) * 0.3f;      // camera looks down -z at the cloud
    md[k] = 0.f;
    for (int i = 0; i < H * W; ++i) {
      float& d = depth[(size_t)k * H * W + i];
      d = k % 7 == 3 ? -1.f - (float)(i % 5) : 2.5f + U(g) * 2.f;             // some images all negative: the key's other branch
      md[k] = std::max(md[k], d);
    }
  }
  // the table every mode is judged by: projection in the kernel's own fp32 expressions (dev_project.hpp), samples in float64
  std::vector<Projected> q((size_t)P * K);
  std::vector<double> ds((size_t)P * K);
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t k = 0; k < K; ++k) {
      q[(size_t)p * K + k] = project(&w2c[16 * k], make_float3(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]), intr[0], intr[1], intr[2],
                                     intr[3], PROJ_EPS_MESHING);
      ds[(size_t)p * K + k] = sample_ref(&depth[(size_t)k * H * W], q[(size_t)p * K + k].u, q[(size_t)p * K + k].v);
    }
  int counts[3] = {0, 0, 0};
  auto run = [&](int mode, uint32_t chunk, uint32_t Kuse) -> int {
    const uint64_t wsb = dns_point_masks_ws_bytes(P, Kuse, mode == 2 ? chunk : 0);
    std::vector<uint8_t> cls(P, 9);
    int32_t* ws = (int32_t*)malloc(std::max<uint64_t>(wsb, 1));
    if (dns_point_masks(pts.data(), P, w2c.data(), Kuse, mode == 1 ? md.data() : nullptr, mode == 2 ? depth.data() : nullptr,
                        mode == 2 ? chunk : 0, H, W, intr, ws, cls.data(), nullptr))
      return printf("mode %d chunk %u refused\n", mode, chunk), 1;
    const uint32_t ch = mode == 2 ? std::min(chunk, P) : P, n_chunks = (P + ch - 1) / ch;
    std::vector<double> mtab;                                              // float64 maxima of the samples per chunk and pose
    if (mode == 2) {
      mtab.assign((size_t)n_chunks * K, -INFINITY);
      for (uint32_t p = 0; p < P; ++p)
        for (uint32_t k = 0; k < Kuse; ++k) mtab[(size_t)(p / ch) * K + k] = std::max(mtab[(size_t)(p / ch) * K + k], ds[(size_t)p * K + k]);
      for (uint32_t c = 0; c < n_chunks; ++c)
        for (uint32_t k = 0; k < Kuse; ++k) {
          const float got = __int_as_float(max_key(ws[(size_t)c * Kuse + k]));
          const double want = mtab[(size_t)c * K + k];
          if (!(std::fabs(got - want) <= 1e-5 * (1 + std::fabs(want)))) return printf("chunk %u pose %u: max %g, want %g\n", c, k, got, want), 1;
        }
    }
    int near = 0, bad = 0;
    for (uint32_t p = 0; p < P; ++p) {
      bool seen = false, fore = false, close = false;
      for (uint32_t k = 0; k < Kuse; ++k) {
        const Projected& a = q[(size_t)p * K + k];
        const bool in = a.u < W && a.u > 0 && a.v < H && a.v > 0 && a.z < 0;
        const bool wide = a.u < W + 1000 && a.u > -1000 && a.v < H + 1000 && a.v > -1000 && a.z < 0;
        const double dz = -(double)a.czw;
        if (mode == 0) seen |= in, fore |= wide;
        if (mode == 1) seen |= in && -a.czw < md[k] * 1.2f, fore |= wide && -a.czw < md[k] * 1.2f;
        if (mode == 2) {
          const double m = mtab[(size_t)(p / ch) * K + k];
          const double s = ds[(size_t)p * K + k];
          seen |= in && dz < s + 0.1 && s - 2.5 < dz;
          fore |= wide && dz < m;
          close |= (in && (std::fabs(dz - s - 0.1) < 1e-4 * (1 + std::fabs(s)) || std::fabs(dz - s + 2.5) < 1e-4 * (1 + std::fabs(s)))) ||
                   (wide && std::fabs(dz - m) < 1e-4 * std::fabs(m));
        }
      }
      const uint8_t want = seen ? 1 : fore ? 2 : 0;
      if (cls[p] > 2) return printf("point %u not written\n", p), 1;
      ++counts[cls[p]];
      if (cls[p] != want) close ? ++near : ++bad;
    }
    free(ws);
    printf("mode %d chunk %u K %u: %d differences at a threshold, %d elsewhere\n", mode, chunk, Kuse, near, bad);
    return bad || near > 3;
  };
  if (run(0, 0, K) || run(1, 0, K) || run(0, 0, 0) || run(1, 0, 7)) return 1;
  for (uint32_t chunk : {300u, 255u, 256u, 257u, 1u << 20, 1499u, 64u}) if (run(2, chunk, K)) return 1;
  if (run(2, 500, 256) || run(2, 500, 257)) return 1;
  printf("classes over all runs: unseen %d seen %d forecast %d\n", counts[0], counts[1], counts[2]);
  if (!counts[0] || !counts[1] || !counts[2]) return 1;
  // refusals
  std::vector<uint8_t> cls(P);
  int32_t ws[4];
  g_refused = 0;
  int n = 0;
  n += dns_point_masks(pts.data(), 1u << 31, w2c.data(), K, nullptr, nullptr, 0, H, W, intr, nullptr, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(pts.data(), P, w2c.data(), K, md.data(), depth.data(), 8, H, W, intr, ws, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(pts.data(), P, w2c.data(), K, nullptr, depth.data(), 0, H, W, intr, ws, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(pts.data(), P, w2c.data(), K, nullptr, nullptr, 8, H, W, intr, ws, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(pts.data(), P, w2c.data(), K, nullptr, nullptr, 0, 0, W, intr, nullptr, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(pts.data(), P, w2c.data(), K, nullptr, depth.data(), 8, H, W, intr, nullptr, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks(nullptr, P, w2c.data(), K, nullptr, nullptr, 0, H, W, intr, nullptr, cls.data(), nullptr) == DNS_E_ARG;
  n += dns_point_masks_ws_bytes(1u << 31, K, 8) == 0 && dns_point_masks_ws_bytes(P, K, 0) == 0;
  n += dns_point_masks_ws_bytes(P, K, 256) == 6ull * K * 4 && dns_point_masks_ws_bytes(P, K, 1u << 30) == 1ull * K * 4;
  if (n != 9 || g_refused != 7) return printf("refusals: %d of 9 (%d)\n", n, g_refused), 1;
  if (dns_point_masks(nullptr, 0, nullptr, 0, nullptr, nullptr, 0, H, W, intr, nullptr, nullptr, nullptr)) return 1;      // P = 0
  printf("OK\n");
  return 0;
}
