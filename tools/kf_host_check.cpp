// Host check of the kernels of dns_slam_amd/csrc/mesh_feature.hip under the address and undefined-behaviour sanitizers: the
// kernel source itself is compiled for the host (one std::thread per lane of a workgroup, a barrier for __syncthreads) and driven
// through its C entry points over 600 points x 300 keyframes (two LDS tiles) with exactly-sized buffers.  Checked against plain
// loops: no access outside a buffer, an emit capacity below the total stores nothing beyond it, the list is point-major with
// ascending keyframes and never on a depth hole, the bilinear value against float64, C = 6 refused, the mean bit-equal to the
// ordered sum.  No GPU is involved.  From the repository root:
//
//   mkdir -p /tmp/kf_check && for f in dev_project.hpp dev_feature.hpp mesh_feature.hip; do \
//     sed -e 's/#include "common.hpp"//' -e 's/extern "C" //' dns_slam_amd/csrc/$f > /tmp/kf_check/$f; done
//   g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       -Wno-unused-value -I/tmp/kf_check tools/kf_host_check.cpp -o /tmp/kf_check/kf_host_check && /tmp/kf_check/kf_host_check
// (dev_project.hpp and dev_feature.hpp are taken from the source tree the same way as the kernels: only their include of the HIP
// headers is dropped.)
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct int4 { int x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
struct float3 { float x, y, z; };
inline float3 make_float3(float a, float b, float c) { return {a, b, c}; }
inline int4 make_int4(int a, int b, int c, int d) { return {a, b, c, d}; }
inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
inline thread_local dim3 threadIdx, blockIdx;
inline std::barrier<>* g_bar;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline float __fmul_rn(float a, float b) { return a * b; }
using std::max; using std::min;
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
typedef void* hipStream_t;
#define DNS_OK 0
#define DNS_E_ARG (-1)
#define DNS_REQUIRE(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return DNS_E_ARG; } } while (0)
inline int check_launch(const char*) { return 0; }
template <class F, class... A>
void launch(F kern, dim3 grid, dim3 block, A... args) {
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bar(block.x);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
      th.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); kern(args...); });
    for (auto& x : th) x.join();
  }
}
#define DNS_LAUNCH(kern, grid, block, lds, st, ...) launch(kern, grid, block, __VA_ARGS__)

#include "mesh_feature.hip"
#include <random>
int main() {
  std::mt19937 g(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  const uint32_t P = 600, K = 300, C = 8, D = 8; const int H = 12, W = 16, h = 6, w = 8;
  std::vector<float> pts(3 * P), w2c(16 * K, 0.f), org(3 * K), depth((size_t)K * H * W), feat((size_t)K * h * w * C);
  for (auto& x : pts) x = U(g) * 1.5f;
  for (uint32_t k = 0; k < K; ++k) {
    float* m = &w2c[16 * k];
    m[0] = m[5] = m[10] = m[15] = 1.f;
    m[3] = U(g) * 0.3f, m[7] = U(g) * 0.3f, m[11] = -2.5f + U(g) * 0.3f;      // camera looks down -z at the cloud
    for (int i = 0; i < 3; ++i) org[3 * k + i] = -m[4 * i + 3];
  }
  for (size_t i = 0; i < depth.size(); ++i) depth[i] = (i % 17 == 0) ? 0.f : 2.5f + U(g) * 1.2f;
  for (auto& x : feat) x = U(g);
  const float intr[4] = {12.f, 12.f, 8.f, 6.f};
  std::vector<int32_t> count(P);
  if (dns_kf_pair_count(pts.data(), P, w2c.data(), K, depth.data(), H, W, intr, count.data(), nullptr)) return 1;
  std::vector<int64_t> off(P);
  int64_t n = 0;
  for (uint32_t p = 0; p < P; ++p) off[p] = n, n += count[p];
  printf("pairs %lld of %u\n", (long long)n, P * K);
  int32_t* rec = (int32_t*)aligned_alloc(16, 16 * (size_t)std::max<int64_t>(n, 1));
  if (dns_kf_pair_emit(pts.data(), P, w2c.data(), K, depth.data(), H, W, intr, off.data(), rec, n, nullptr)) return 1;
  // a capacity below the total: nothing beyond it may be stored (the sanitizer sees the exact allocation)
  int32_t* rec_small = (int32_t*)aligned_alloc(16, 16 * (size_t)(n / 2));
  if (dns_kf_pair_emit(pts.data(), P, w2c.data(), K, depth.data(), H, W, intr, off.data(), rec_small, n / 2, nullptr)) return 1;
  if (memcmp(rec, rec_small, 16 * (size_t)(n / 2))) return printf("truncated list differs\n"), 1;
  // list order and counts
  int64_t i = 0;
  for (uint32_t p = 0; p < P; ++p)
    for (int32_t j = 0; j < count[p]; ++j, ++i) {
      const int32_t* r = rec + 4 * i;
      if (r[0] != (int)p || (j && r[1] <= r[-3]) || r[1] < 0 || r[1] >= (int)K || r[2] < 0 || r[2] >= W || r[3] < 0 || r[3] >= H)
        return printf("bad record %lld\n", (long long)i), 1;
      const float d = depth[((size_t)r[1] * H + r[3]) * W + r[2]];
      if (!(d > 0.f)) return printf("pair on a depth hole\n"), 1;
    }
  bool lo = false, hi = false;
  for (int64_t q = 0; q < n; ++q) (rec[4 * q + 1] < 256 ? lo : hi) = true;
  printf("keyframes below / above the tile: %d %d\n", lo, hi);
  const uint32_t ld = 12 + C;
  float* rows = (float*)aligned_alloc(16, 4 * (size_t)n * ld);
  std::vector<float> rel(3 * (size_t)n);
  memset(rows, 0, 4 * (size_t)n * ld);
  if (dns_kf_pair_rows(rec, n, pts.data(), P, org.data(), K, feat.data(), C, h, w, H, W, rel.data(), rows + 12, ld, nullptr)) return 1;
  if (dns_kf_pair_rows(rec, n, pts.data(), P, org.data(), K, feat.data(), 6, h, w, H, W, rel.data(), rows + 12, ld, nullptr) != DNS_E_ARG) return 1;
  double worst = 0;
  for (int64_t q = 0; q < n; ++q) {
    const int32_t* r = rec + 4 * q;
    for (int a = 0; a < 3; ++a)
      if (rel[3 * q + a] != pts[3 * r[0] + a] - org[3 * r[1] + a]) return printf("rel differs\n"), 1;
    const double sx = (double)r[2] * (w - 1) / (W - 1), sy = (double)r[3] * (h - 1) / (H - 1);
    const int x0 = (int)sx, y0 = (int)sy, x1 = std::min(x0 + 1, w - 1), y1 = std::min(y0 + 1, h - 1);
    const double lx = sx - x0, ly = sy - y0;
    auto F = [&](int y, int x, uint32_t c) { return (double)feat[(((size_t)r[1] * h + y) * w + x) * C + c]; };
    for (uint32_t c = 0; c < C; ++c) {
      const double want = (1 - ly) * ((1 - lx) * F(y0, x0, c) + lx * F(y0, x1, c)) + ly * ((1 - lx) * F(y1, x0, c) + lx * F(y1, x1, c));
      worst = std::max(worst, std::fabs(want - rows[q * ld + 12 + c]));
    }
    for (int c = 0; c < 12; ++c) if (rows[q * ld + c] != 0.f) return printf("columns below the code written\n"), 1;
  }
  printf("bilinear value: worst |difference| to float64 %.2e\n", worst);
  if (worst > 1e-5) return 1;
  // mean: latents = the code columns of the rows (stride ld), D = C
  float* code = (float*)aligned_alloc(16, 4 * (size_t)P * D);
  if (dns_kf_code_mean(rows + 12, ld, n, off.data(), count.data(), P, D, code, nullptr)) return 1;
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t c = 0; c < D; ++c) {
      float s = 0.f;
      for (int32_t j = 0; j < count[p]; ++j) s += rows[(off[p] + j) * ld + 12 + c];
      const float want = count[p] ? s / (float)count[p] : 0.f;
      if (code[p * D + c] != want) return printf("mean differs at %u %u\n", p, c), 1;
    }
  int maxc = 0;
  for (auto c : count) maxc = std::max(maxc, (int)c);
  printf("mean: bit-equal to the ordered loop, max count %d\nOK\n", maxc);
  free(rec), free(rec_small), free(rows), free(code);
  return 0;
}
