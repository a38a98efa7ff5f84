// Host check of the draw path of dns_slam_amd/csrc/dev_raster.hpp under the address and undefined-behaviour sanitizers: the header's
// kernels are compiled for the host (no barrier and no cross-lane operation in them, so plain loops over blocks and threads) and
// launched by the library's own walk, rs_draw, with both pixel sinks, into buffers of exactly the elements a draw may touch.  Four
// scenes it builds itself (3 poses, 40 x 24 pixels), each under both methods and list_cap 0, 7 and F.  Every check is exact: the
// depth sink's image is the upper half of the key sink's, the images are the same bits for every method and cap, the counts of
// the two sinks agree and status[1] is the sum of the launches' counters, the walk hands every (face, view) pair to exactly one
// launch of at most cap pairs, the lattice's pixels hold 2.0, a bad index and a NaN vertex are flagged and only their faces
// missing, culled faces are absent and never reach the list.  No GPU is involved.  From the repository root:
//
//   mkdir -p /tmp/rs_check && cp dns_slam_amd/csrc/ws_carve.hpp /tmp/rs_check && \
//     sed -e 's/#include "common.hpp"//' dns_slam_amd/csrc/dev_raster.hpp > /tmp/rs_check/dev_raster.hpp
//   g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I/tmp/rs_check -Iinclude tools/raster_host_check.cpp -o /tmp/rs_check/check && /tmp/rs_check/check
#include <math.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <tuple>
#include <vector>
#include "dns_hip.h"
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 threadIdx, blockIdx, gridDim;
using std::min;
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
template <class T> T atomicMin(T* a, T v) { const T old = *a; *a = std::min(old, v); return old; }
inline uint32_t atomicAdd(uint32_t* a, uint32_t v) { const uint32_t old = *a; *a = old + v; return old; }
inline uint32_t atomicOr(uint32_t* a, uint32_t v) { const uint32_t old = *a; *a = old | v; return old; }
#define __hip_atomic_load(p, order, scope) (*(p))
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
typedef void* hipStream_t;
#define DNS_REQUIRE(cond, ...) do { if (!(cond)) return DNS_E_ARG; } while (0)

// every launch: all blocks and threads in order; a set-up launch (14 arguments) is also recorded for the checks of the walk
struct SetupLaunch { uint32_t f_lo, f_hi, v_lo, nv, cap; const uint32_t* counter; };
static std::vector<SetupLaunch> g_setups;
template <class K, class... A>
void launch(K kern, dim3 grid, dim3 block, A... args) {
  if constexpr (sizeof...(A) == 14) {
    const auto t = std::make_tuple(args...);
    g_setups.push_back({std::get<3>(t), std::get<4>(t), std::get<6>(t), grid.y, std::get<10>(t), std::get<11>(t)});
  }
  gridDim = grid;
  for (unsigned by = 0; by < grid.y; ++by)
    for (unsigned bx = 0; bx < grid.x; ++bx)
      for (unsigned t = 0; t < block.x; ++t) threadIdx = dim3(t), blockIdx = dim3(bx, by), kern(args...);
}
#define DNS_LAUNCH_AS(name, kern, grid, block, lds, st, ...) launch(kern, grid, block, __VA_ARGS__)

#include "dev_raster.hpp"
using namespace dns;

static const uint32_t H = 24, W = 40, V = 3;
static const float INTR[4] = {32.f, 32.f, 19.5f, 11.5f}, Z_NEAR = 0.01f, Z_FAR = 20.f;
// the camera moved by whole pixels of the plane z = 2 (1/16 each): every coordinate stays a small dyadic number
static const float W2C[V * 16] = {1, 0, 0, 0,          0, 1, 0, 0,         0, 0, 1, 0, 0, 0, 0, 1,
                                  1, 0, 0, 1.f / 16,   0, 1, 0, 0,         0, 0, 1, 0, 0, 0, 0, 1,
                                  1, 0, 0, -2.f / 16,  0, 1, 0, 1.f / 16,  0, 0, 1, 0, 0, 0, 0, 1};

struct Scene {
  const char* name;
  std::vector<float> verts;
  std::vector<int32_t> faces;
  uint32_t P() const { return (uint32_t)verts.size() / 3; }
  uint32_t F() const { return (uint32_t)faces.size() / 3; }
};

struct Drawn {
  std::vector<uint64_t> img;                                      // either sink's words
  uint32_t status[4];
  bool operator==(const Drawn& o) const { return img == o.img; }
};

#define FAIL(...) return printf(__VA_ARGS__), printf("\n"), 1

// One draw as the library's wrappers make it, every part of the workspace its own allocation; checks 3 (the counter sum) and 4.
template <class Sink>
static int draw(const Scene& sc, uint32_t flags, uint32_t list_cap, Drawn* out) {
  using Word = typename Sink::Word;
  const uint32_t P = sc.P(), F = sc.F();
  RsCam cam;
  RsCut cut;
  if (rs_check("check", P, F, V, H, W, INTR, Z_NEAR, Z_FAR, list_cap, &cam, &cut)) FAIL("%s: refused", sc.name);
  const size_t n_words = (size_t)V * H * W;
  const uint64_t n_list = rs_list_entries(F, V, cut.cap);
  if (cut.n_launch > RS_MAX_LAUNCHES || n_list > rs_list_entries(F, V, RS_LIST_CAP)) FAIL("%s: beyond the layout", sc.name);
  const std::unique_ptr<Word[]> img(new Word[n_words]);
  const std::unique_ptr<uint32_t[]> counters(new uint32_t[cut.n_launch]), status(new uint32_t[4]);
  const std::unique_ptr<uint64_t[]> list(new uint64_t[n_list]);
  const RsWs w = {nullptr, counters.get(), list.get()};
  g_setups.clear();
  rs_draw<Sink>(sc.verts.data(), P, sc.faces.data(), F, W2C, V, cam, flags, cut, w, img.get(), status.get(), nullptr);
  status[1] = rs_list_total(counters.get(), (uint32_t)cut.n_launch);       // as both units' last kernels do
  out->img.assign(img.get(), img.get() + n_words);
  memcpy(out->status, status.get(), sizeof out->status);
  // the walk: every pair in exactly one launch of at most cap pairs, launch k on counter k < n_launch
  if (g_setups.size() != cut.n_launch) FAIL("%s: %zu launches, the cut says %llu", sc.name, g_setups.size(), (unsigned long long)cut.n_launch);
  std::vector<uint8_t> seen((size_t)F * V, 0);
  uint64_t sum = 0;
  for (size_t k = 0; k < g_setups.size(); ++k) {
    const SetupLaunch& s = g_setups[k];
    const uint32_t cap = list_cap ? list_cap : RS_LIST_CAP;
    if (s.counter != counters.get() + k || s.cap != cap || s.f_lo >= s.f_hi || s.f_hi > F || !s.nv || s.v_lo + s.nv > V ||
        (uint64_t)(s.f_hi - s.f_lo) * s.nv > cap || *s.counter > (uint64_t)(s.f_hi - s.f_lo) * s.nv)
      FAIL("%s: launch %zu: faces [%u, %u), views [%u, +%u), cap %u, %u entries", sc.name, k, s.f_lo, s.f_hi, s.v_lo, s.nv, s.cap, *s.counter);
    for (uint32_t v = s.v_lo; v < s.v_lo + s.nv; ++v)
      for (uint32_t f = s.f_lo; f < s.f_hi; ++f) ++seen[(size_t)v * F + f];
    sum += *s.counter;
  }
  if (std::count(seen.begin(), seen.end(), 1) != (ptrdiff_t)seen.size()) FAIL("%s: a pair is in no launch or in two", sc.name);
  if (sum != status[1] || ((flags & DNS_RASTER_SIMPLE) && sum)) FAIL("%s: status[1] %u, the counters hold %llu", sc.name, status[1], (unsigned long long)sum);
  return 0;
}

// Both sinks under one setting; check 1 and the sinks' half of check 3.
static int both(const Scene& sc, uint32_t flags, uint32_t list_cap, Drawn* depth, Drawn* keys) {
  if (draw<RsDepthSink>(sc, flags, list_cap, depth) || draw<RsKeySink>(sc, flags, list_cap, keys)) return 1;
  for (size_t q = 0; q < keys->img.size(); ++q) {
    const uint64_t k = keys->img[q], d = depth->img[q];
    if (k == RsKeySink::EMPTY ? d != RsDepthSink::EMPTY : d != k >> 32) FAIL("%s: pixel %zu: depth %#llx, key %#llx", sc.name, q, (unsigned long long)d, (unsigned long long)k);
  }
  if (memcmp(depth->status, keys->status, sizeof depth->status)) FAIL("%s: the sinks' status words differ", sc.name);
  return 0;
}

// A scene under both methods and the three caps (check 2); -> the auto images and counts.
static int scene(const Scene& sc, Drawn* depth, Drawn* keys) {
  if (both(sc, DNS_RASTER_STATS, 0, depth, keys)) return 1;
  for (uint32_t method : {0u, DNS_RASTER_SIMPLE})
    for (uint32_t cap : {0u, 7u, sc.F()}) {
      Drawn d, k;
      if (both(sc, method | DNS_RASTER_STATS, cap, &d, &k)) return 1;
      if (!(d == *depth) || !(k == *keys)) FAIL("%s: method %u, cap %u: another image", sc.name, method, cap);
      // a pair is drawn by its set-up thread or through the list, whatever the method and the cut
      if (d.status[0] != depth->status[0] || d.status[1] + d.status[2] != depth->status[1] + depth->status[2] ||
          (!method && d.status[1] != depth->status[1]))
        FAIL("%s: method %u, cap %u: status %u %u %u", sc.name, method, cap, d.status[0], d.status[1], d.status[2]);
    }
  size_t covered = 0;
  for (uint64_t d : depth->img) covered += d != RsDepthSink::EMPTY;
  printf("%-8s %3u faces: %4zu pixels covered, %3u pairs through the list, %3u by their set-up thread, status[0] %u: ok\n", sc.name,
         sc.F(), covered, depth->status[1], depth->status[2], depth->status[0]);
  return 0;
}

// 2 x (n x n) triangles in the plane z = 2, the vertices on the pixel centres (i0 + i, j0 + j) of the first pose.
static Scene lattice(const char* name, int n, int i0, int j0) {
  Scene sc{name, {}, {}};
  for (int i = 0; i <= n; ++i)
    for (int j = 0; j <= n; ++j) {
      const float xyz[3] = {((float)(j0 + j) - INTR[2]) / INTR[0] * 2.f, ((float)(i0 + i) - INTR[3]) / INTR[1] * 2.f, 2.f};
      sc.verts.insert(sc.verts.end(), xyz, xyz + 3);
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const int32_t a = i * (n + 1) + j, s = n + 1, f[6] = {a, a + 1, a + s + 1, a, a + s + 1, a + s};
      sc.faces.insert(sc.faces.end(), f, f + 6);
    }
  return sc;
}

int main() {
  Drawn d, k, d2, k2;
  // 1. a quad over most of the image: both triangles draw through the list
  const Scene quad{"quad", {-1.1f, -0.6f, 2.f, 1.1f, -0.6f, 2.f, 1.1f, 0.6f, 2.f, -1.1f, 0.6f, 2.f}, {0, 1, 2, 0, 2, 3}};
  if (scene(quad, &d, &k)) return 1;
  if (d.status[1] != 2 * V || d.status[2] != 0) FAIL("quad: %u pairs through the list", d.status[1]);
  // 2. the lattice: every triangle by its set-up thread; its 7 x 7 pixel centres, moved with the pose, hold 2.0 and nothing else is hit
  const int N = 6, I0 = 8, J0 = 16;
  const Scene lat = lattice("lattice", N, I0, J0);
  if (scene(lat, &d, &k)) return 1;
  if (d.status[1] != 0 || d.status[2] != lat.F() * V) FAIL("lattice: %u pairs by their set-up thread", d.status[2]);
  const int shift[V][2] = {{0, 0}, {0, 1}, {1, -2}};                 // (rows, columns): fy t.y / 2, fx t.x / 2 pixels
  for (uint32_t v = 0; v < V; ++v)
    for (int i = 0; i < (int)H; ++i)
      for (int j = 0; j < (int)W; ++j) {
        const int a = i - I0 - shift[v][0], b = j - J0 - shift[v][1];
        const bool in = a >= 0 && a <= N && b >= 0 && b <= N;
        const uint32_t got = (uint32_t)d.img[((size_t)v * H + i) * W + j];
        if (got != (in ? __float_as_uint(2.f) : RsDepthSink::EMPTY)) FAIL("lattice: view %u pixel (%d, %d) holds %g", v, i, j, uint_as_float(got));
      }
  // 3. one vertex behind the camera: the whole-image box, through the list
  const Scene behind{"behind", {-0.5f, -0.3f, 2.f, 0.5f, -0.3f, 2.f, 0.f, 0.4f, -1.f}, {0, 1, 2}};
  if (scene(behind, &d2, &k2)) return 1;
  if (d2.status[1] != V || d2.status[2] != 0) FAIL("behind: %u pairs through the list", d2.status[1]);
  // 4. the lattice with a face that holds the index P and one with a NaN vertex: flagged, and what the lattice draws without the two
  Scene bad = lat, want = lat;
  bad.name = "flagged", want.name = "two less";
  bad.verts.insert(bad.verts.end(), {NAN, 0.f, 2.f});
  want.verts.insert(want.verts.end(), {0.f, 0.f, 2.f});
  bad.faces[3 * 10 + 1] = (int32_t)bad.P(), bad.faces[3 * 40 + 2] = (int32_t)bad.P() - 1;
  for (int c = 0; c < 3; ++c) want.faces[3 * 10 + c] = want.faces[3 * 40 + c] = 0;      // n = 0: skipped, not flagged
  if (scene(bad, &d2, &k2)) return 1;
  if (d2.status[0] != (DNS_RASTER_BAD_INDEX | DNS_RASTER_NONFINITE) || d2.status[2] != (lat.F() - 2) * V) FAIL("flagged: status[0] %u", d2.status[0]);
  Drawn dw, kw;
  if (both(want, DNS_RASTER_STATS, 0, &dw, &kw)) return 1;
  if (!(dw == d2) || !(kw == k2) || dw.status[0] || kw == k) FAIL("flagged: not the lattice less two faces");
  // 7. culling (the key sink): a face is all there or not at all, by its winding; a culled pair never reaches the list
  for (const Scene* sc : {&lat, &quad}) {
    Drawn all, back, front, none;
    none.img.assign((size_t)V * H * W, RsKeySink::EMPTY);
    if (draw<RsKeySink>(*sc, DNS_RASTER_STATS, 7, &all) || draw<RsKeySink>(*sc, DNS_RASTER_STATS | DNS_RENDER_CULL_BACK, 7, &back) ||
        draw<RsKeySink>(*sc, DNS_RASTER_STATS | DNS_RENDER_CULL_FRONT, 7, &front))
      return 1;
    RsTri t;
    uint32_t st = 0;
    const RsCam cam = {INTR[0], INTR[1], INTR[2], INTR[3], Z_NEAR, Z_FAR, (int)H, (int)W};
    if (!rs_setup(sc->verts.data(), sc->P(), sc->faces.data(), 0, W2C, cam, t, &st) || t.num == 0.f) FAIL("%s: face 0 is not drawn", sc->name);
    const Drawn &kept = t.num < 0.f ? back : front, &gone = t.num < 0.f ? front : back;      // num < 0: front-facing
    if (!(kept == all) || kept.status[1] != all.status[1] || kept.status[2] != all.status[2]) FAIL("%s: the kept side differs", sc->name);
    if (!(gone == none) || gone.status[1] || gone.status[2]) FAIL("%s: the culled side drew %u + %u pairs", sc->name, gone.status[1], gone.status[2]);
    printf("%-8s culled: %s-facing, kept and dropped whole: ok\n", sc->name, t.num < 0.f ? "front" : "back");
  }
  // no faces: no launch of the walk, an empty image; the shared refusals
  const Scene empty{"empty", {0.f, 0.f, 2.f}, {}};
  if (both(empty, 0, 0, &d, &k) || std::count(k.img.begin(), k.img.end(), RsKeySink::EMPTY) != (ptrdiff_t)k.img.size()) FAIL("empty: drew");
  RsCam cam;
  RsCut cut;
  const float nan_intr[4] = {32.f, NAN, 0.f, 0.f};
  if (rs_check("check", 3, 1, 0, H, W, nullptr, Z_NEAR, Z_FAR, 0, &cam, &cut) != DNS_OK ||                // V = 0 reads no intrinsics
      rs_check("check", 3, 1u << 31, V, H, W, INTR, Z_NEAR, Z_FAR, 0, &cam, &cut) != DNS_E_ARG ||
      rs_check("check", 3, 1, V, 0, W, INTR, Z_NEAR, Z_FAR, 0, &cam, &cut) != DNS_E_ARG ||
      rs_check("check", 3, 1, V, H, W, INTR, 0.f, Z_FAR, 0, &cam, &cut) != DNS_E_ARG ||
      rs_check("check", 3, 1, V, H, W, nullptr, Z_NEAR, Z_FAR, 0, &cam, &cut) != DNS_E_ARG ||
      rs_check("check", 3, 1, V, H, W, nan_intr, Z_NEAR, Z_FAR, 0, &cam, &cut) != DNS_E_ARG ||
      rs_check("check", 3, 70000, V, H, W, INTR, Z_NEAR, Z_FAR, 1, &cam, &cut) != DNS_E_ARG)              // 210000 launches
    FAIL("rs_check: a refusal is missing");
  printf("OK\n");
  return 0;
}
