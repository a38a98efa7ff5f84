// Host check of the workspace carver (dns_slam_amd/csrc/ws_carve.hpp) under the address and undefined-behaviour sanitizers.
// No GPU is involved and nothing is loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/ws_carve_check.cpp -o /tmp/ws_carve_check
//   /tmp/ws_carve_check
//
// A layout is a list of parts, each an element size (1, 2, 4, 8, 12, 16 or 40 bytes) and a count.  The lists are every
// combination of three counts out of 0, 1, 63, 64, 65, 255, 256, 257, 1000003 with rotating element sizes, and one list of
// ten parts.  For every list:
//   (a) the walk on a NULL base returns NULL for every part;
//   (b) the walk on a real buffer of exactly end() bytes of the NULL walk puts every part on a multiple of 256 bytes from the
//       base, in order, each starting at or after the end of the one before and less than 256 bytes after it, and the first
//       and last element of every part is written (an overrun is an ASan report);
//   (c) the real walk ends exactly where the NULL walk said;
//   (d) end() is the last part's own end, end256() is end() rounded up to 256, and a carver that took nothing has both 0.
// A second pass restates the old size formulas of three units whose last terms differ (the last part not rounded; every part
// rounded; a closing part of 64 words) and compares them with the carver up to 2^31 - 1.
// mesh_holes_plan.hpp is included as well: the two headers are free of HIP together, and its plan agrees with a carver walk.
#include <stdio.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>
#include "../dns_slam_amd/csrc/ws_carve.hpp"
#include "../dns_slam_amd/csrc/mesh_holes_plan.hpp"

using dns::WsCarve;
using dns::align256;

static long g_fail = 0, g_lists = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++g_fail <= 40) {              \
        printf("FAIL %s: ", #cond);      \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

struct E12 {
  float v[3];
};
struct E40 {
  double v[5];
};

struct Part {
  int size;          // sizeof of the element
  uint64_t count;
};

static char* take(WsCarve& c, const Part& p) {
  switch (p.size) {
    case 1: return (char*)c.take<uint8_t>(p.count);
    case 2: return (char*)c.take<uint16_t>(p.count);
    case 4: return (char*)c.take<uint32_t>(p.count);
    case 8: return (char*)c.take<uint64_t>(p.count);
    case 12: return (char*)c.take<E12>(p.count);
    case 16: return (char*)c.take<long double>(p.count);
    default: return (char*)c.take<E40>(p.count);
  }
}

static void check_list(const std::vector<Part>& parts) {
  ++g_lists;
  WsCarve size(nullptr);
  CHECK(size.end() == 0 && size.end256() == 0, "an empty carver ends at %zu / %zu", size.end(), size.end256());
  for (const Part& p : parts) {
    CHECK(take(size, p) == nullptr, "a NULL base gave a pointer");
    CHECK(size.end256() == align256(size.end()) && size.end256() - size.end() < 256, "ends %zu / %zu", size.end(), size.end256());
  }
  const size_t bytes = size.end();
  char* buf = new char[bytes ? bytes : 1];
  WsCarve real(buf);
  size_t prev_end = 0;
  for (size_t i = 0; i < parts.size(); ++i) {
    const size_t n = (size_t)parts[i].count * parts[i].size;
    char* p = take(real, parts[i]);
    const size_t at = (size_t)(p - buf);
    CHECK(at % 256 == 0, "part %zu at %zu", i, at);
    CHECK(at >= prev_end && at - prev_end < 256, "part %zu at %zu after a part ending at %zu", i, at, prev_end);
    CHECK(real.end() == at + n, "part %zu of %zu bytes at %zu ends at %zu", i, n, at, real.end());
    if (n) memset(p, 0x5a, parts[i].size), memset(p + n - parts[i].size, 0xa5, parts[i].size);
    prev_end = at + n;
  }
  CHECK(real.end() == bytes && real.end256() == size.end256(), "the real walk ends at %zu, the NULL walk at %zu", real.end(), bytes);
  delete[] buf;
}

// The size formulas as the units spelt them before they were carved, against the carver.
static void check_formulas(uint64_t n) {
  {  // last part not rounded (marching cubes over n points)
    const uint64_t chunks = (n + 63) / 64, blocks = (n + 255) / 256;
    WsCarve c(nullptr);
    c.take<uint64_t>(chunks * 3), c.take<uint32_t>(blocks * 2), c.take<uint64_t>(blocks * 2);
    CHECK(c.end() == align256(chunks * 24) + align256(blocks * 8) + blocks * 16, "n %llu: last part raw", (unsigned long long)n);
  }
  {  // every part rounded (list counters and list of the rasterisers)
    WsCarve c(nullptr);
    c.take<uint32_t>(65536), c.take<uint64_t>(n);
    CHECK(c.end256() == align256(65536 * 4) + align256(n * 8), "n %llu: last part rounded", (unsigned long long)n);
  }
  {  // a closing "+ 256" is a last part of 64 words
    WsCarve c(nullptr);
    c.take<int32_t>(n), c.take<double>(n), c.take<uint32_t>(64);
    CHECK(c.end() == align256(n * 4) + align256(n * 8) + 256, "n %llu: closing 64 words", (unsigned long long)n);
  }
}

// The hole filling's plan is the walk a carver makes over its nine parts.
static void check_holes_plan(uint32_t F, uint32_t V) {
  using namespace dns::holesp;
  Plan p;
  if (!make_plan(F, V, &p)) return;
  WsCarve c(nullptr);
  uint64_t off[9];
  for (int i = 0; i < 4; ++i) c.take<uint32_t>(V), off[i] = c.end() - 4ull * V;
  for (int i = 4; i < 6; ++i) c.take<uint32_t>(2ull * p.v_blocks), off[i] = c.end() - 8ull * p.v_blocks;
  c.take<uint64_t>(p.cap), off[6] = c.end() - 8ull * p.cap;
  c.take<uint32_t>(p.cap), off[7] = c.end() - 4ull * p.cap;
  c.take<uint32_t>(p.cap), off[8] = c.end() - 4ull * p.cap;
  CHECK(off[0] == p.off_n_out && off[1] == p.off_n_in && off[2] == p.off_next && off[3] == p.off_cnt && off[4] == p.off_bcount &&
            off[5] == p.off_bpre && off[6] == p.off_keys && off[7] == p.off_count && off[8] == p.off_holder && c.end256() == p.bytes,
        "F %u V %u: the plan is not the carver's walk", F, V);
}

int main() {
  const uint64_t counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000003};
  const int sizes[] = {1, 2, 4, 8, 12, 16, 40};
  int rot = 0;
  for (uint64_t a : counts)
    for (uint64_t b : counts)
      for (uint64_t c : counts) {
        check_list({{sizes[rot % 7], a}, {sizes[(rot + 3) % 7], b}, {sizes[(rot + 5) % 7], c}});
        ++rot;
      }
  check_list({});
  check_list({{4, 0}});
  check_list({{4, 1000}, {4, 1000}, {4, 1000}, {8, 1000}, {8, 256}, {4, 64}, {4, 64}, {40, 1024}, {12, 1}, {4, 64}});
  check_list({{16, 1u << 24}, {1, 3}, {8, (1u << 24) + 1}});       // large: 256 MiB and 128 MiB parts

  std::vector<uint64_t> ns = {0, 1, 63, 64, 65, 255, 256, 257, 1000003};
  for (int k = 1; k <= 31; ++k)
    for (uint64_t x : {(1ull << k) - 1, 1ull << k, (1ull << k) + 1})
      if (x < (1ull << 31)) ns.push_back(x);
  for (uint64_t n : ns) check_formulas(n);
  for (uint32_t F : {0u, 1u, 64u, 1000003u, (1u << 29) - 1, 1u << 29})
    for (uint32_t V : {0u, 1u, 3u, 255u, 256u, 257u, 1000003u, (1u << 31) - 1, 1u << 31}) check_holes_plan(F, V);
  printf("ws_carve_check: %ld part lists, %zu sizes, %ld failed conditions\n", g_lists, ns.size(), g_fail);
  return g_fail ? 1 : 0;
}
