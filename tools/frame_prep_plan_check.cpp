// Host check of the frame preparation's tables (dns_slam_amd/csrc/frame_prep_plan.hpp) under the address and undefined-behaviour
// sanitizers.  No GPU is involved and nothing is loaded into Python.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/frame_prep_plan_check.cpp -o /tmp/frame_prep_plan_check
//   /tmp/frame_prep_plan_check
//
// Sizes sweep 1, 2, 3, 5, 7, 64, 65, the dataset sides (480, 484, 640, 648, 680, 968, 1200, 1296) and the limit 32768: src = 1,
// src = dst, up-sampling and down-sampling all occur.  For every (src, dst) pair and each of the four rules:
//   (a) every index lies in [0, src);
//   (b) each weight pair is finite, non-negative and sums to 1 within one ulp of 1;
//   (c) src = dst is the identity: index d, weights exactly (1, 0);
//   (d) indices do not decrease along the axis; the two linear rules start at source 0 and, where dst > 1 or src = 1, the
//       align_corners rule ends at source src - 1.
// For dims built from the same sides: refused sizes are refused; the parts of the blob lie in the stated order, without gaps or
// overlap, and end at `words`; the identity stages are recognised exactly when their sizes are equal; fill_tables writes every word
// of a buffer of exactly `words` words (a guard pattern must be gone, and ASan sees any write past the end); the grid covers H W.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../dns_slam_amd/csrc/frame_prep_plan.hpp"

using namespace dns::fprep;

static long g_fail = 0, g_pairs = 0, g_plans = 0;
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

static bool pair_ok(const float* w) {
  const float s = w[0] + w[1];
  return isfinite(w[0]) && isfinite(w[1]) && w[0] >= 0.0f && w[1] >= 0.0f && fabsf(s - 1.0f) <= FLT_EPSILON;
}

static void check_axis(uint32_t src, uint32_t dst) {
  ++g_pairs;
  int32_t prev[4] = {0, 0, 0, 0};
  for (uint32_t d = 0; d < dst; ++d) {
    int32_t i[4];
    float wc[2], wt[2];
    cv_linear(d, src, dst, &i[0], wc);
    torch_linear(d, src, dst, &i[1], wt);
    i[2] = cv_nearest(d, src, dst);
    i[3] = torch_nearest(d, src, dst);
    for (int r = 0; r < 4; ++r) {
      CHECK(i[r] >= 0 && i[r] < (int32_t)src, "rule %d, %u -> %u, d %u: index %d", r, src, dst, d, i[r]);
      CHECK(d == 0 || i[r] >= prev[r], "rule %d, %u -> %u, d %u: index %d after %d", r, src, dst, d, i[r], prev[r]);
      prev[r] = i[r];
      if (src == dst) CHECK(i[r] == (int32_t)d, "rule %d, %u -> %u, d %u: index %d is not the identity", r, src, dst, d, i[r]);
    }
    CHECK(pair_ok(wc), "cv linear %u -> %u, d %u: weights %g %g", src, dst, d, (double)wc[0], (double)wc[1]);
    CHECK(pair_ok(wt), "torch linear %u -> %u, d %u: weights %g %g", src, dst, d, (double)wt[0], (double)wt[1]);
    if (src == dst) {
      CHECK(wc[0] == 1.0f && wc[1] == 0.0f, "cv linear %u, d %u: identity weights %g %g", src, d, (double)wc[0], (double)wc[1]);
      CHECK(wt[0] == 1.0f && wt[1] == 0.0f, "torch linear %u, d %u: identity weights %g %g", src, d, (double)wt[0], (double)wt[1]);
    }
    if (d == 0) CHECK(i[1] == 0 && wt[1] == 0.0f && i[2] == 0 && i[3] == 0, "%u -> %u: the first coordinate reads %d %d %d", src, dst, i[1], i[2], i[3]);
    if (d == dst - 1 && dst > 1) {
      // align_corners: the last coordinate is the last source pixel, up to the rounding of scale (dst - 1)
      const bool last = (i[1] == (int32_t)src - 1) || (i[1] == (int32_t)src - 2 && wt[1] > 0.99f);
      CHECK(last, "torch linear %u -> %u: the last coordinate reads %d (%g)", src, dst, i[1], (double)wt[1]);
    }
  }
}

static void check_dims(const DnsFramePrepDims& d) {
  Plan p;
  const bool labels = d.Hl || d.Wl;
  const bool want = side_ok(d.Hc) && side_ok(d.Wc) && side_ok(d.Hd) && side_ok(d.Wd) && side_ok(d.Hs) && side_ok(d.Ws) &&
                    (!labels || (side_ok(d.Hl) && side_ok(d.Wl))) && d.edge < MAX_SIDE && 2ull * d.edge < d.Hs && 2ull * d.edge < d.Ws;
  const bool ok = make_plan(d, &p);
  CHECK(ok == want, "dims %u %u %u %u %u %u %u %u %u: planned %d", d.Hc, d.Wc, d.Hd, d.Wd, d.Hl, d.Wl, d.Hs, d.Ws, d.edge, (int)ok);
  if (!ok) return;
  ++g_plans;
  CHECK(p.H == d.Hs - 2 * d.edge && p.W == d.Ws - 2 * d.edge && p.H >= 1 && p.W >= 1, "output %u x %u", p.H, p.W);
  const uint64_t off[13] = {p.cv_x_idx, p.cv_x_w, p.cv_y_idx, p.cv_y_w, p.tb_x_idx, p.tb_x_w, p.tb_y_idx, p.tb_y_w, p.tn_x, p.tn_y, p.cn_x, p.cn_y, p.words};
  const uint64_t need[12] = {d.Wd, 2ull * d.Wd, d.Hd, 2ull * d.Hd, d.Ws, 2ull * d.Ws, d.Hs, 2ull * d.Hs, d.Ws, d.Hs, d.Wd, d.Hd};
  CHECK(off[0] == 0, "first part at %llu", (unsigned long long)off[0]);
  for (int i = 0; i < 12; ++i) CHECK(off[i + 1] - off[i] == need[i], "part %d: %llu words for %llu", i, (unsigned long long)(off[i + 1] - off[i]), (unsigned long long)need[i]);
  CHECK(((p.ident & IDENT_CV) != 0) == (d.Hc == d.Hd && d.Wc == d.Wd), "cv linear identity flag %u", p.ident);
  CHECK(((p.ident & IDENT_TORCH) != 0) == (d.Hs == d.Hd && d.Ws == d.Wd), "torch identity flag %u", p.ident);
  CHECK(((p.ident & IDENT_CVN) != 0) == (labels && d.Hl == d.Hd && d.Wl == d.Wd), "cv nearest identity flag %u", p.ident);
  CHECK((uint64_t)p.grid_x * FP_BLOCK >= (uint64_t)p.H * p.W && (uint64_t)p.grid_x * FP_BLOCK < (uint64_t)p.H * p.W + FP_BLOCK, "grid %u", p.grid_x);
  CHECK((uint64_t)p.H * p.W <= (1ull << 30), "%u x %u output pixels", p.H, p.W);
  const int32_t guard = (int32_t)0x7fc0dead;          // no index and no weight in [0, 1] has these bits
  std::vector<int32_t> words((size_t)p.words, guard);
  fill_tables(d, p, words.data());
  uint64_t left = 0;
  for (int32_t w : words) left += w == guard;
  CHECK(left == 0, "%llu words of %llu not written", (unsigned long long)left, (unsigned long long)p.words);
  const uint32_t srcs[4] = {d.Wc, d.Hc, d.Wd, d.Hd}, lims[4] = {d.Wd, d.Hd, d.Ws, d.Hs};
  const uint64_t idx[4] = {p.cv_x_idx, p.cv_y_idx, p.tb_x_idx, p.tb_y_idx}, wts[4] = {p.cv_x_w, p.cv_y_w, p.tb_x_w, p.tb_y_w};
  for (int t = 0; t < 4; ++t)
    for (uint32_t k = 0; k < lims[t]; ++k) {
      float w[2];
      memcpy(w, &words[(size_t)(wts[t] + 2ull * k)], sizeof w);
      CHECK(words[(size_t)(idx[t] + k)] >= 0 && words[(size_t)(idx[t] + k)] < (int32_t)srcs[t] && pair_ok(w), "table %d entry %u", t, k);
    }
  const uint32_t nsrc[4] = {d.Wd, d.Hd, labels ? d.Wl : 1u, labels ? d.Hl : 1u}, nlim[4] = {d.Ws, d.Hs, d.Wd, d.Hd};
  const uint64_t nidx[4] = {p.tn_x, p.tn_y, p.cn_x, p.cn_y};
  for (int t = 0; t < 4; ++t)
    for (uint32_t k = 0; k < nlim[t]; ++k)
      CHECK(words[(size_t)(nidx[t] + k)] >= 0 && words[(size_t)(nidx[t] + k)] < (int32_t)nsrc[t], "nearest table %d entry %u", t, k);
}

int main() {
  const std::vector<uint32_t> sides = {1, 2, 3, 5, 7, 64, 65, 480, 484, 640, 648, 680, 968, 1200, 1296, 32768};
  for (uint32_t s : sides)
    for (uint32_t d : sides) check_axis(s, d);
  const std::vector<uint32_t> small = {0, 1, 5, 7, 65, 32768, 32769};
  for (uint32_t c : small)
    for (uint32_t dd : small)
      for (uint32_t l : {0u, 1u, 7u, 32769u})
        for (uint32_t s : {0u, 1u, 5u, 65u})
          for (uint32_t e : {0u, 1u, 2u, 32u}) {
            check_dims({c, dd, dd, c, l, l, s, dd ? dd : 1u, e});
            check_dims({c, c, c, c, l, c, c, c, e});
          }
  check_dims({680, 1200, 680, 1200, 680, 1200, 680, 1200, 0});      // Replica
  check_dims({968, 1296, 480, 640, 968, 1296, 480, 640, 10});       // ScanNet
  check_dims({968, 1296, 480, 640, 968, 1296, 484, 648, 10});
  check_dims({7, 1, 5, 3, 0, 9, 5, 3, 0});                          // labels with one side 0: refused
  printf("frame_prep_plan_check: %ld axis pairs, %ld plans, %ld failed conditions\n", g_pairs, g_plans, g_fail);
  return g_fail ? 1 : 0;
}
