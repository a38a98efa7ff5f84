// Host check of the table scatter's launch plan (dns_slam_amd/csrc/scatter_plan.hpp) under the address and undefined-behaviour
// sanitizers.  No GPU is involved and nothing is loaded into Python: the plan is a plain C++ value.  From the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra tools/scatter_plan_check.cpp -o /tmp/scatter_plan_check
//   /tmp/scatter_plan_check --expect tools/scatter_plan_expected.txt
//
// Sweep: P in {0, 1, 63, 1023, 1025, 5000, 262144, 2^30} x the grids of the tests and the benchmark (log2 T, finest resolution:
// (12, 64), (14, 200), (16, 592), (20, 231); level tables from grid_meta_fill, the body of dns_grid_meta_init) x the scatter forms
// x queue_cap in {0, 64} x the default knobs and every knob at both ends of its accepted range.  Every plan is held to what the
// kernels and launch_table_scatter rely on (check_plan below: conditions, not measurements).  One line per (grid, P, form) goes
// to stdout: the default knobs' numbers and a hash over all the plans of that line; --plans prints one line per plan instead,
// to find which one moved.  --expect FILE fails on any difference from FILE: tools/scatter_plan_expected.txt holds the lines of
// the arithmetic as it stood before the plan became one value, so a change of any plan is a deliberate change of that file
// (--write FILE writes it).
#include <math.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../dns_slam_amd/csrc/scatter_plan.hpp"

using namespace dns;

static int g_fail = 0;
static std::string g_cfg;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 40) {                                \
        printf("FAIL [%s] %s: ", g_cfg.c_str(), #cond);    \
        printf(__VA_ARGS__);                               \
        printf("\n");                                      \
      }                                                    \
    }                                                      \
  } while (0)

constexpr uint32_t ATTR_BINNED_LDS = 8192 * 2 * 8;       // the attribute scatter_init_attrs registers for the binned and queue kernels

static bool pow2(uint32_t v) { return v && !(v & (v - 1u)); }

static void check_launch_shape(const char* what, const ScatterLaunch& L, uint32_t lds_limit) {
  CHECK(L.grid >= 1 && L.grid <= 0x7fffffffu, "%s grid %u", what, L.grid);
  CHECK(L.grid_y >= 1 && L.grid_y <= 65535u, "%s grid.y %u", what, L.grid_y);
  CHECK(L.block >= 64 && L.block <= 1024 && L.block % 64 == 0, "%s block %u", what, L.block);
  CHECK(L.lds <= lds_limit && L.lds <= (uint32_t)MAX_DYN_LDS, "%s lds %u > %u", what, L.lds, lds_limit);
}

// which (level, chunk, slice) a workgroup of hashgrid_bwd_binned_kernel takes: the kernel's XCD-major decode; false = padding
static bool sweep_job_of(const BinPlan& plan, uint32_t block, uint32_t& l, uint32_t& chunk, uint32_t& slice) {
  const uint32_t xcd = block & 7u;
  uint32_t q = block >> 3;
  for (l = 0; l < plan.n_levels; ++l) {
    const uint32_t g_lo = plan.group_prefix[l], g_hi = plan.group_prefix[l + 1];
    const uint32_t first = g_lo + ((xcd + 8u - (g_lo & 7u)) & 7u);
    const uint32_t cnt = first < g_hi ? (g_hi - first + 7u) / 8u : 0u;
    const uint32_t nj = cnt * plan.chunks[l];
    if (q < nj) {
      slice = first + 8u * (q / plan.chunks[l]) - g_lo;
      chunk = q % plan.chunks[l];
      return true;
    }
    q -= nj;
  }
  return false;
}

static void check_plan(uint32_t P, const GridLevels& lv, uint32_t flags, uint32_t queue_cap, const ScatterKnobs& k, const ScatterPlan& S) {
  const uint32_t L = lv.n_levels;
  const bool issued = P > 0;                             // dns_encode_bwd returns before any launch when there are no points
  // ---- workspace: [gradient copy | 4 max words | list counters | queue counters | queues | lists | replayed rows], no overlap
  const uint32_t n_lists = S.lists ? S.lp.qoff[S.lp.n] : 0u;
  uint64_t at = (uint64_t)P * L * 2;                     // dg_t: [L][P] float2 from ws + 0
  CHECK(S.gmax == at, "gmax %llu", (unsigned long long)S.gmax);
  at += 4;
  CHECK(S.lcount == at, "lcount");
  if (S.lists) at += (uint64_t)4 * n_lists + 4;          // counts, cursors, list starts, job prefix (n_lists + 1)
  CHECK(S.qcount == at, "qcount");
  CHECK(S.gmax + S.clear_words <= S.qcount, "the first fill (%u words) runs past the counters", S.clear_words);
  CHECK(S.clear_words == 4 + 2 * n_lists, "clear_words %u", S.clear_words);
  if (S.part) at += (uint64_t)DNS_MAX_LEVELS * PART_MAX_CHUNKS;
  CHECK(S.queues == at, "queues");
  if (S.part) {
    CHECK(S.pp.qoff[S.pp.n] <= DNS_MAX_LEVELS * PART_MAX_CHUNKS, "queue counters %u", S.pp.qoff[S.pp.n]);
    for (uint32_t i = 0; i < S.pp.n; ++i)
      CHECK(S.queues + S.pp.qbase[i] + (uint64_t)S.pp.chunks[i] * S.pp.cap[i] * 3u <= S.queues + part_floats(S.pp), "queue %u past its region", i);
    at += part_floats(S.pp);
  }
  CHECK(S.lwords == at, "lwords");
  if (S.lists) {
    for (uint32_t i = 0; i < S.lp.n; ++i) {
      const uint64_t extent = S.lp.dense[i] ? (uint64_t)S.lp.cap[i] : (uint64_t)S.lp.chunks[i] * S.lp.cap[i];
      CHECK(S.lp.qbase[i] + extent <= list_words(S.lp), "list level %u past the lists' region", i);
      if (i + 1 < S.lp.n) CHECK(S.lp.qbase[i] + extent <= S.lp.qbase[i + 1], "list levels %u and %u overlap", i, i + 1);
    }
    at += list_words(S.lp);
  }
  at = (at + 3u) & ~(uint64_t)3u;
  CHECK(S.replay == at && S.replay % 4 == 0, "replay %llu", (unsigned long long)S.replay);
  if (flags & DNS_SCATTER_REPLAY) at += (uint64_t)P * L * 4;
  CHECK(S.total == at, "total %llu", (unsigned long long)S.total);
  CHECK(S.n_replay <= L && S.replay + (uint64_t)S.n_replay * P * 4 <= S.total, "%u replayed planes past the workspace", S.n_replay);
  CHECK(!S.n_replay || (flags & DNS_SCATTER_REPLAY), "replay without its flag");
  // ---- every level of more than one chunk by exactly one form; one-chunk levels by the sweep
  const BinPlan& B = S.bins;
  CHECK(B.n_levels == L && B.chunk_rows >= 1024 && B.chunk_rows <= 8192, "chunk_rows %u", B.chunk_rows);
  uint32_t slots = 0;
  for (uint32_t l = 0; l < L; ++l) {
    const bool in_list = S.lists && S.in_list[l], in_part = S.part && S.in_part[l], in_sweep = B.chunks[l] > 0;
    CHECK((int)in_list + (int)in_part + (int)in_sweep == 1, "level %u (%u rows): lists %d queues %d sweep %d", l, lv.size[l], in_list, in_part, in_sweep);
    if (lv.size[l] <= 8192u) CHECK(in_sweep, "one-chunk level %u not in the sweep", l);
    if (in_sweep) CHECK((uint64_t)B.chunks[l] * B.chunk_rows >= lv.size[l], "level %u: %u chunks of %u rows < %u", l, B.chunks[l], B.chunk_rows, lv.size[l]);
    CHECK(B.slices[l] >= 1, "level %u: no slice", l);
    CHECK(B.job_prefix[l + 1] - B.job_prefix[l] == B.chunks[l] * B.slices[l], "job_prefix at level %u", l);
    CHECK(B.group_prefix[l + 1] - B.group_prefix[l] == B.slices[l], "group_prefix at level %u", l);
    if (S.rp.slot[l] >= 0) {
      CHECK((uint32_t)S.rp.slot[l] == slots, "replay slot of level %u", l);
      CHECK(in_sweep && lv.hashed[l] && pow2(lv.size[l]) && lv.size[l] <= 65536u, "replayed level %u: 16-bit rows of a hashed level", l);
      ++slots;
    }
  }
  CHECK(slots == S.n_replay, "n_replay %u", S.n_replay);
  CHECK(B.job_prefix[0] == 0 && B.group_prefix[0] == 0, "prefixes start at 0");
  for (uint32_t l = L; l < DNS_MAX_LEVELS; ++l) {
    CHECK(B.job_prefix[l + 1] == B.job_prefix[L] && B.group_prefix[l + 1] == B.group_prefix[L], "prefix tail at %u", l);
    CHECK(S.rp.slot[l] == -1, "replay slot past the levels");
  }
  // ---- the XCD-major grid: eight times the fullest XCD, and every (level, chunk, slice) is some workgroup's, once
  {
    uint32_t per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t l = 0; l < L; ++l)
      for (uint32_t g = B.group_prefix[l]; g < B.group_prefix[l + 1]; ++g) per_xcd[g & 7u] += B.chunks[l];
    uint32_t mx = 0;
    for (int i = 0; i < 8; ++i) mx = per_xcd[i] > mx ? per_xcd[i] : mx;
    const uint32_t jobs = B.job_prefix[L];
    CHECK(B.xcd_major == 1 && S.sweep.grid == 8 * mx && S.sweep.grid >= jobs, "sweep grid %u, %u jobs", S.sweep.grid, jobs);
    std::vector<uint8_t> seen(jobs, 0);
    uint32_t n_seen = 0;
    for (uint32_t b = 0; b < S.sweep.grid; ++b) {
      uint32_t l, chunk, slice;
      if (!sweep_job_of(B, b, l, chunk, slice)) continue;
      CHECK(chunk < B.chunks[l] && slice < B.slices[l], "workgroup %u -> level %u chunk %u slice %u", b, l, chunk, slice);
      if (!(chunk < B.chunks[l] && slice < B.slices[l])) continue;
      const uint32_t j = B.job_prefix[l] + chunk * B.slices[l] + slice;
      CHECK(!seen[j], "job %u twice", j);
      seen[j] = 1;
      ++n_seen;
    }
    CHECK(n_seen == jobs, "%u of %u sweep jobs have a workgroup", n_seen, jobs);
  }
  // ---- launches
  if (issued) {
    check_launch_shape("transpose", S.transpose, 0);
    CHECK(S.dg_tiles >= 1 && (uint64_t)S.transpose.grid * S.dg_tiles * 256u >= P, "transpose covers %u points", P);
  }
  if (S.sweep.grid) {
    check_launch_shape("sweep", S.sweep, ATTR_BINNED_LDS);
    CHECK(S.sweep.lds == B.chunk_rows * 16u, "sweep lds %u", S.sweep.lds);
  }
  CHECK(S.lds_ok == (S.list_bins.lds <= (uint32_t)MAX_DYN_LDS), "lds_ok");
  if (S.lists) {
    const ListPlan& lp = S.lp;
    CHECK(P < (1u << 30) && lp.n >= 1 && lp.n <= L, "list levels %u", lp.n);
    CHECK(n_lists < 8192u, "%u lists: the scan kernel holds 8191", n_lists);
    CHECK(lp.chunk_shift >= 10 && lp.chunk_shift <= 13 && lp.chunk_shift == k.list_shift, "list shift %u", lp.chunk_shift);
    CHECK(lp.tiles >= 1 && lp.tiles <= 32 && lp.slices >= 1 && lp.target >= 1, "tiles %u slices %u target %u", lp.tiles, lp.slices, lp.target);
    CHECK(lp.max_jobs >= n_lists, "max_jobs %u < %u lists", lp.max_jobs, n_lists);
    CHECK(lp.balanced == (lp.n_dense ? 1u : 0u), "balanced");
    uint32_t nd = 0;
    for (uint32_t i = 0; i < lp.n; ++i) {
      CHECK(lp.qoff[i + 1] - lp.qoff[i] == lp.chunks[i] && lp.chunks[i] >= 1 && lp.chunks[i] <= PART_MAX_CHUNKS, "list level %u: qoff / %u chunks", i, lp.chunks[i]);
      CHECK(((uint64_t)lp.chunks[i] << lp.chunk_shift) >= lv.size[lp.level[i]], "list level %u: chunks cover the level", i);
      CHECK(lp.cap[i] % 4 == 0, "list level %u: cap %u", i, lp.cap[i]);
      // (narrowed: a caller-chosen queue_cap is taken as it is, also above 8 P -- such lists are merely never full)
      if (lp.dense[i] || !queue_cap) CHECK(lp.cap[i] <= (((uint64_t)P * 8u + 3u) & ~3ull), "list level %u: cap %u > 8 P", i, lp.cap[i]);
      else CHECK(lp.cap[i] == ((queue_cap + 3u) & ~3u), "list level %u: cap %u for queue_cap %u", i, lp.cap[i], queue_cap);
      CHECK(lp.dense[i] == (lv.hashed[lp.level[i]] ? 0u : 1u), "list level %u: dense flag", i);
      if (lp.dense[i]) {
        CHECK(lp.cap[i] >= (uint64_t)P * 8u, "dense list level %u: region %u < 8 P", i, lp.cap[i]);
        CHECK(nd < lp.n_dense && lp.dense_idx[nd] == i, "dense_idx");
        ++nd;
      }
    }
    CHECK(nd == lp.n_dense, "n_dense");
    if (issued) {
      check_launch_shape("list count", S.list_count, 0);
      CHECK(S.list_count.grid_y == lp.n && (uint64_t)S.list_count.grid * LIST_THREADS * lp.tiles >= P, "list count grid");
      if (lp.balanced) {
        check_launch_shape("list scan", S.list_scan, 0);
        check_launch_shape("list write", S.list_write, 0);
        CHECK(S.list_scan.grid == 1 && S.list_scan.block == 1024, "scan: one workgroup of 1024");
        CHECK(S.list_write.grid == S.list_count.grid && S.list_write.grid_y == lp.n_dense, "list write grid");
      }
      if (S.lds_ok) check_launch_shape("list bins", S.list_bins, (uint32_t)MAX_DYN_LDS);
      CHECK(S.list_bins.grid == (lp.balanced ? lp.max_jobs : n_lists * lp.slices), "list bins grid %u", S.list_bins.grid);
      CHECK(S.list_bins.lds == (16u << lp.chunk_shift) + (lp.balanced ? 4u * (n_lists + 1u) : 0u), "list bins lds %u", S.list_bins.lds);
    }
  } else {
    CHECK(S.lds_ok, "refusal without lists");
  }
  if (S.part) {
    const PartPlan& pp = S.pp;
    CHECK(pp.n >= 1 && pp.n <= L && pp.chunk_shift == 13 && pp.slices >= 1, "partition levels %u", pp.n);
    for (uint32_t i = 0; i < pp.n; ++i) {
      CHECK(pp.qoff[i + 1] - pp.qoff[i] == pp.chunks[i] && pp.chunks[i] >= 2 && pp.chunks[i] <= PART_MAX_CHUNKS, "queue level %u: qoff / %u chunks", i, pp.chunks[i]);
      CHECK(((uint64_t)pp.chunks[i] << 13) >= lv.size[pp.level[i]], "queue level %u: chunks cover the level", i);
      CHECK(pp.cap[i] % 4 == 0 && pp.cap[i] >= 1, "queue level %u: cap %u", i, pp.cap[i]);
    }
    if (issued) {
      check_launch_shape("partition", S.partition, 0);
      check_launch_shape("queue", S.queue, ATTR_BINNED_LDS);
      CHECK((uint64_t)S.partition.grid * PART_THREADS >= P, "partition covers %u points", P);
      CHECK(S.queue.grid == pp.qoff[pp.n] * pp.slices && S.queue.lds == ATTR_BINNED_LDS, "queue grid %u", S.queue.grid);
    }
  }
}

// ---- one line per configuration: the numbers a launch shows, and a hash over every field of the plan that a kernel reads
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(uint64_t v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xffu;
      h *= 1099511628211ull;
    }
  }
  void add(const ScatterLaunch& L) { add(L.grid); add(L.grid_y); add(L.block); add(L.lds); }
};

static uint64_t plan_hash(uint32_t L, const ScatterPlan& S) {
  Fnv f;
  f.add(S.part); f.add(S.lists);
  f.add(S.gmax); f.add(S.qcount); f.add(S.queues); f.add(S.lcount); f.add(S.lwords); f.add(S.replay); f.add(S.total);
  if (S.part) {
    const PartPlan& p = S.pp;
    f.add(p.n); f.add(p.chunk_shift); f.add(p.slices); f.add(p.qoff[DNS_MAX_LEVELS]);
    for (uint32_t i = 0; i < DNS_MAX_LEVELS; ++i) { f.add(p.level[i]); f.add(p.chunks[i]); f.add(p.qoff[i]); f.add(p.cap[i]); f.add(p.qbase[i]); f.add(S.in_part[i]); }
  }
  if (S.lists) {
    const ListPlan& p = S.lp;
    f.add(p.n); f.add(p.chunk_shift); f.add(p.slices); f.add(p.tiles); f.add(p.n_dense); f.add(p.balanced); f.add(p.target); f.add(p.max_jobs);
    f.add(p.qoff[DNS_MAX_LEVELS]);
    for (uint32_t i = 0; i < DNS_MAX_LEVELS; ++i) {
      f.add(p.level[i]); f.add(p.chunks[i]); f.add(p.qoff[i]); f.add(p.cap[i]); f.add(p.qbase[i]); f.add(p.dense[i]); f.add(p.dense_idx[i]); f.add(S.in_list[i]);
    }
  }
  const BinPlan& b = S.bins;
  f.add(b.n_levels); f.add(b.chunk_rows); f.add(b.strided_dense); f.add(b.dense_runs); f.add(b.xcd_major);
  for (uint32_t l = 0; l <= DNS_MAX_LEVELS; ++l) { f.add(b.job_prefix[l]); f.add(b.group_prefix[l]); }
  for (uint32_t l = 0; l < L; ++l) { f.add(b.chunks[l]); f.add(b.slices[l]); }     // (entries past the levels are not read)
  for (uint32_t l = 0; l < DNS_MAX_LEVELS; ++l) f.add((uint64_t)(int64_t)S.rp.slot[l]);
  f.add(S.n_replay); f.add(S.dg_tiles); f.add(S.clear_words); f.add(S.lds_ok);
  f.add(S.transpose); f.add(S.sweep); f.add(S.list_count); f.add(S.list_scan); f.add(S.list_write); f.add(S.list_bins); f.add(S.partition); f.add(S.queue);
  return f.h;
}

static const char* const HEADER =
    "# log2T P flags | default knobs, queue_cap 0: workspace floats, grids of sweep, list count (x), list bins, queue, list bins LDS bytes"
    " | the same, queue_cap 64 | hash over the plans of both queue_caps x every knob case";

// one plan's numbers, as they stand in a line
static std::string plan_numbers(const ScatterPlan& S) {
  char buf[128];
  snprintf(buf, sizeof(buf), "%llu %u %u %u %u %u", (unsigned long long)S.total, S.sweep.grid, S.list_count.grid, S.list_bins.grid, S.queue.grid, S.list_bins.lds);
  return buf;
}

struct KnobCase {
  const char* name;
  ScatterKnobs k;
};

static std::vector<KnobCase> knob_cases() {
  std::vector<KnobCase> v;
  v.push_back({"default", SCATTER_KNOBS_DEFAULT});
  auto with = [&](const char* name, uint32_t ScatterKnobs::*field, uint32_t value) {
    ScatterKnobs k = SCATTER_KNOBS_DEFAULT;
    k.*field = value;
    v.push_back({name, k});
  };
  with("bin_rows=1024", &ScatterKnobs::bin_rows, 1024);
  with("bin_rows=8192", &ScatterKnobs::bin_rows, 8192);
  with("bin_jobs=1", &ScatterKnobs::bin_jobs, 1);
  with("bin_jobs=65535", &ScatterKnobs::bin_jobs, 65535);
  with("bin_threads=64", &ScatterKnobs::bin_threads, 64);
  with("bin_threads=1024", &ScatterKnobs::bin_threads, 1024);
  with("dense_runs=0", &ScatterKnobs::dense_runs, 0);
  with("dense_runs=1", &ScatterKnobs::dense_runs, 1);
  with("dg_tiles=1", &ScatterKnobs::dg_tiles, 1);
  with("dg_tiles=64", &ScatterKnobs::dg_tiles, 64);
  with("list_shift=10", &ScatterKnobs::list_shift, 10);
  with("list_shift=13", &ScatterKnobs::list_shift, 13);
  with("list_threads=64", &ScatterKnobs::list_threads, 64);
  with("list_threads=1024", &ScatterKnobs::list_threads, 1024);
  with("list_tiles=1", &ScatterKnobs::list_tiles, 1);
  with("list_tiles=32", &ScatterKnobs::list_tiles, 32);
  with("list_jobs=1", &ScatterKnobs::list_jobs, 1);
  with("list_jobs=65535", &ScatterKnobs::list_jobs, 65535);
  with("list_dense_min=1", &ScatterKnobs::list_dense_min, 1);
  with("list_dense_min=2147483647", &ScatterKnobs::list_dense_min, 0x7fffffffu);
  return v;
}

// the sweep; plan_of(P, lv, flags, queue_cap, knobs) builds the plan under test.  One line per (grid, P, form): the default knobs'
// numbers for either queue_cap, and one hash that folds the hash of every plan of that line (2 queue_caps x the knob cases), so
// the expected file stays a few hundred lines and still pins every swept plan.  With every_plan, one line per plan instead.
static size_t g_plans = 0;
template <typename PlanFn>
static std::vector<std::string> sweep_lines(const std::vector<KnobCase>& cases, PlanFn plan_of, bool check, bool every_plan) {
  static const uint32_t Ps[] = {0u, 1u, 63u, 1023u, 1025u, 5000u, 262144u, 1u << 30};
  static const uint32_t grids[][2] = {{12, 64}, {14, 200}, {16, 592}, {20, 231}};
  static const uint32_t forms[] = {DNS_SCATTER_AUTO, DNS_SCATTER_ATOMIC, DNS_SCATTER_BINNED, DNS_SCATTER_QUEUES, DNS_SCATTER_AUTO | DNS_SCATTER_REPLAY,
                                   DNS_SCATTER_BINNED | DNS_SCATTER_LISTS, DNS_SCATTER_AUTO | DNS_SCATTER_LISTS};
  static const uint32_t caps[] = {0u, 64u};
  std::vector<std::string> lines;
  char buf[256];
  for (const auto& g : grids) {
    DnsGridMeta meta;
    // the level table as ops.GridMeta asks for it: 16 levels, 2 features, base resolution 16, per-level scale from the finest
    const double pls = exp2(log2((double)g[1] / 16.0) / 15.0);
    if (!grid_meta_fill(&meta, 16, 2, g[0], 16, pls)) {
      printf("FAIL grid (%u, %u): table too large\n", g[0], g[1]);
      ++g_fail;
      continue;
    }
    const GridLevels lv = to_levels(&meta);
    for (uint32_t P : Ps)
      for (uint32_t flags : forms) {
        Fnv fold;
        std::string numbers;
        for (uint32_t cap : caps)
          for (const KnobCase& kc : cases) {
            const ScatterPlan S = plan_of(P, lv, flags, cap, kc.k);
            const uint64_t h = plan_hash(lv.n_levels, S);
            fold.add(h);
            ++g_plans;
            if (&kc == &cases[0]) numbers += " | " + plan_numbers(S);
            snprintf(buf, sizeof(buf), "%s %u %u 0x%x %u | %s | %016llx", kc.name, g[0], P, flags, cap, plan_numbers(S).c_str(), (unsigned long long)h);
            if (every_plan) lines.push_back(buf);
            if (check) {
              g_cfg = buf;
              check_plan(P, lv, flags, cap, kc.k, S);
            }
          }
        snprintf(buf, sizeof(buf), "%u %u 0x%x%s | %016llx", g[0], P, flags, numbers.c_str(), (unsigned long long)fold.h);
        if (!every_plan) lines.push_back(buf);
      }
  }
  return lines;
}

int main(int argc, char** argv) {
  const char* expect = nullptr;
  const char* write = nullptr;
  bool every_plan = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--plans")) every_plan = true;
    if (i + 1 < argc && !strcmp(argv[i], "--expect")) expect = argv[i + 1];
    if (i + 1 < argc && !strcmp(argv[i], "--write")) write = argv[i + 1];
  }
  const std::vector<std::string> lines = sweep_lines(knob_cases(), scatter_plan, true, every_plan && !expect && !write);
  if (!expect && !write) {
    if (!every_plan) puts(HEADER);
    for (const std::string& s : lines) puts(s.c_str());
  }
  if (write) {
    FILE* f = fopen(write, "w");
    if (!f) { printf("cannot write %s\n", write); return 2; }
    fprintf(f, "%s\n", HEADER);
    for (const std::string& s : lines) fprintf(f, "%s\n", s.c_str());
    fclose(f);
  }
  size_t n_diff = 0;
  if (expect) {
    FILE* f = fopen(expect, "r");
    if (!f) { printf("cannot read %s\n", expect); return 2; }
    char buf[512];
    size_t i = 0;
    while (fgets(buf, sizeof(buf), f)) {
      buf[strcspn(buf, "\n")] = 0;
      if (buf[0] == '#' || !buf[0]) continue;
      if (i >= lines.size() || lines[i] != buf) {
        if (++n_diff <= 10) printf("DIFFERS at line %zu:\n  expected %s\n  got      %s\n", i, buf, i < lines.size() ? lines[i].c_str() : "(nothing)");
      }
      ++i;
    }
    fclose(f);
    if (i != lines.size()) {
      printf("DIFFERS: %zu lines expected, %zu produced\n", i, lines.size());
      ++n_diff;
    }
  }
  printf("scatter_plan_check: %zu plans, %d failed conditions%s\n", g_plans, g_fail,
         expect ? (n_diff ? ", DIFFERENT from the expected plans" : ", all equal to the expected plans") : "");
  return g_fail || n_diff ? 1 : 0;
}
