// Host launch plan of the table-gradient scatter (scatter.hip), free of HIP headers: which form carries which level, the workspace
// layout, and every launch's grid, block and dynamic LDS, computed ONCE by scatter_plan().  dns_encode_bwd_ws_floats returns the
// plan's .total, dns_encode_bwd hands the same plan to launch_table_scatter, and tools/scatter_plan_check.cpp holds it to the
// conditions the kernels rely on, under sanitizers, on a machine without a GPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/dns_hip.h"
#include "grid_levels.hpp"

namespace dns {

// The plan structs below are kernel arguments (passed by value): their layouts are part of the kernels.
struct BinPlan {
  uint32_t n_levels;
  uint32_t chunk_rows;                    // rows per chunk
  uint32_t strided_dense;                 // dense levels: one contiguous run of points per thread
  uint32_t dense_runs;                    // ... whose per-cell sums are kept in registers until the cell changes
  uint32_t job_prefix[DNS_MAX_LEVELS + 1];  // prefix sum over levels of chunks[l] * slices[l]
  uint32_t group_prefix[DNS_MAX_LEVELS + 1];  // prefix sum over levels of slices[l]: a group = one (level, slice)
  uint32_t xcd_major;                     // 1: blockIdx -> (xcd = b % 8, q = b / 8), a group's chunks adjacent in q
  uint32_t chunks[DNS_MAX_LEVELS];
  uint32_t slices[DNS_MAX_LEVELS];
};

// Row replay (DNS_SCATTER_REPLAY, see dgrid_transpose_kernel)
struct ReplayPlan {
  int32_t slot[DNS_MAX_LEVELS];                  // level -> index of its [P] uint4 plane in rows16, -1 = not replayed
};

constexpr uint32_t DG_TILES = 2;                 // 256-point tiles per workgroup of the transpose
constexpr uint32_t PART_MAX_CHUNKS = 256;      // chunks per level (8192-row chunks: T <= 2^21; the lists' 4096-row chunks: T <= 2^20)
constexpr uint32_t PART_THREADS = 256;         // points per pass-1 workgroup
constexpr uint32_t PART_ENTRIES = PART_THREADS * 8;

struct PartPlan {
  uint32_t n;                                  // levels handled by the partition form
  uint32_t level[DNS_MAX_LEVELS];              // their level indices
  uint32_t chunks[DNS_MAX_LEVELS];             // 8192-row chunks of the level
  uint32_t qoff[DNS_MAX_LEVELS + 1];           // first queue of the level (prefix sum of chunks)
  uint32_t cap[DNS_MAX_LEVELS];                // entries per queue of the level
  uint64_t qbase[DNS_MAX_LEVELS];              // float offset of the level's first queue
  uint32_t chunk_shift;                        // log2(rows per chunk) = 13
  uint32_t slices;                             // pass-2 workgroups per queue
};

constexpr uint32_t LIST_THREADS = 256;           // points per pass-1 workgroup
constexpr uint32_t LIST_TILES = 8;               // 256-point tiles per pass-1 workgroup (<= 32: one bit each; DNS_LIST_TILES)

struct ListPlan {
  uint32_t n;                                  // levels handled by the pair-list form
  uint32_t level[DNS_MAX_LEVELS];
  uint32_t chunks[DNS_MAX_LEVELS];
  uint32_t qoff[DNS_MAX_LEVELS + 1];           // first list of the level (prefix sum of chunks)
  uint32_t cap[DNS_MAX_LEVELS];                // entries per list of the level
  uint64_t qbase[DNS_MAX_LEVELS];              // word offset of the level's first list
  uint32_t chunk_shift;                        // log2(rows per chunk) = 13
  uint32_t slices;                             // pass-2 workgroups per list (static slicing: hashed levels only)
  uint32_t tiles;                              // 256-point tiles per pass-1 workgroup
  // Dense levels (round 4, second half): their lists fill by where the rays are, so (a) they are sized EXACTLY -- a counting
  // sweep, a scan kernel that places each chunk's list inside the level's region (at most 8 entries per point), a writing sweep --
  // and (b) pass 2 cuts every list into jobs of `target` entries from the actual counts (`balanced`: the scan kernel's job
  // prefix, searched in LDS) instead of a fixed number of slices per list.
  uint32_t dense[DNS_MAX_LEVELS];              // 1: exact-size lists; qbase = the level's region, cap = its size (8 P)
  uint32_t n_dense;
  uint32_t dense_idx[DNS_MAX_LEVELS];          // list-level indices of the dense levels (grid.y of the writing sweep)
  uint32_t balanced;                           // 1: jobs from the scan kernel
  uint32_t target;                             // entries per balanced job
  uint32_t max_jobs;                           // upper bound of the balanced job count (grid of pass 2)
};

// A measurement knob: the integer in environment variable `name`, or `fallback` unless lo <= n <= hi and n % multiple_of == 0.
// `after`: the integer is the one behind the value's first `after` character ("3,2"); `set`: whether the variable exists at all.
inline uint32_t env_u32(const char* name, long lo, long hi, long multiple_of, uint32_t fallback, char after = 0, bool* set = nullptr) {
  const char* e = getenv(name);
  if (set) *set = e != nullptr;
  if (e && after) {
    e = strchr(e, after);
    if (e) ++e;
  }
  const long n = e ? atol(e) : 0;
  return n >= lo && n <= hi && n % multiple_of == 0 ? (uint32_t)n : fallback;
}

// The scatter's measurement knobs; 0 = the default where one is named.  scatter_plan() takes them as an argument (the host check
// sweeps them); the library reads the environment once, scatter_knobs_env().
struct ScatterKnobs {
  uint32_t bin_rows;        // DNS_BIN_ROWS 1024..8192: rows per chunk of the sweep form (0: 8192)
  uint32_t bin_jobs;        // DNS_BIN_JOBS 1..65535: workgroups of the sweep form (0: bin_target_jobs)
  uint32_t bin_threads;     // DNS_BIN_THREADS 64..1024, whole waves: its workgroup size (1024)
  uint32_t dense_runs;      // DNS_DENSE_RUNS: 0 only for a leading '0' (1)
  uint32_t dg_tiles;        // DNS_DG_TILES 1..64: 256-point tiles per workgroup of the transpose (DG_TILES)
  uint32_t list_shift;      // DNS_LIST_SHIFT 10..13: log2 rows per chunk of the lists (12)
  uint32_t list_threads;    // DNS_LIST_THREADS 64..1024, whole waves: pass-2 workgroup size (0: list_threads)
  uint32_t list_tiles;      // DNS_LIST_TILES 1..32: 256-point tiles per pass-1 workgroup (0: LIST_TILES)
  uint32_t list_jobs;       // DNS_LIST_JOBS 1..65535: pass-2 workgroups of the pair-list form (1536)
  uint32_t list_dense_min;  // DNS_LIST_DENSE_MIN >= 1: see list_plan (6; 0x7fffffff = none)
};
constexpr ScatterKnobs SCATTER_KNOBS_DEFAULT = {0u, 0u, 1024u, 1u, DG_TILES, 12u, 0u, 0u, 1536u, 6u};

inline const ScatterKnobs& scatter_knobs_env() {
  static const ScatterKnobs k = [] {
    ScatterKnobs v;
    v.bin_rows = env_u32("DNS_BIN_ROWS", 1024, 8192, 1, 0);
    v.bin_jobs = env_u32("DNS_BIN_JOBS", 1, 65535, 1, 0);
    v.bin_threads = env_u32("DNS_BIN_THREADS", 64, 1024, 64, 1024);
    const char* runs = getenv("DNS_DENSE_RUNS");
    v.dense_runs = runs && runs[0] == '0' ? 0u : 1u;
    v.dg_tiles = env_u32("DNS_DG_TILES", 1, 64, 1, DG_TILES);
    v.list_shift = env_u32("DNS_LIST_SHIFT", 10, 13, 1, 12);
    v.list_threads = env_u32("DNS_LIST_THREADS", 64, 1024, 64, 0);
    v.list_tiles = env_u32("DNS_LIST_TILES", 1, 32, 1, 0);
    v.list_jobs = env_u32("DNS_LIST_JOBS", 1, 65535, 1, 1536);
    v.list_dense_min = env_u32("DNS_LIST_DENSE_MIN", 1, 0xffffffffl, 1, 6);
    return v;
  }();
  return k;
}

inline uint32_t list_threads(const ScatterKnobs& k, uint32_t shift) { return k.list_threads ? k.list_threads : 1024u >> (13u - shift); }

// dense levels of at least k.list_dense_min 8192-row chunks go through (exact-size) lists, smaller ones through the run-combining
// sweep.
// Lists: 4 pairs per point-level spread over the level's chunks.  Hashed levels get the uniform-hash expectation + 1/8 slack,
// dense levels (spatially clustered points) four times the expectation; what does not fit takes the atomics fallback.
inline bool list_plan(const GridLevels& lv, uint32_t P, uint32_t queue_cap, const ScatterKnobs& k, ListPlan& lp) {
  lp.n = 0;
  lp.n_dense = 0;
  for (uint32_t i = 0; i < DNS_MAX_LEVELS; ++i) lp.dense[i] = lp.dense_idx[i] = 0;
  lp.chunk_shift = k.list_shift;
  uint32_t queues = 0;
  uint64_t words = 0;
  if (P >= (1u << 30)) return false;             // {point, pair} in 32 bits
  for (uint32_t l = 0; l < lv.n_levels; ++l) {
    const uint32_t chunks = (lv.size[l] + (1u << lp.chunk_shift) - 1u) >> lp.chunk_shift;
    if (lv.size[l] <= 8192u || chunks > PART_MAX_CHUNKS) continue;   // one-chunk levels stay with the sweep
    if (lv.hashed[l] && (lv.size[l] & (lv.size[l] - 1u))) continue;
    const bool dense = !lv.hashed[l];
    if (dense && ((lv.size[l] + 8191u) >> 13) < k.list_dense_min) continue;   // small dense levels: the run-combining sweep
    const uint64_t expect = ((uint64_t)P * 4u + chunks - 1) / chunks;
    uint64_t cap = expect + expect / 8u + 4096u;
    if (cap > (uint64_t)P * 8u) cap = (uint64_t)P * 8u;          // a level emits at most 8 entries per point
    if (queue_cap) cap = queue_cap;                               // caller-chosen capacity (tests: the overflow fallback)
    if (dense) cap = (uint64_t)P * 8u;                            // exact lists: the level's whole region
    cap = (cap + 3u) & ~3ull;
    if (cap > 0x7FFFFFFFull) return false;
    const uint32_t i = lp.n++;
    lp.level[i] = l;
    lp.chunks[i] = chunks;
    lp.qoff[i] = queues;
    lp.cap[i] = (uint32_t)cap;
    lp.qbase[i] = words;
    lp.dense[i] = dense ? 1u : 0u;
    if (dense) lp.dense_idx[lp.n_dense++] = i;
    queues += chunks;
    words += dense ? cap : (uint64_t)chunks * cap;
  }
  lp.qoff[lp.n] = queues;
  for (uint32_t i = lp.n; i < DNS_MAX_LEVELS; ++i) {
    lp.level[i] = 0;
    lp.chunks[i] = 0;
    lp.cap[i] = 0;
    lp.qbase[i] = words;
    lp.qoff[i + 1] = queues;
  }
  if (!lp.n || queues >= 8192u) return false;
  lp.slices = (k.list_jobs + queues - 1) / queues;
  if (lp.slices < 1) lp.slices = 1;
  lp.balanced = lp.n_dense ? 1u : 0u;
  lp.target = 16u * list_threads(k, lp.chunk_shift);                 // 16 entries per thread
  uint64_t mj = queues;                                           // every list's last, partial job
  for (uint32_t i = 0; i < lp.n; ++i) mj += (lp.dense[i] ? (uint64_t)lp.cap[i] : (uint64_t)lp.chunks[i] * lp.cap[i]) / lp.target;
  if (mj > 0x7FFFFFFFull) return false;
  lp.max_jobs = (uint32_t)mj;
  lp.tiles = k.list_tiles ? k.list_tiles : LIST_TILES;
  return true;
}

inline uint64_t list_words(const ListPlan& lp) {
  uint64_t w = 0;
  for (uint32_t i = 0; i < lp.n; ++i) w += lp.dense[i] ? (uint64_t)lp.cap[i] : (uint64_t)lp.chunks[i] * lp.cap[i];
  return w;
}

// Levels with at least PART_MIN_CHUNKS chunks go through the partition form; hashed levels get the uniform-hash
// expectation + 1/8 slack per queue, dense levels (spatially clustered points) twice the expectation.
constexpr uint32_t PART_MIN_CHUNKS = 16;

inline bool part_plan(const GridLevels& lv, uint32_t P, uint32_t min_chunks, uint32_t queue_cap, PartPlan& pp,
                      const bool* skip = nullptr) {
  pp.n = 0;
  pp.chunk_shift = 13;
  uint32_t queues = 0;
  uint64_t floats = 0;
  for (uint32_t l = 0; l < lv.n_levels; ++l) {
    const uint32_t chunks = (lv.size[l] + 8191u) >> 13;
    if (chunks < min_chunks || chunks > PART_MAX_CHUNKS || (skip && skip[l])) continue;
    if (lv.hashed[l] && (lv.size[l] & (lv.size[l] - 1u))) continue;
    const uint64_t expect = ((uint64_t)P * 8u + chunks - 1) / chunks;
    uint64_t cap = (lv.hashed[l] ? expect + expect / 8u : 2u * expect) + 4096u;
    if (queue_cap) cap = queue_cap;                               // caller-chosen capacity (tests: the overflow fallback)
    cap = (cap + 3u) & ~3ull;
    if (cap > 0x7FFFFFFFull) return false;
    const uint32_t i = pp.n++;
    pp.level[i] = l;
    pp.chunks[i] = chunks;
    pp.qoff[i] = queues;
    pp.cap[i] = (uint32_t)cap;
    pp.qbase[i] = floats;
    queues += chunks;
    floats += (uint64_t)chunks * cap * 3u;
  }
  pp.qoff[pp.n] = queues;
  for (uint32_t i = pp.n; i < DNS_MAX_LEVELS; ++i) {
    pp.level[i] = 0;
    pp.chunks[i] = 0;
    pp.cap[i] = 0;
    pp.qbase[i] = floats;
    pp.qoff[i + 1] = queues;
  }
  if (!pp.n) return false;
  pp.slices = (1024u + queues - 1) / queues;
  if (pp.slices < 1) pp.slices = 1;
  return true;
}

inline uint64_t part_floats(const PartPlan& pp) {
  uint64_t f = 0;
  for (uint32_t i = 0; i < pp.n; ++i) f += (uint64_t)pp.chunks[i] * pp.cap[i] * 3u;
  return f;
}

inline uint32_t part_min_chunks(uint32_t flags) {
  const uint32_t form = flags & DNS_SCATTER_MASK;
  if (form == DNS_SCATTER_QUEUES) return 2u;                   // every multi-chunk level through the queues
  if (form == DNS_SCATTER_BINNED) return PART_MAX_CHUNKS + 1u;  // none
  return PART_MIN_CHUNKS;
}

// workgroups of the sweep form (DNS_BIN_JOBS overrides, for measurement): ~1280 when it carries the hashed levels too (above),
// one round of the chip when only the dense levels are left to it (every job zeroes and flushes a whole chunk)
inline uint32_t bin_target_jobs(const ScatterKnobs& k, bool lists) { return k.bin_jobs ? k.bin_jobs : (lists ? 512u : 1280u); }

// Workspace of the table scatter, in floats: [level-major gradient copy | max word, non-finite flag, pad | list counters | queue
// counters + queues of the partition form | lists of the pair-list form | replayed rows (16-byte aligned)]
struct ScatterWs {
  bool part, lists;
  PartPlan pp;
  ListPlan lp;
  bool in_part[DNS_MAX_LEVELS], in_list[DNS_MAX_LEVELS];
  uint64_t gmax, qcount, queues, lcount, lwords, replay, total;
};
inline ScatterWs scatter_ws(uint32_t P, const GridLevels& lv, uint32_t flags, uint32_t queue_cap, const ScatterKnobs& k) {
  ScatterWs w = {};
  w.lists = ((flags & DNS_SCATTER_LISTS) || (flags & DNS_SCATTER_MASK) == DNS_SCATTER_AUTO) && list_plan(lv, P, queue_cap, k, w.lp);
  if (w.lists)
    for (uint32_t i = 0; i < w.lp.n; ++i) w.in_list[w.lp.level[i]] = true;
  w.part = part_plan(lv, P, part_min_chunks(flags), queue_cap, w.pp, w.in_list);
  if (w.part)
    for (uint32_t i = 0; i < w.pp.n; ++i) w.in_part[w.pp.level[i]] = true;
  uint64_t n = (uint64_t)P * lv.n_levels * 2;
  w.gmax = n;
  n += 4;
  w.lcount = n;                                  // directly behind the max words: one fill clears max words, counts and cursors
  if (w.lists) n += (uint64_t)4u * w.lp.qoff[w.lp.n] + 4u;      // [counts | cursors | list starts | job prefix (+1)]
  w.qcount = n;
  if (w.part) n += (uint64_t)DNS_MAX_LEVELS * PART_MAX_CHUNKS;
  w.queues = n;
  if (w.part) n += part_floats(w.pp);
  w.lwords = n;
  if (w.lists) n += list_words(w.lp);
  n = (n + 3u) & ~(uint64_t)3u;
  w.replay = n;
  if (flags & DNS_SCATTER_REPLAY) n += (uint64_t)P * lv.n_levels * 4;
  w.total = n;
  return w;
}

// One launch of the scatter: grid (x, y), workgroup size, dynamic LDS bytes.  All zero: not issued.
struct ScatterLaunch {
  uint32_t grid, grid_y, block, lds;
};

// Everything dns_encode_bwd's table scatter does on the host, as one value: the workspace layout and per-form plans of ScatterWs,
// the sweep form's BinPlan, the replay slots, and the up to eight kernel launches in order (transpose; sweep -- skipped when every
// level went to lists or queues --; lists: counting sweep, scan + writing sweep when balanced, bins; queues: partition, queue).
struct ScatterPlan : ScatterWs {
  BinPlan bins;
  ReplayPlan rp;
  uint32_t n_replay;                             // planes of replayed rows behind .replay (each P uint4)
  uint32_t dg_tiles;                             // 256-point tiles per workgroup of the transpose
  uint32_t clear_words;                          // words cleared from .gmax on before the transpose
  bool lds_ok;                                   // false: the pair-list bins exceed MAX_DYN_LDS (refused by dns_encode_bwd)
  ScatterLaunch transpose, sweep, list_count, list_scan, list_write, list_bins, partition, queue;
};

inline ScatterPlan scatter_plan(uint32_t P, const GridLevels& lv, uint32_t flags, uint32_t queue_cap, const ScatterKnobs& k) {
  ScatterPlan S = {};
  // multi-chunk levels: pair lists (DNS_SCATTER_LISTS), else the partition form for levels of large tables
  // (DNS_SCATTER_QUEUES sends every multi-chunk level there, _BINNED none)
  static_cast<ScatterWs&>(S) = scatter_ws(P, lv, flags, queue_cap, k);
  const ScatterWs& W = S;
  BinPlan& plan = S.bins;
  plan.n_levels = lv.n_levels;
  plan.chunk_rows = k.bin_rows ? k.bin_rows : 8192u;
  plan.xcd_major = 1u;
  plan.strided_dense = 1u;
  plan.dense_runs = k.dense_runs;
  bool in_part[DNS_MAX_LEVELS];
  for (uint32_t l = 0; l < DNS_MAX_LEVELS; ++l) in_part[l] = W.in_part[l] || W.in_list[l];
  uint32_t chunk_of[DNS_MAX_LEVELS];
  for (uint32_t l = 0; l < lv.n_levels; ++l) chunk_of[l] = in_part[l] ? 0u : (lv.size[l] + plan.chunk_rows - 1) / plan.chunk_rows;
  // ~1280 workgroups in all (five per CU; one fits a CU at a time): a dense level's jobs are sliced 4x (one chunk) / 2x finer,
  // see below.  Round 2 aimed at 512 (two rounds): stand-alone the kernel does not care (221-224 us at 5, 10 slices per hashed
  // level), but inside the two-stream step finer jobs leave fewer CUs idle behind the last round and interleave better with
  // the other stream's kernels: 2.08-2.10 -> 2.05-2.07 ms per step at 10-12 slices, worse again at 16-20
  uint32_t weight = 0;
  for (uint32_t l = 0; l < lv.n_levels; ++l) weight += chunk_of[l] * (lv.hashed[l] ? 1u : (chunk_of[l] == 1 ? 4u : 2u));
  if (weight == 0) weight = 1;
  uint32_t ns = (bin_target_jobs(k, W.lists) + weight - 1) / weight;
  if (ns < 1) ns = 1;
  const uint32_t max_ns = (P + k.bin_threads - 1) / k.bin_threads;   // at least ~one point per thread
  if (ns > max_ns) ns = max_ns ? max_ns : 1;
  uint32_t jobs = 0, groups = 0;
  uint32_t per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t l = 0; l < lv.n_levels; ++l) {
    plan.chunks[l] = chunk_of[l];
    // dense (coarse) levels: every corner of every point lands in the chunk -> ~4x the work per point
    uint32_t nsl = lv.hashed[l] ? ns : ns * (chunk_of[l] == 1 ? 4u : 2u);
    if (nsl > max_ns) nsl = max_ns ? max_ns : 1;
    plan.slices[l] = nsl;
    plan.job_prefix[l] = jobs;
    plan.group_prefix[l] = groups;
    for (uint32_t g = groups; g < groups + nsl; ++g) per_xcd[g & 7u] += chunk_of[l];
    jobs += chunk_of[l] * nsl;
    groups += nsl;
  }
  for (uint32_t l = lv.n_levels; l <= DNS_MAX_LEVELS; ++l) {
    plan.job_prefix[l] = jobs;
    plan.group_prefix[l] = groups;
  }
  if (plan.xcd_major) {
    uint32_t mx = 0;
    for (int i = 0; i < 8; ++i) mx = per_xcd[i] > mx ? per_xcd[i] : mx;
    jobs = 8u * mx;                                          // padded: workgroups past an XCD's last job exit at once
  }
  const size_t lds_bytes = (size_t)8192u * 2 * sizeof(unsigned long long);          // queue / list kernels: 8192-row chunks
  const size_t bin_lds = (size_t)plan.chunk_rows * 2 * sizeof(unsigned long long);
  // row replay: hashed levels of <= 2^16 rows that this (binned) form handles in more than one chunk
  ReplayPlan& rp = S.rp;
  uint32_t& n_replay = S.n_replay;
  for (uint32_t l = 0; l < DNS_MAX_LEVELS; ++l) {
    const bool yes = (flags & DNS_SCATTER_REPLAY) && l < lv.n_levels && lv.hashed[l] && !in_part[l] && lv.size[l] <= 65536u && chunk_of[l] > 1u;
    rp.slot[l] = yes ? (int32_t)n_replay++ : -1;
  }

  // the launches, in the order launch_table_scatter issues them
  const uint32_t blocks = (P + 255) / 256;
  S.dg_tiles = k.dg_tiles;
  S.transpose = {(blocks + k.dg_tiles - 1) / k.dg_tiles, 1u, 256u, 0u};
  S.sweep = {jobs, 1u, k.bin_threads, (uint32_t)bin_lds};
  S.clear_words = 4 + (W.lists ? 2u * W.lp.qoff[W.lp.n] : 0u);                   // max word, non-finite flag, pad; list counts and cursors
  S.lds_ok = true;
  if (W.lists) {
    const ListPlan& lp = W.lp;
    const uint32_t n_lists = lp.qoff[lp.n];
    const uint32_t gx = (P + LIST_THREADS * lp.tiles - 1) / (LIST_THREADS * lp.tiles);
    S.list_count = {gx, lp.n, LIST_THREADS, 0u};
    size_t bins_lds = lds_bytes >> (13u - lp.chunk_shift);
    uint32_t jobs2 = n_lists * lp.slices;
    if (lp.balanced) {
      S.list_scan = {1u, 1u, 1024u, 0u};
      S.list_write = {gx, lp.n_dense, LIST_THREADS, 0u};
      bins_lds += (size_t)4u * (n_lists + 1u);
      jobs2 = lp.max_jobs;
    }
    S.lds_ok = bins_lds <= (size_t)MAX_DYN_LDS;
    S.list_bins = {jobs2, 1u, list_threads(k, lp.chunk_shift), (uint32_t)bins_lds};
  }
  if (W.part) {
    S.partition = {(P + PART_THREADS - 1) / PART_THREADS, 1u, PART_THREADS, 0u};
    S.queue = {W.pp.qoff[W.pp.n] * W.pp.slices, 1u, 1024u, (uint32_t)lds_bytes};
  }
  return S;
}

}  // namespace dns
