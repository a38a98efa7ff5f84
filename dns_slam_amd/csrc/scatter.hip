// Table-gradient scatter of the hash grid (tcnn kernel_grid_backward's d_table): the level-major gradient copy, the LDS-bin sweep,
// the partition / queue pair, the three pair-list kernels, and launch_table_scatter, which issues what a ScatterPlan
// (scatter_plan.hpp: forms per level, workspace layout, grids and LDS sizes) says.  Called by dns_encode_bwd (encode.hip).
//
// Compiled like encode.hip with -ffp-contract=off: the cell, fraction and corner weights of a point are the encoder's own functions
// (dev_encode.hpp: grid_cell, corner_weight, pair_weights), and the corner rows formed here from the cell must be the forward's.
#include <type_traits>
#include "common.hpp"
#include "dev_encode.hpp"
#include "scatter_plan.hpp"

namespace dns {

// ------------------------------------------------------------------------------------------------
// Table gradient by LDS binning (float64 bins in the binned kernel, 64-bit fixed point in the queue kernel).
//
// Per-corner global atomics (one lane = one random row) run ~17x below the coalesced atomic rate on gfx950
// and serialise on the 4096-cell coarse levels.  Instead a workgroup owns one CHUNK of one level (8192 rows held
// in LDS), sweeps a slice of the points, recomputes that level's 8 corner rows per point (cheap integer math)
// and accumulates the corners that fall in its chunk; the chunk then leaves as fully coalesced global float
// atomics (256 B per wave instruction, the full-rate shape).
//
// The LDS accumulators are 64 bits wide, never fp32: measured on MI355X (tools/lds_atomic_rate.hip) ds_add_f32 retires
// ~1 lane per 3 cycles per CU (195 cycles per wave instruction, 0.2 T lane-atomics/s chip-wide) while ds_add_u64 takes 11.9
// cycles per wave instruction (3.3 T/s) and ds_add_f64 21.6.  (fp32 bins over 16 384-row chunks -- half the re-hashing --
// were measured in round 2: 476 us against 312 us per 262 144 points.)  Round 1 added every contribution w*g as an integer
// (scaled by a power of two chosen from max|dL/dy| of the launch so the fp32 product converts to int64 exactly): exact,
// order-independent sums, at 11 vector instructions per converted value in a VALU-bound kernel.  The binned kernel now adds
// the fp32 product into a float64 bin (ds_add_f64): 276 us, sums good to ~1e-16 whatever the order; the queue kernel (large
// tables) keeps the fixed-point form.

// d_grid rows [P, ld] (32 contiguous floats per point) -> level-major [L][P] float2, so that a binned job reads
// only its level's 8 bytes per point; also max |d_grid| of the launch (bit pattern, atomicMax) for the fixed-point scale.
// Row replay (DNS_SCATTER_REPLAY): per hashed level of at most 2^16 rows the 8 corner rows of every point are computed HERE,
// once, and stored as eight 16-bit values (16 bytes per point and level, coalesced): the binned kernel's 8 visits per level
// then extract and compare them instead of hashing the 8 corners again in every visit.
__global__ __launch_bounds__(256) void dgrid_transpose_kernel(const float* __restrict__ d_grid, uint32_t ld, uint32_t P,
                                                              uint32_t n_levels, float2* __restrict__ dg_t,
                                                              uint32_t* __restrict__ gmax, const float* __restrict__ xin,
                                                              GridLevels lv, ReplayPlan rp, uint4* __restrict__ rows16,
                                                              uint32_t n_tiles) {
  // 256 points per workgroup through an LDS tile: rows are read as whole 128-byte lines (8 lanes x 16 B per point),
  // level planes are written as 2-KB contiguous runs (lane = point).  Row stride 34 floats keeps both sides <= 2-way.
  // A workgroup takes DG_TILES consecutive tiles: the NEXT tile's rows are requested before this tile goes through LDS and out, so
  // the read stream of one tile overlaps the write stream of the one before (one tile per workgroup ran the two phases of the
  // whole grid in lock-step: 26 us for 67 MB).
  constexpr uint32_t LDT = 34;
  __shared__ float tile[256 * LDT];
  const uint32_t nf = n_levels * 2;                  // floats per row (<= 32 with the supported 16 levels)
  const bool vec = ((ld & 3u) == 0) && ((((uintptr_t)d_grid) & 15u) == 0) && ((nf & 3u) == 0);
  float m = 0.f;
  bool bad = false;                                  // a NaN / Inf in the upstream gradient
  // all eight 16-byte loads of a thread are requested before the first is used (clamped addresses, no branch between
  // them: a guarded load per trip made every trip wait its own memory round trip)
  auto issue = [&](uint32_t p0, float4 (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t e = threadIdx.x + 256u * i;
      const uint32_t r = e >> 3, q = e & 7u;
      const uint32_t pc = min(p0 + r, P - 1u), qc = min(4u * q, nf - 4u);
      v[i] = *reinterpret_cast<const float4*>(d_grid + (size_t)pc * ld + qc);
    }
  };
  float4 v[8], vn[8];
  const uint32_t tile0 = blockIdx.x * n_tiles;
  if (vec && tile0 * 256u < P) issue(tile0 * 256u, v);
  for (uint32_t t = 0; t < n_tiles; ++t) {
    const uint32_t p0 = (tile0 + t) * 256u;
    if (p0 >= P) break;                              // uniform
    if (vec) {
      if (t + 1 < n_tiles && p0 + 256u < P) issue(p0 + 256u, vn);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t e = threadIdx.x + 256u * i;
        const uint32_t r = e >> 3, q = e & 7u;
        if (!(p0 + r < P && 4u * q < nf)) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        float* d = tile + r * LDT + 4 * q;
        d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[i].x), fabsf(v[i].y)), fmaxf(fabsf(v[i].z), fabsf(v[i].w))));
        bad = bad || !(fabsf(v[i].x) < INFINITY) || !(fabsf(v[i].y) < INFINITY) || !(fabsf(v[i].z) < INFINITY) || !(fabsf(v[i].w) < INFINITY);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = vn[i];
    } else {
      for (uint32_t e = threadIdx.x; e < 256u * 8u; e += 256u) {
        const uint32_t r = e >> 3, q = e & 7u;
        const uint32_t p = p0 + r;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < P && 4 * q < nf) {
          const float* src = d_grid + (size_t)p * ld + 4 * q;
          w.x = src[0];
          if (4 * q + 1 < nf) w.y = src[1];
          if (4 * q + 2 < nf) w.z = src[2];
          if (4 * q + 3 < nf) w.w = src[3];
        }
        float* d = tile + r * LDT + 4 * q;
        d[0] = w.x; d[1] = w.y; d[2] = w.z; d[3] = w.w;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(w.x), fabsf(w.y)), fmaxf(fabsf(w.z), fabsf(w.w))));
        bad = bad || !(fabsf(w.x) < INFINITY) || !(fabsf(w.y) < INFINITY) || !(fabsf(w.z) < INFINITY) || !(fabsf(w.w) < INFINITY);
      }
    }
    __syncthreads();
    const uint32_t p = p0 + threadIdx.x;
    if (p < P) {
      for (uint32_t l = 0; l < n_levels; ++l)
        dg_t[(size_t)l * P + p] = make_float2(tile[threadIdx.x * LDT + 2 * l], tile[threadIdx.x * LDT + 2 * l + 1]);
      if (rows16) {
        const float xc[3] = {xin[(size_t)p * 3], xin[(size_t)p * 3 + 1], xin[(size_t)p * 3 + 2]};
        for (uint32_t l = 0; l < n_levels; ++l) {
          const int slot = rp.slot[l];
          if (slot < 0) continue;                      // uniform
          uint32_t g[3];
          float f[3];                                  // (only the cell is needed)
          grid_cell(xc, lv.scale[l], g, f);
          const uint32_t mask = lv.size[l] - 1u;       // hashed levels are exactly 2^T rows (<= 2^16 here)
          const uint32_t ay0 = g[1] * 2654435761u, ay1 = ay0 + 2654435761u, az0 = g[2] * 805459861u, az1 = az0 + 805459861u;
          uint32_t r[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) r[c] = ((g[0] + (uint32_t)(c & 1)) ^ ((c & 2) ? ay1 : ay0) ^ ((c & 4) ? az1 : az0)) & mask;
          rows16[(size_t)slot * P + p] = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
        }
      }
    }
    __syncthreads();                                   // the tile is overwritten by the next trip
  }
  // max |d_grid|: wave reduce, then ONE conditional atomic per workgroup -- 4096 unconditional same-address atomics
  // serialised into ~40 us of this kernel's 56; a (possibly stale) read of the running max lets all but the first few
  // workgroups skip theirs (staleness only costs a redundant atomic, never a wrong maximum)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wmax[4];
  if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float bm = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (bm > 0.f && bm < INFINITY && bm > __uint_as_float(__atomic_load_n(gmax, __ATOMIC_RELAXED))) atomicMax(gmax, __float_as_uint(bm));
  }
  // The fixed-point bins cannot carry NaN / Inf (fmaxf drops a NaN, the integer conversion of a non-finite product is
  // undefined): a non-finite upstream gradient raises gmax[1] instead and the scatter kernels then write NaN into every
  // row they own, so a diverged step shows up in d_table exactly as it does with per-corner float atomics.
  if (__any(bad) && (threadIdx.x & 63u) == 0 && __atomic_load_n(gmax + 1, __ATOMIC_RELAXED) == 0u) atomicOr(gmax + 1, 1u);
}

// round-to-nearest-even of an fp32 value with |v| < 2^40 to a 64-bit integer: v = hi * 2^16 + lo exactly (hi = trunc(v /
// 2^16), |hi| < 2^24; lo = v - hi * 2^16 is exact in fp32), and rint(v) = hi * 2^16 + rint(lo) because hi * 2^16 is even
__device__ __forceinline__ long long fixed_rn(float v) {
  const float hi_f = truncf(v * (1.0f / 65536.0f));
  const float lo_f = fmaf(-hi_f, 65536.0f, v);
  const int hi = (int)hi_f, lo = (int)rintf(lo_f);
  return ((long long)hi << 16) + (long long)lo;
}

// the same for |v| < 2^51 through the float64 adder: v + 1.5 * 2^52 has v's nearest integer (ties to even) in its low mantissa
// bits; subtracting the constant's bit pattern leaves it as a two's-complement 64-bit integer (4 instructions instead of 11)
__device__ __forceinline__ unsigned long long fixed_rn_f64(float v) {
  const double d = (double)v + 6755399441055744.0;
  return (unsigned long long)__double_as_longlong(d) - 0x4338000000000000ull;
}

__global__ __launch_bounds__(1024) void hashgrid_bwd_binned_kernel(const float* __restrict__ xin, uint32_t P,
                                                                    GridLevels lv, BinPlan plan,
                                                                    const float2* __restrict__ dg_t,
                                                                    const uint32_t* __restrict__ gmax,
                                                                    float* __restrict__ d_table, ReplayPlan rp,
                                                                    const uint4* __restrict__ rows16) {
  // Bins: one float64 per table float, added with ds_add_f64.  Every w*g product is formed in fp32 (as tcnn forms it) and
  // summed in float64, so a cell's sum carries ~1e-16 of relative error whatever the order of the adds -- after the final
  // rounding to fp32 the result is the correctly rounded sum except on near-ties.  Measured LDS atomic rates on MI355X
  // (tools/lds_atomic_rate.hip, cycles per wave-instruction per CU): ds_add_u64 11.9, ds_add_f64 21.6, ds_add_f32 195.
  // Round 1 used 64-bit fixed-point bins (ds_add_u64 of an 11-instruction exact float -> fixed conversion per value): this
  // kernel is VALU-bound, the conversions cost more than the slower atomic (312 -> 276 us per 262 144 points).
  extern __shared__ __attribute__((aligned(16))) unsigned long long bins[];
  double* const dbins = reinterpret_cast<double*>(bins);
  const float mx = __uint_as_float(*gmax);
  const bool poisoned = gmax[1] != 0u;           // NaN / Inf upstream (dgrid_transpose_kernel): NaN into the owned rows
  if (!(mx > 0.f) && !poisoned) return;          // all-zero upstream gradient: nothing to add (uniform exit)
  // job -> (level, chunk, slice).  All chunks of one (level, slice) group sweep the SAME points, so they should share
  // an L2: workgroups are dealt round-robin over the 8 XCDs (xcd = blockIdx % 8), hence group g goes to XCD g % 8 and
  // its chunks sit at consecutive q = blockIdx / 8 -- they start together on that XCD's 32 CUs and 7 of 8 point reads
  // hit L2 instead of each XCD pulling the slice from HBM on its own.
  uint32_t l = 0, chunk, slice;
  if (plan.xcd_major) {
    const uint32_t xcd = blockIdx.x & 7u;
    uint32_t q = blockIdx.x >> 3;
    bool found = false;
    for (l = 0; l < plan.n_levels; ++l) {
      const uint32_t g_lo = plan.group_prefix[l], g_hi = plan.group_prefix[l + 1];
      const uint32_t first = g_lo + ((xcd + 8u - (g_lo & 7u)) & 7u);          // first group of this level on this XCD
      const uint32_t cnt = first < g_hi ? (g_hi - first + 7u) / 8u : 0u;
      const uint32_t nj = cnt * plan.chunks[l];
      if (q < nj) {
        slice = first + 8u * (q / plan.chunks[l]) - g_lo;
        chunk = q % plan.chunks[l];
        found = true;
        break;
      }
      q -= nj;
    }
    if (!found) return;                          // padding workgroup of the XCD-major grid (uniform exit)
  } else {
    while (l + 1 < plan.n_levels && blockIdx.x >= plan.job_prefix[l + 1]) ++l;
    const uint32_t rem = blockIdx.x - plan.job_prefix[l];
    chunk = rem / plan.slices[l];
    slice = rem % plan.slices[l];
  }
  const uint32_t ns = plan.slices[l];
  const uint32_t base = chunk * plan.chunk_rows;
  const uint32_t size = lv.size[l];
  const uint32_t rows = min(plan.chunk_rows, size - base);
  if (poisoned) {                                // uniform
    float* out = d_table + 2 * ((size_t)lv.offset[l] + base);
    for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) out[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) dbins[i] = 0.0;
  __syncthreads();
  const float s = lv.scale[l];
  const uint32_t res = lv.resolution[l], hashed = lv.hashed[l];
  const uint32_t p_lo = (uint32_t)(((uint64_t)P * slice) / ns), p_hi = (uint32_t)(((uint64_t)P * (slice + 1)) / ns);
  const float2* __restrict__ dgl = dg_t + (size_t)l * P;
  // Hashed levels: consecutive lanes = consecutive points (coalesced reads; the hash spreads neighbouring cells).
  // Dense (coarse) levels: neighbouring samples of a ray sit in the same cell, so a coalesced walk puts ~64 lanes on a
  // handful of LDS addresses per atomic; there each thread walks its own contiguous run instead (DNS_SCATTER_WALK=c
  // forces the coalesced walk everywhere, for measurement).
  const uint32_t n_it = (p_hi - p_lo + blockDim.x - 1) / blockDim.x;
  const bool strided = !hashed && plan.strided_dense;
  auto point_of = [&](uint32_t it) -> uint32_t {
    return strided ? p_lo + threadIdx.x * n_it + it : p_lo + it * blockDim.x + threadIdx.x;
  };
  // software pipeline: the next point's 20 bytes are requested before this point's corners are processed, so the
  // two L2 round trips per step hide under the integer / LDS work of the 4 waves per SIMD this kernel can hold
  float2 gg_n = make_float2(0.f, 0.f);
  float xn[3] = {0.f, 0.f, 0.f};
  {
    const uint32_t p = point_of(0);
    if (n_it > 0 && p < p_hi) {
      gg_n = dgl[p];
      xn[0] = xin[(size_t)p * 3];
      xn[1] = xin[(size_t)p * 3 + 1];
      xn[2] = xin[(size_t)p * 3 + 2];
    }
  }
  // The kernel is VALU-bound (SQ counters: 77 % VALU-busy, 288 vector instructions per 64-point visit before this form):
  // the per-axis hash / stride terms are computed once per point (two quarter-rate multiplies instead of two per corner
  // and again per hit), the dense / hashed split is hoisted to a uniform branch, and the bins take the fp32 product as a
  // float64 (one conversion) instead of a 64-bit fixed-point value (11 instructions).
  auto sweep = [&](auto hashed_tag) {
    constexpr bool HASHED = decltype(hashed_tag)::value;
    const uint32_t mask = size - 1u, res2 = res * res;
    for (uint32_t it = 0; it < n_it; ++it) {
      const float2 gg = gg_n;
      const float xc[3] = {xn[0], xn[1], xn[2]};
      const bool live = point_of(it) < p_hi;
      gg_n = make_float2(0.f, 0.f);
      if (it + 1 < n_it) {
        const uint32_t pn = point_of(it + 1);
        if (pn < p_hi) {
          gg_n = dgl[pn];
          xn[0] = xin[(size_t)pn * 3];
          xn[1] = xin[(size_t)pn * 3 + 1];
          xn[2] = xin[(size_t)pn * 3 + 2];
        }
      }
      const bool work = live && !(gg.x == 0.f && gg.y == 0.f);
      float f[3];
      uint32_t g[3];
      grid_cell(xc, s, g, f);
      // per-axis terms of the row index: hashed  x ^ y*P1 ^ z*P2,  dense  x + y*res + z*res^2
      const uint32_t ax0 = g[0], ax1 = g[0] + 1u;
      const uint32_t ay0 = HASHED ? g[1] * 2654435761u : g[1] * res, ay1 = ay0 + (HASHED ? 2654435761u : res);
      const uint32_t az0 = HASHED ? g[2] * 805459861u : g[2] * res2, az1 = az0 + (HASHED ? 805459861u : res2);
      auto row_of = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t {
        if (HASHED) return (x ^ y ^ z) & mask;                            // hashed levels are exactly 2^T rows
        uint32_t idx = x + y + z;
        if (idx >= size) idx %= size;
        return idx;
      };
      const uint32_t rows_eff = work ? rows : 0u;                          // idle lanes never hit
      // Corners are handled as the four x-PAIRS (x, x + 1 at the same y, z): on a hashed level the two rows of a pair differ
      // only in low bits (x ^ (x + 1) is a run of ones, the chunk is the row's high bits), so a pair lands in ONE chunk --
      // about half of the points have a pair here (~4 random chunks of 8 per point) -- and on a dense level the two rows are
      // neighbours.  A branch-free pass builds the lane's 4-bit pair mask, then the wave pops one pair per lane per round: half
      // the rounds of a per-corner loop (SQ counters, round 4: this kernel is VALU-bound, 75 % busy, and the pop loop -- not the
      // hashing, which a stored-rows variant removed without any effect -- is most of its vector instructions).
      uint32_t hit_mask = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t y = (c & 1) ? ay1 : ay0, z = (c & 2) ? az1 : az0;
        const uint32_t l0 = row_of(ax0, y, z) - base, l1 = row_of(ax1, y, z) - base;
        hit_mask |= ((l0 < rows_eff || l1 < rows_eff) ? 1u : 0u) << c;
      }
      while (__any(hit_mask != 0)) {
        if (hit_mask) {
          const uint32_t c = (uint32_t)__ffs((int)hit_mask) - 1u;
          hit_mask &= hit_mask - 1u;
          const uint32_t y = (c & 1u) ? ay1 : ay0, z = (c & 2u) ? az1 : az0;
          const uint32_t l0 = row_of(ax0, y, z) - base, l1 = row_of(ax1, y, z) - base;
          float w0, w1;
          pair_weights(f, c, w0, w1);
          if (l0 < rows_eff) {
            atomicAdd(dbins + 2 * l0, (double)(w0 * gg.x));
            atomicAdd(dbins + 2 * l0 + 1, (double)(w0 * gg.y));
          }
          if (l1 < rows_eff) {
            atomicAdd(dbins + 2 * l1, (double)(w1 * gg.x));
            atomicAdd(dbins + 2 * l1 + 1, (double)(w1 * gg.y));
          }
        }
      }
    }
  };
  // Dense levels, strided walk: a thread's consecutive points are consecutive samples of a ray (or Morton neighbours of the
  // lattice) and stay in one cell for a while on these coarse levels, and near a camera a thousand rays share a handful of
  // cells -- per-point atomics pile many deep on single LDS addresses (measured: the four dense levels of the 16-level grid cost
  // 76 us of the launch).  The thread keeps the 8 corners x 2 features of its CURRENT cell in float64 registers and adds them to
  // the bins when the cell changes: one set of atomics per run instead of per point, with few lanes active at a time.
  auto sweep_dense_runs = [&]() {
    const uint32_t res2 = res * res;
    // row of the current cell's corner (0, 0, 0), as the uint32 sum the forward forms (grid_row) BEFORE its % size: a cell below the
    // box on some axis has coordinate 0xffffffff there and the sum wraps -- every value is a live one, hence the separate flag
    uint32_t cur = 0u;
    bool have = false, in_range = false;
    double acc[8][2];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c][0] = acc[c][1] = 0.0;
    auto flush = [&]() {
#pragma unroll
      for (uint32_t c = 0; c < 8; ++c) {
        uint32_t idx = cur + (c & 1u) + ((c >> 1) & 1u) * res + (c >> 2) * res2;
        if (idx >= size) idx %= size;
        const uint32_t local = idx - base;
        if (local < rows) {
          atomicAdd(dbins + 2 * local, acc[c][0]);
          atomicAdd(dbins + 2 * local + 1, acc[c][1]);
        }
        acc[c][0] = acc[c][1] = 0.0;
      }
    };
    for (uint32_t it = 0; it < n_it; ++it) {
      const float2 gg = gg_n;
      const float xc[3] = {xn[0], xn[1], xn[2]};
      const bool live = point_of(it) < p_hi;
      gg_n = make_float2(0.f, 0.f);
      if (it + 1 < n_it) {
        const uint32_t pn = point_of(it + 1);
        if (pn < p_hi) {
          gg_n = dgl[pn];
          xn[0] = xin[(size_t)pn * 3];
          xn[1] = xin[(size_t)pn * 3 + 1];
          xn[2] = xin[(size_t)pn * 3 + 2];
        }
      }
      if (!(live && !(gg.x == 0.f && gg.y == 0.f))) continue;
      float f[3];
      uint32_t g[3];
      grid_cell(xc, s, g, f);
      const uint32_t r000 = g[0] + g[1] * res + g[2] * res2;
      if (!have || r000 != cur) {
        if (in_range) flush();
        cur = r000;
        have = true;
        // a cell none of whose rows can lie in this chunk is skipped whole -- decidable only where the eight sums r000 .. last
        // neither wrap past 2^32 (last < r000: a cell outside the box) nor reach the level's size (flush takes them % size)
        const uint32_t last = r000 + 1u + res + res2;
        in_range = last < r000 || last >= size || (last >= base && r000 < base + rows);
      }
      if (!in_range) continue;
#pragma unroll
      for (uint32_t c = 0; c < 8; ++c) {
        const float w = corner_weight(f, c);
        acc[c][0] += (double)(w * gg.x);
        acc[c][1] += (double)(w * gg.y);
      }
    }
    if (in_range) flush();
  };
  // Row replay: the level's 8 corner rows of every point were stored by dgrid_transpose_kernel (eight 16-bit values): a visit
  // is a 16-byte load, eight extract-and-compare steps and the three fractions for the weights -- no floor / convert / hash.
  auto sweep_replay = [&](const uint4* __restrict__ rl) {
    uint4 rn = make_uint4(0u, 0u, 0u, 0u);
    {
      const uint32_t p = point_of(0);
      if (n_it > 0 && p < p_hi) rn = rl[p];
    }
    for (uint32_t it = 0; it < n_it; ++it) {
      const float2 gg = gg_n;
      const float xc[3] = {xn[0], xn[1], xn[2]};
      const uint4 rr = rn;
      const bool live = point_of(it) < p_hi;
      gg_n = make_float2(0.f, 0.f);
      if (it + 1 < n_it) {
        const uint32_t pn = point_of(it + 1);
        if (pn < p_hi) {
          gg_n = dgl[pn];
          rn = rl[pn];
          xn[0] = xin[(size_t)pn * 3];
          xn[1] = xin[(size_t)pn * 3 + 1];
          xn[2] = xin[(size_t)pn * 3 + 2];
        }
      }
      const bool work = live && !(gg.x == 0.f && gg.y == 0.f);
      const uint32_t rows_eff = work ? rows : 0u;
      const uint32_t w4[4] = {rr.x, rr.y, rr.z, rr.w};
      uint32_t hit_mask = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t local = ((c & 1) ? (w4[c >> 1] >> 16) : (w4[c >> 1] & 0xffffu)) - base;
        hit_mask |= (local < rows_eff ? 1u : 0u) << c;
      }
      if (!__any(hit_mask != 0)) continue;       // (uniform) most visits of a wave whose points miss this chunk end here
      float f[3];
      uint32_t g[3];                               // (the rows are the stored ones)
      grid_cell(xc, s, g, f);
      while (__any(hit_mask != 0)) {
        if (hit_mask) {
          const uint32_t c = (uint32_t)__ffs((int)hit_mask) - 1u;
          hit_mask &= hit_mask - 1u;
          const uint32_t wsel = (c >> 1) == 0u ? rr.x : ((c >> 1) == 1u ? rr.y : ((c >> 1) == 2u ? rr.z : rr.w));
          const uint32_t local = ((c & 1u) ? (wsel >> 16) : (wsel & 0xffffu)) - base;
          const float w = corner_weight(f, c);
          atomicAdd(dbins + 2 * local, (double)(w * gg.x));
          atomicAdd(dbins + 2 * local + 1, (double)(w * gg.y));
        }
      }
    }
  };
  if (hashed && rows16 && rp.slot[l] >= 0) sweep_replay(rows16 + (size_t)rp.slot[l] * P);
  else if (hashed) sweep(std::true_type{});
  else if (strided && plan.dense_runs) sweep_dense_runs();
  else sweep(std::false_type{});
  __syncthreads();
  float* out = d_table + 2 * ((size_t)lv.offset[l] + base);
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) {
    const double v = dbins[i];
    if (v != 0.0) atomicAdd(out + i, (float)v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Hashed levels of LARGE tables, partition form.  The binned kernel above visits every (point, level) once per 8192-row
// chunk of the level: 8 visits at T = 2^16, 128 at T = 2^20 (11 ms of an 18 ms iteration at 1 M points).  Here every
// (point, level) is hashed ONCE: pass 1 partitions its 8 corner contributions {local row, w*g0, w*g1} by chunk through
// LDS and appends each chunk's run to that chunk's global queue (structure of arrays: coalesced both ways); pass 2
// streams a queue slice into the same 64-bit fixed-point LDS bins with every lane busy.  The queues cost 24 bytes of
// HBM traffic per corner, which at 8 chunks per level is MORE than the redundant hashing it removes (measured at
// T = 2^16, 262 k points: 141 + 122 us against ~190 us for the same levels binned) -- so the host picks this form from
// 16 chunks per level up.  Queues are sized for the uniform-hash expectation plus slack; what does not fit goes straight
// to d_table with float atomics (correct, merely slow: only reachable with adversarially clustered points).

__global__ __launch_bounds__(PART_THREADS) void hashgrid_bwd_partition_kernel(const float* __restrict__ xin, uint32_t P,
                                                                               GridLevels lv, PartPlan pp,
                                                                               const float2* __restrict__ dg_t,
                                                                               uint32_t* __restrict__ qcount,
                                                                               float* __restrict__ queues,
                                                                               float* __restrict__ d_table) {
  __shared__ uint32_t cnt[PART_MAX_CHUNKS], base[PART_MAX_CHUNKS + 1], gofs[PART_MAX_CHUNKS];
  __shared__ uint32_t st_row[PART_ENTRIES];
  __shared__ float st_v0[PART_ENTRIES], st_v1[PART_ENTRIES];
  __shared__ uint8_t st_chunk[PART_ENTRIES];
  const uint32_t p = blockIdx.x * PART_THREADS + threadIdx.x;
  const bool live = p < P;
  float xc[3] = {0.f, 0.f, 0.f};
  if (live) {
    xc[0] = xin[(size_t)p * 3];
    xc[1] = xin[(size_t)p * 3 + 1];
    xc[2] = xin[(size_t)p * 3 + 2];
  }
  const uint32_t row_mask = (1u << pp.chunk_shift) - 1u;
  for (uint32_t li = 0; li < pp.n; ++li) {
    const uint32_t l = pp.level[li], C = pp.chunks[li], cap = pp.cap[li];
    const float2 gg = live ? dg_t[(size_t)l * P + p] : make_float2(0.f, 0.f);
    const bool work = live && !(gg.x == 0.f && gg.y == 0.f);
    const float s = lv.scale[l];
    const uint32_t size = lv.size[l], res = lv.resolution[l];
    const bool hashed = lv.hashed[l] != 0;       // uniform
    float f[3];
    uint32_t g[3];
    grid_cell(xc, s, g, f);
    // per-axis terms of the row index: hashed  x ^ y*P1 ^ z*P2 (size = 2^T),  dense  (x + y*res + z*res^2) mod size
    const uint32_t ax0 = g[0], ax1 = g[0] + 1u;
    const uint32_t ay0 = hashed ? g[1] * 2654435761u : g[1] * res, ay1 = ay0 + (hashed ? 2654435761u : res);
    const uint32_t az0 = hashed ? g[2] * 805459861u : g[2] * res * res, az1 = az0 + (hashed ? 805459861u : res * res);
    for (uint32_t i = threadIdx.x; i < C; i += PART_THREADS) cnt[i] = 0;
    __syncthreads();
    uint32_t rows8[8], slot8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint32_t x = (c & 1) ? ax1 : ax0, y = (c & 2) ? ay1 : ay0, z = (c & 4) ? az1 : az0;
      uint32_t r;
      if (hashed) {
        r = (x ^ y ^ z) & (size - 1u);
      } else {
        r = x + y + z;
        if (r >= size) r %= size;
      }
      rows8[c] = r;
      slot8[c] = work ? atomicAdd(&cnt[r >> pp.chunk_shift], 1u) : 0u;
    }
    __syncthreads();
    // exclusive scan of the <= 128 chunk counts by the first wave, and one global reservation per chunk
    if (threadIdx.x < 64u) {
      uint32_t run = 0;
      for (uint32_t c0 = 0; c0 < C; c0 += 64u) {
        const uint32_t c = c0 + threadIdx.x;
        const uint32_t v = c < C ? cnt[c] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = __shfl_up(incl, o);
          if ((int)threadIdx.x >= o) incl += t;
        }
        if (c < C) {
          base[c] = run + incl - v;
          gofs[c] = v ? atomicAdd(&qcount[pp.qoff[li] + c], v) : 0u;
        }
        run += __shfl(incl, 63);
      }
      if (threadIdx.x == 0) base[C] = run;
    }
    __syncthreads();
    if (work) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float w = corner_weight(f, (uint32_t)c);
        const uint32_t ch = rows8[c] >> pp.chunk_shift;
        const uint32_t at = base[ch] + slot8[c];
        st_row[at] = rows8[c] & row_mask;
        st_v0[at] = w * gg.x;
        st_v1[at] = w * gg.y;
        st_chunk[at] = (uint8_t)ch;
      }
    }
    __syncthreads();
    const uint32_t total = base[C];
    for (uint32_t i = threadIdx.x; i < total; i += PART_THREADS) {
      const uint32_t ch = st_chunk[i];
      const uint32_t at = gofs[ch] + (i - base[ch]);
      if (at < cap) {
        float* q = queues + pp.qbase[li] + (size_t)ch * cap * 3u;
        reinterpret_cast<uint32_t*>(q)[at] = st_row[i];
        q[cap + at] = st_v0[i];
        q[2u * (size_t)cap + at] = st_v1[i];
      } else {                                     // queue full (clustered points on a dense level): straight to the table
        float* t = d_table + 2 * ((size_t)lv.offset[l] + ((size_t)ch << pp.chunk_shift) + st_row[i]);
        atomicAdd(t, st_v0[i]);
        atomicAdd(t + 1, st_v1[i]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void hashgrid_bwd_queue_kernel(GridLevels lv, PartPlan pp, const uint32_t* __restrict__ qcount,
                                                                   const float* __restrict__ queues,
                                                                   const uint32_t* __restrict__ gmax,
                                                                   float* __restrict__ d_table) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long bins[];
  const float mx = __uint_as_float(*gmax);
  const bool poisoned = gmax[1] != 0u;           // NaN / Inf upstream: NaN into the queue's rows (see the binned kernel)
  if (!(mx > 0.f) && !poisoned) return;          // all-zero upstream gradient (uniform exit)
  int ex;
  (void)frexpf(mx, &ex);
  const float scale = ldexpf(1.0f, 40 - ex);     // as in the binned kernel: |w*g| * scale < 2^40
  const double inv_scale = (double)ldexpf(1.0f, ex - 40);
  const uint32_t qi = blockIdx.x / pp.slices, slice = blockIdx.x % pp.slices;   // queue = (level, chunk)
  uint32_t li = 0;
  while (li + 1 < pp.n && qi >= pp.qoff[li + 1]) ++li;
  const uint32_t ch = qi - pp.qoff[li], l = pp.level[li], cap = pp.cap[li];
  const uint32_t row0 = ch << pp.chunk_shift;
  const uint32_t rows = min(1u << pp.chunk_shift, lv.size[l] - row0);
  if (poisoned) {                                // uniform
    float* out = d_table + 2 * ((size_t)lv.offset[l] + row0);
    for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) out[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  const uint32_t n = min(qcount[qi], cap);
  const uint32_t lo = (uint32_t)(((uint64_t)n * slice) / pp.slices), hi = (uint32_t)(((uint64_t)n * (slice + 1)) / pp.slices);
  if (lo >= hi) return;                          // uniform per workgroup
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) bins[i] = 0ull;
  __syncthreads();
  const float* q = queues + pp.qbase[li] + (size_t)ch * cap * 3u;
  const uint32_t* qr = reinterpret_cast<const uint32_t*>(q);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const uint32_t r = qr[i];
    const float v0 = q[cap + i], v1 = q[2u * (size_t)cap + i];
    atomicAdd(bins + 2 * r, (unsigned long long)fixed_rn(v0 * scale));
    atomicAdd(bins + 2 * r + 1, (unsigned long long)fixed_rn(v1 * scale));
  }
  __syncthreads();
  float* out = d_table + 2 * ((size_t)lv.offset[l] + row0);
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) {
    const long long v = (long long)bins[i];
    if (v != 0) atomicAdd(out + i, (float)((double)v * inv_scale));
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Multi-chunk levels, PAIR-LIST form (round 4, DNS_SCATTER_LISTS).  The binned kernel's vector work is its chunk visits (every
// point-level is hashed and tested once per chunk of its level, ~175 vector instructions per 64-point visit of which 32 lanes'
// worth is useful), the queue form's cost is 24 bytes of traffic per corner.  Here pass 1 hashes every point-level once and
// appends, per x-PAIR of corners (x, x + 1 at the same y, z: one chunk on a hashed level), ONE 32-bit word {point, pair} to the
// list of the pair's chunk -- 16 bytes per point-level instead of 192 --, and pass 2 gives every lane one list entry: it fetches
// the entry's point (12 + 8 bytes, consecutive entries are nearly consecutive points), forms the pair's two rows and weights
// and adds into the chunk's float64 LDS bins -- no tests, no idle lanes.  A pair whose two rows straddle a chunk boundary (dense
// levels only) is entered in both chunks; the consumer range-checks each corner.  A full list (clustered points on a dense
// level) sends the pair straight to d_table with float atomics.

// the two rows (level-relative) and weights of x-pair c (bit 0: y + 1, bit 1: z + 1) of a point
struct PairRows {
  uint32_t l0, l1;
  float w0, w1;
};
__device__ __forceinline__ void pair_rows_only(const uint32_t g[3], uint32_t c, bool hashed, uint32_t res, uint32_t size,
                                               uint32_t& l0, uint32_t& l1) {
  const uint32_t gy = g[1] + (c & 1u), gz = g[2] + ((c >> 1) & 1u);
  if (hashed) {                                  // uniform per level
    const uint32_t h = (gy * 2654435761u) ^ (gz * 805459861u);
    l0 = (g[0] ^ h) & (size - 1u);
    l1 = ((g[0] + 1u) ^ h) & (size - 1u);
  } else {
    uint32_t r = g[0] + gy * res + gz * res * res;
    if (r >= size) r %= size;
    l0 = r;
    r = g[0] + 1u + gy * res + gz * res * res;
    if (r >= size) r %= size;
    l1 = r;
  }
}
__device__ __forceinline__ PairRows pair_rows(const float xc[3], float s, uint32_t c, bool hashed, uint32_t res, uint32_t size) {
  uint32_t g[3];
  float f[3];
  grid_cell(xc, s, g, f);
  PairRows r;
  pair_rows_only(g, c, hashed, res, size, r.l0, r.l1);
  pair_weights(f, c, r.w0, r.w1);
  return r;
}

__global__ __launch_bounds__(LIST_THREADS) void hashgrid_bwd_pairlist_kernel(const float* __restrict__ xin, uint32_t P,
                                                                              GridLevels lv, ListPlan lp,
                                                                              const float2* __restrict__ dg_t,
                                                                              const uint32_t* __restrict__ gmax,
                                                                              uint32_t* __restrict__ qcount,
                                                                              uint32_t* __restrict__ lists,
                                                                              float* __restrict__ d_table, uint32_t mode,
                                                                              const uint32_t* __restrict__ lbase) {
  // mode 0: every list level; a hashed level is counted, reserved and written here, a DENSE level is only counted (qcount = the
  // lists' sizes).  mode 1: the dense levels' writing sweep (blockIdx.y indexes lp.dense_idx; qcount = the lists' cursors, lbase =
  // where the scan kernel placed each list inside its level's region).
  // A workgroup takes LIST_TILES x 256 consecutive points of one level.  Sweep A counts its entries per chunk in LDS, the first
  // wave then reserves one run per chunk in the global lists -- ONE atomic per chunk and 2048 points: a reservation per 256 points
  // put 4096 same-address atomics per list behind each other and took longer than everything else --, sweep B forms the chunks
  // again (two multiplies and a few xors per pair) and writes every entry at its run's next free slot.
  __shared__ uint32_t cnt[PART_MAX_CHUNKS], gofs[PART_MAX_CHUNKS];
  if (!(__uint_as_float(*gmax) > 0.f) || gmax[1] != 0u) return;   // all-zero or poisoned upstream gradient: pass 2 handles both
  const uint32_t li = mode ? lp.dense_idx[blockIdx.y] : blockIdx.y;
  const uint32_t l = lp.level[li], C = lp.chunks[li], cap = lp.cap[li];
  const bool exact = lp.dense[li] != 0;          // uniform
  const float s = lv.scale[l];
  const uint32_t size = lv.size[l], res = lv.resolution[l];
  const bool hashed = lv.hashed[l] != 0;         // uniform
  const float2* __restrict__ dgl = dg_t + (size_t)l * P;
  const uint32_t p_base = blockIdx.x * (LIST_THREADS * lp.tiles) + threadIdx.x;
  for (uint32_t i = threadIdx.x; i < C; i += LIST_THREADS) cnt[i] = 0;
  __syncthreads();
  uint32_t work_bits = 0;                        // bit t: the point of tile t carries a gradient
#pragma unroll 2
  for (uint32_t t = 0; t < lp.tiles; ++t) {
    const uint32_t p = p_base + t * LIST_THREADS;
    if (p >= P) break;
    const float2 gg = dgl[p];
    if (gg.x == 0.f && gg.y == 0.f) continue;
    work_bits |= 1u << t;
    const float xc[3] = {xin[(size_t)p * 3], xin[(size_t)p * 3 + 1], xin[(size_t)p * 3 + 2]};
    uint32_t g[3];
    float f[3];
    grid_cell(xc, s, g, f);
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      uint32_t l0, l1;
      pair_rows_only(g, c, hashed, res, size, l0, l1);
      const uint32_t c0 = l0 >> lp.chunk_shift, c1 = l1 >> lp.chunk_shift;
      atomicAdd(&cnt[c0], 1u);
      if (c1 != c0) atomicAdd(&cnt[c1], 1u);
    }
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < C; c += LIST_THREADS) {
    const uint32_t v = cnt[c];
    gofs[c] = v ? atomicAdd(&qcount[lp.qoff[li] + c], v) : 0u;
    if (mode) gofs[c] += lbase[lp.qoff[li] + c];  // exact lists: slot inside the level's region
    cnt[c] = 0;                                  // now the run's next free slot
  }
  if (exact && !mode) return;                    // (uniform) dense level, counting launch: nothing is written yet
  __syncthreads();
  uint32_t* __restrict__ ql = lists + lp.qbase[li];
  float* __restrict__ tl = d_table + 2 * (size_t)lv.offset[l];
#pragma unroll 2
  for (uint32_t t = 0; t < lp.tiles; ++t) {
    if (!((work_bits >> t) & 1u)) continue;
    const uint32_t p = p_base + t * LIST_THREADS;
    const float xc[3] = {xin[(size_t)p * 3], xin[(size_t)p * 3 + 1], xin[(size_t)p * 3 + 2]};
    uint32_t g[3];
    float f[3];
    grid_cell(xc, s, g, f);
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      uint32_t l0, l1;
      pair_rows_only(g, c, hashed, res, size, l0, l1);
      const uint32_t c0 = l0 >> lp.chunk_shift, c1 = l1 >> lp.chunk_shift;
      const uint32_t at0 = gofs[c0] + atomicAdd(&cnt[c0], 1u);
      const uint32_t at1 = c1 != c0 ? gofs[c1] + atomicAdd(&cnt[c1], 1u) : 0u;
      if (exact) {                               // every entry has its place
        ql[at0] = (p << 2) | c;
        if (c1 != c0) ql[at1] = (p << 2) | c;
        continue;
      }
      const bool over0 = at0 >= cap, over1 = c1 != c0 && at1 >= cap;
      if (!over0) ql[(size_t)c0 * cap + at0] = (p << 2) | c;
      if (c1 != c0 && !over1) ql[(size_t)c1 * cap + at1] = (p << 2) | c;
      if (over0 || over1) {                      // list full: the pair's corners in that chunk go straight to the table
        const float2 gg = dgl[p];
        float w0, w1;
        pair_weights(f, c, w0, w1);
        if (over0) {
          atomicAdd(tl + 2 * (size_t)l0, w0 * gg.x);
          atomicAdd(tl + 2 * (size_t)l0 + 1, w0 * gg.y);
        }
        if (c1 == c0 ? over0 : over1) {
          atomicAdd(tl + 2 * (size_t)l1, w1 * gg.x);
          atomicAdd(tl + 2 * (size_t)l1 + 1, w1 * gg.y);
        }
      }
    }
  }
}

// Exclusive prefix sums over the lists (one workgroup, <= 8192 lists): where each dense list starts inside its level's region,
// and how many jobs of `target` entries precede each list (jobstart[n_lists] = all of them).
__global__ __launch_bounds__(1024) void hashgrid_bwd_pairscan_kernel(ListPlan lp, const uint32_t* __restrict__ qcount,
                                                                      uint32_t* __restrict__ lbase, uint32_t* __restrict__ jobstart) {
  __shared__ uint32_t s_n[8192], s_wave[16];
  // the plan's per-level arrays in LDS (a per-thread index into the kernel-argument struct would go through scratch memory), the
  // level of every list in one byte, the counts read once
  __shared__ uint32_t s_qoff[DNS_MAX_LEVELS + 1], s_cap[DNS_MAX_LEVELS], s_dense[DNS_MAX_LEVELS];
  __shared__ uint8_t s_lvl[8192];
  const uint32_t n_lists = lp.qoff[lp.n];
  if (threadIdx.x <= DNS_MAX_LEVELS) s_qoff[threadIdx.x] = lp.qoff[threadIdx.x < DNS_MAX_LEVELS ? threadIdx.x : DNS_MAX_LEVELS];
  if (threadIdx.x < DNS_MAX_LEVELS) {
    s_cap[threadIdx.x] = lp.cap[threadIdx.x];
    s_dense[threadIdx.x] = lp.dense[threadIdx.x];
  }
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < n_lists; q += blockDim.x) {
    uint32_t li = 0;
    while (li + 1 < lp.n && q >= s_qoff[li + 1]) ++li;
    s_lvl[q] = (uint8_t)li;
    s_n[q] = s_dense[li] ? qcount[q] : min(qcount[q], s_cap[li]);
  }
  __syncthreads();
  constexpr uint32_t PER = 8;                    // lists per thread
  const uint32_t t0 = threadIdx.x * PER;
  auto level_of = [&](uint32_t q) { return (uint32_t)s_lvl[q]; };
  uint32_t cnt[PER];
#pragma unroll
  for (uint32_t k = 0; k < PER; ++k) cnt[k] = t0 + k < n_lists ? s_n[t0 + k] : 0u;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {         // pass 0: entries of dense lists (placement), pass 1: jobs of every list
    uint32_t v[PER], run = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      const uint32_t q = t0 + k;
      uint32_t x = 0;
      if (q < n_lists) {
        const uint32_t n = cnt[k];
        x = pass == 0 ? (s_dense[level_of(q)] ? n : 0u) : (n + lp.target - 1u) / lp.target;
      }
      v[k] = run;
      run += x;
    }
    uint32_t incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o);
      if ((int)(threadIdx.x & 63u) >= o) incl += t;
    }
    __syncthreads();
    if ((threadIdx.x & 63u) == 63u) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - run;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) base += s_wave[w];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k)
      if (t0 + k < n_lists) s_n[t0 + k] = base + v[k];
    if (threadIdx.x == 1023u) s_n[8191] = base + run;     // grand total (n_lists < 8192 is checked on the host)
    __syncthreads();
    if (pass == 0) {
#pragma unroll
      for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t q = t0 + k;
        if (q < n_lists) lbase[q] = s_n[q] - s_n[s_qoff[level_of(q)]];   // restart at every level
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k < PER; ++k)
        if (t0 + k < n_lists) jobstart[t0 + k] = s_n[t0 + k];
      if (threadIdx.x == 0) jobstart[n_lists] = s_n[8191];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void hashgrid_bwd_pairbins_kernel(const float* __restrict__ xin, uint32_t P, GridLevels lv,
                                                                      ListPlan lp, const float2* __restrict__ dg_t,
                                                                      const uint32_t* __restrict__ qcount,
                                                                      const uint32_t* __restrict__ lists,
                                                                      const uint32_t* __restrict__ gmax,
                                                                      float* __restrict__ d_table,
                                                                      const uint32_t* __restrict__ lbase,
                                                                      const uint32_t* __restrict__ jobstart) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long bins[];
  const float mx = __uint_as_float(*gmax);
  const bool poisoned = gmax[1] != 0u;           // NaN / Inf upstream: NaN into the list's rows (see the binned kernel)
  if (!(mx > 0.f) && !poisoned) return;          // all-zero upstream gradient (uniform exit)
  // 64-bit FIXED-POINT bins (|w g| * 2^(40 - ex) < 2^40, rounded to nearest: exact, order-independent sums with 2^24 entries of
  // headroom): this kernel is bound by the LDS atomic unit, not by its vector instructions, and ds_add_u64 issues at 11.9 cycles
  // per wave instruction against 21.6 for ds_add_f64 -- the conversion that lost in the (vector-bound) sweep form pays here
  int ex;
  (void)frexpf(mx, &ex);
  //  gradients below 2^-87 would push the scale 2^(40 - ex) past fp32's range (inf, then NaN into the bins): the
  // exponent is held at -80 -- such values then lose low bits below 2^-120 of themselves, i.e. nothing fp32 could represent
  // in the sum anyway
  ex = max(ex, -80);
  const float scale = ldexpf(1.0f, 40 - ex);
  const double inv_scale = (double)ldexpf(1.0f, ex - 40);
  uint32_t qi, slice;                            // list = (level, chunk), and which part of it
  if (lp.balanced && !poisoned) {
    // job -> list: the job prefix (n_lists + 1 words, behind the bins in LDS) is searched for the last list that starts at or
    // before this job
    uint32_t* js = reinterpret_cast<uint32_t*>(bins + ((size_t)2 << lp.chunk_shift));
    const uint32_t n_lists = lp.qoff[lp.n];
    for (uint32_t i = threadIdx.x; i <= n_lists; i += blockDim.x) js[i] = jobstart[i];
    __syncthreads();
    if (blockIdx.x >= js[n_lists]) return;       // (uniform) past the last job of this launch
    uint32_t lo_q = 0, hi_q = n_lists;           // invariant: js[lo_q] <= job < js[hi_q]
    while (hi_q - lo_q > 1u) {
      const uint32_t mid = (lo_q + hi_q) >> 1;
      if (js[mid] <= blockIdx.x) lo_q = mid; else hi_q = mid;
    }
    qi = lo_q;
    slice = blockIdx.x - js[qi];
    __syncthreads();                             // js lives in LDS the bins do not use; nothing else to order
  } else if (lp.balanced) {                      // poisoned: one job per list writes the NaNs
    qi = blockIdx.x;
    slice = 0;
    if (qi >= lp.qoff[lp.n]) return;
  } else {
    qi = blockIdx.x / lp.slices;
    slice = blockIdx.x % lp.slices;
  }
  uint32_t li = 0;
  while (li + 1 < lp.n && qi >= lp.qoff[li + 1]) ++li;
  const uint32_t ch = qi - lp.qoff[li], l = lp.level[li], cap = lp.cap[li];
  const uint32_t row0 = ch << lp.chunk_shift;
  const uint32_t size = lv.size[l], res = lv.resolution[l];
  const uint32_t rows = min(1u << lp.chunk_shift, size - row0);
  if (poisoned) {                                // uniform
    float* out = d_table + 2 * ((size_t)lv.offset[l] + row0);
    if (slice == 0)
      for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) out[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  const uint32_t n = lp.dense[li] ? qcount[qi] : min(qcount[qi], cap);
  uint32_t lo, hi;
  if (lp.balanced) {
    lo = slice * lp.target;
    hi = min(n, lo + lp.target);
  } else {
    lo = (uint32_t)(((uint64_t)n * slice) / lp.slices);
    hi = (uint32_t)(((uint64_t)n * (slice + 1)) / lp.slices);
  }
  if (lo >= hi) return;                          // uniform per workgroup
  const uint32_t* __restrict__ q = lists + lp.qbase[li] + (lp.dense[li] ? (size_t)lbase[qi] : (size_t)ch * cap);
  const float2* __restrict__ dgl = dg_t + (size_t)l * P;
  const float s = lv.scale[l];
  const bool hashed = lv.hashed[l] != 0;         // uniform
  // The loop is a chain of dependent memory round trips (entry -> point -> bins) on few waves per SIMD (one 128-KB workgroup per
  // CU): every thread keeps U entries of a trip in flight together, two stages deep -- the entries of trip t + 2 and the points of
  // trip t + 1 are requested while trip t computes.
  constexpr uint32_t U = 4;
  // Lane <-> entry.  A list is in point order; on a DENSE level consecutive samples of a ray share a cell, hence a pair's two rows,
  // and with consecutive entries on consecutive lanes a wave's atomics pile several deep on one address: there lane j of wave w
  // takes entry j * n_waves + w of every round of blockDim.x entries (neighbouring lanes n_waves entries apart; the workgroup's
  // waves share the lines they read).  Hashed levels keep the coalesced order (measured 20 % faster there).
  const uint32_t nt = blockDim.x;
  const uint32_t i0 = lo + (hashed ? threadIdx.x : (threadIdx.x & 63u) * (nt >> 6) + (threadIdx.x >> 6));
  uint32_t e_n[U], e_nn[U];
  float xn[U][3];
  float2 gn[U];
#pragma unroll
  for (uint32_t u = 0; u < U; ++u) e_n[u] = (i0 + u * nt < hi) ? q[i0 + u * nt] : 0u;
#pragma unroll
  for (uint32_t u = 0; u < U; ++u) e_nn[u] = (i0 + (U + u) * nt < hi) ? q[i0 + (U + u) * nt] : 0u;
#pragma unroll
  for (uint32_t u = 0; u < U; ++u) {
    const uint32_t pn = e_n[u] >> 2;             // 0 past the end: a valid point, never used
    xn[u][0] = xin[(size_t)pn * 3];
    xn[u][1] = xin[(size_t)pn * 3 + 1];
    xn[u][2] = xin[(size_t)pn * 3 + 2];
    gn[u] = dgl[pn];
  }
  // the bins are cleared while the first entries and points are on their way
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) bins[i] = 0ull;
  __syncthreads();
  for (uint32_t i = i0; i < hi; i += U * nt) {
    uint32_t e[U];
    float xc[U][3];
    float2 gg[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      e[u] = e_n[u];
      xc[u][0] = xn[u][0];
      xc[u][1] = xn[u][1];
      xc[u][2] = xn[u][2];
      gg[u] = gn[u];
      e_n[u] = e_nn[u];
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      const uint32_t pn = e_n[u] >> 2;
      xn[u][0] = xin[(size_t)pn * 3];
      xn[u][1] = xin[(size_t)pn * 3 + 1];
      xn[u][2] = xin[(size_t)pn * 3 + 2];
      gn[u] = dgl[pn];
    }
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) e_nn[u] = (i + (2u * U + u) * nt < hi) ? q[i + (2u * U + u) * nt] : 0u;
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      if (i + u * nt >= hi) break;
      const PairRows r = hashed ? pair_rows(xc[u], s, e[u] & 3u, true, res, size) : pair_rows(xc[u], s, e[u] & 3u, false, res, size);
      const uint32_t a0 = r.l0 - row0, a1 = r.l1 - row0;
      if (a0 < rows) {
        atomicAdd(bins + 2 * a0, fixed_rn_f64(r.w0 * gg[u].x * scale));
        atomicAdd(bins + 2 * a0 + 1, fixed_rn_f64(r.w0 * gg[u].y * scale));
      }
      if (a1 < rows) {
        atomicAdd(bins + 2 * a1, fixed_rn_f64(r.w1 * gg[u].x * scale));
        atomicAdd(bins + 2 * a1 + 1, fixed_rn_f64(r.w1 * gg[u].y * scale));
      }
    }
  }
  __syncthreads();
  float* out = d_table + 2 * ((size_t)lv.offset[l] + row0);
  for (uint32_t i = threadIdx.x; i < rows * 2; i += blockDim.x) {
    const long long v = (long long)bins[i];
    if (v != 0) atomicAdd(out + i, (float)((double)v * inv_scale));
  }
}

static int scatter_init_attrs() {
  const int bytes = 8192 * 2 * (int)sizeof(unsigned long long);   // one 8192-row chunk of 64-bit bins: 128 KB
  if (hipFuncSetAttribute((const void*)hashgrid_bwd_binned_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess ||
      hipFuncSetAttribute((const void*)hashgrid_bwd_queue_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess ||
      // (+ the job prefix of balanced dense lists: 4 (n_lists + 1) bytes behind the bins; with DNS_LIST_SHIFT=13 the bins alone
      //  are the whole 128 KB -- ADVICE r4)
      hipFuncSetAttribute((const void*)hashgrid_bwd_pairbins_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) != hipSuccess) {
    set_error("dns_init: hipFuncSetAttribute failed for the hash-grid scatter kernels");
    return DNS_E_LAUNCH;
  }
  return DNS_OK;
}
static AttrRegistrar scatter_attr_registrar(scatter_init_attrs);

int launch_table_scatter(const float* x, uint32_t P, const GridLevels& lv, const float* d_grid, uint32_t ld_dgrid, float* d_table,
                         float* ws, const ScatterPlan& W, hipStream_t st) {
  const ReplayPlan& rp = W.rp;
  uint4* rows16 = W.n_replay ? reinterpret_cast<uint4*>(ws + W.replay) : nullptr;
  uint32_t* gmax = (uint32_t*)(ws + W.gmax);
  {                                                                          // max word, non-finite flag, pad
    const int rc = fill_words(gmax, 0u, W.clear_words, st, "dns_encode_bwd");
    if (rc != DNS_OK) return rc;
  }
  DNS_LAUNCH(dgrid_transpose_kernel, dim3(W.transpose.grid), dim3(W.transpose.block), 0, st, d_grid, ld_dgrid, P, lv.n_levels, (float2*)ws, gmax, x, lv, rp,
             rows16, W.dg_tiles);
  if (W.sweep.grid)
    DNS_LAUNCH(hashgrid_bwd_binned_kernel, dim3(W.sweep.grid), dim3(W.sweep.block), W.sweep.lds, st, x, P, lv, W.bins, (const float2*)ws, gmax, d_table,
               rp, (const uint4*)rows16);
  if (W.lists) {
    const ListPlan& lp = W.lp;
    uint32_t* lcount = reinterpret_cast<uint32_t*>(ws + W.lcount);
    uint32_t* lists = reinterpret_cast<uint32_t*>(ws + W.lwords);
    const uint32_t n_lists = lp.qoff[lp.n];
    uint32_t* lcursor = lcount + n_lists;
    uint32_t* lbase = lcursor + n_lists;
    uint32_t* jobstart = lbase + n_lists;
    DNS_LAUNCH(hashgrid_bwd_pairlist_kernel, dim3(W.list_count.grid, W.list_count.grid_y), dim3(W.list_count.block), 0, st, x, P, lv, lp, (const float2*)ws, gmax, lcount,
               lists, d_table, 0u, (const uint32_t*)nullptr);
    if (lp.balanced) {
      DNS_LAUNCH(hashgrid_bwd_pairscan_kernel, dim3(W.list_scan.grid), dim3(W.list_scan.block), 0, st, lp, (const uint32_t*)lcount, lbase, jobstart);
      DNS_LAUNCH(hashgrid_bwd_pairlist_kernel, dim3(W.list_write.grid, W.list_write.grid_y), dim3(W.list_write.block), 0, st, x, P, lv, lp, (const float2*)ws, gmax,
                 lcursor, lists, d_table, 1u, (const uint32_t*)lbase);
    }
    DNS_LAUNCH(hashgrid_bwd_pairbins_kernel, dim3(W.list_bins.grid), dim3(W.list_bins.block), W.list_bins.lds, st, x, P, lv, lp,
               (const float2*)ws, lcount, lists, gmax, d_table, (const uint32_t*)lbase, (const uint32_t*)jobstart);
  }
  if (W.part) {
    const PartPlan& pp = W.pp;
    uint32_t* qcount = reinterpret_cast<uint32_t*>(ws + W.qcount);
    float* queues = ws + W.queues;
    {
      const int rc = fill_words(qcount, 0u, pp.qoff[pp.n], st, "dns_encode_bwd");
      if (rc != DNS_OK) return rc;
    }
    DNS_LAUNCH(hashgrid_bwd_partition_kernel, dim3(W.partition.grid), dim3(W.partition.block), 0, st, x, P, lv,
                       pp, (const float2*)ws, qcount, queues, d_table);
    DNS_LAUNCH(hashgrid_bwd_queue_kernel, dim3(W.queue.grid), dim3(W.queue.block), W.queue.lds, st, lv, pp,
                       qcount, queues, gmax, d_table);
  }
  return DNS_OK;
}

}  // namespace dns
