// Point encoding kernels: fp64 normalisation + OneBlob + multi-resolution hash grid.
//
// Replaces tcnn OneBlob / HashGrid behind Pos_Encoding.forward (reference models/decoder.py:45-48,
// models/pos_encoding.py:31-46,61-71) and the normalisation of slams/mapping.py:608.
//
// Layout: one lane = one point; all 16 levels x 8 corners of a point are issued by the same lane, so
// 128 independent 8-byte gathers are in flight per lane (the table is L2 / Infinity-Cache resident:
// 6.8 MB at T=2^16, 58 MB at T=2^20) and the lane's 32 grid features leave as 16-byte stores.
// Bound: memory system (random 8-B gathers, 1024 B per point), not MFMA.
//
// Arithmetic contract shared with oracle/tcnn_ref.py: pos = x*scale + 0.5 is two IEEE roundings
// (never contracted), the cell is (uint32)(int)floorf(pos); hash primes
// {1, 2654435761, 805459861}; index % level size.  Those make the table rows bit-exact.  The arithmetic
// itself -- cell, weights, level gather, OneBlob -- lives in dev_encode.hpp, one spelling for these kernels,
// the table scatter and the fused tracker; this file owns the tiles, the phases and the launches.
#include <type_traits>
#include "common.hpp"
#include "split_rows.hpp"
#include "dev_encode.hpp"
#include "scatter_plan.hpp"

namespace dns {

// The (row, column group) pairs of a rows x nq tile, dealt to the workgroup's threads in row-major order: fn(r, c).  (row, column)
// advance incrementally: an integer division per element was a visible cost.
template <typename F>
__device__ __forceinline__ void tile_walk(uint32_t rows, uint32_t nq, F fn) {
  const uint32_t dr = blockDim.x / nq, dc = blockDim.x - dr * nq;
  uint32_t r = threadIdx.x / nq, c = threadIdx.x - r * nq;
  for (uint32_t i = threadIdx.x; i < rows * nq; i += blockDim.x) {
    fn(r, c);
    r += dr;
    c += dc;
    if (c >= nq) { c -= nq; ++r; }
  }
}

// One lane = one point.  TILED = the [P, 3*n_bins + 2*L] output rows are contiguous (OneBlob | grid in one buffer):
// the lane's channels go to an LDS tile (row stride +1 float: conflict-free) and the workgroup's tile leaves as one
// contiguous, fully coalesced run.  Direct 16-byte row stores at a 320-byte lane stride were measured to cost 3.4x
// the bytes in HBM writes (rocprofv3 WRITE_SIZE 286 MB for an 84 MB output): every store instruction touches 64 lines.
// TILED: the workgroup's output rows leave as contiguous runs through an LDS tile (direct 16-byte row stores at a 320-byte
// lane stride cost 3.4x the bytes in HBM writes).  The tile is used TWICE -- OneBlob columns, flush, then grid columns,
// flush -- so it holds max(pe_dim, g_dim) + 1 floats per point (25 KB instead of 41 KB): LDS, not registers (68 VGPRs),
// is what limits this gather kernel's occupancy, and 12 waves per CU hide the table-gather latency better than 6.
// HALF (with TILED; ABI v12, DNS_SPLIT_PLAIN): the row leaves as plain f16 -- the flush converts eight tile values to one
// 16-byte store; pe_out / grid_out then point at halfs and ld_pe / ld_grid count halfs.  (The scaled split-row writer below
// evaluates OneBlob twice and flushes in four steps: 98.6 us against this kernel's 84 at 262 144 points.)
template <bool TILED, bool HALF = false>
__global__ __launch_bounds__(128) void encode_fwd_kernel(const float* __restrict__ in, Bound6 bd, int normalise,
                                                         uint32_t P, uint32_t n_bins,
                                                         const float2* __restrict__ table, GridLevels lv,
                                                         float* __restrict__ x_out, float* __restrict__ pe_out,
                                                         uint32_t ld_pe, float* __restrict__ grid_out,
                                                         uint32_t ld_grid, float2* __restrict__ dydx, uint32_t pe_ph,
                                                         uint32_t g_ph) {
  extern __shared__ float tile[];
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t pe_dim = 3 * n_bins;
  // (TILED) the tile is used pe_ph + g_ph times: OneBlob in 1 or 3 phases (all axes / one axis each), the grid in g_ph groups of
  // levels -- every phase ends in a flush, so the tile holds the widest PHASE + 1 floats per point
  const uint32_t lpp = lv.n_levels / g_ph;                // levels per grid phase (host: g_ph divides n_levels)
  const uint32_t ldt = max(pe_dim / pe_ph, 2u * lpp) + 1;
  const bool live = p < P;
  float x[3] = {0.f, 0.f, 0.f};
  if (live) load_point(in, bd, normalise != 0, p, x);
  if (live && x_out) {
    x_out[(size_t)p * 3 + 0] = x[0];
    x_out[(size_t)p * 3 + 1] = x[1];
    x_out[(size_t)p * 3 + 2] = x[2];
  }
  float* trow = tile + threadIdx.x * ldt;
  auto col_ptr = [](float* base, uint32_t col) -> float* {           // column `col` of an output row (HALF: the row holds halfs)
    return HALF ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(base) + col) : base + col;
  };
  // rows [p0, p0 + rows) x columns [c0, c0 + nc) of the row-major output with leading dimension ld, from the tile
  auto flush = [&](float* out_base, uint32_t ld, uint32_t nc) {
    __syncthreads();
    const uint32_t p0 = blockIdx.x * blockDim.x;
    const uint32_t rows = min(blockDim.x, P - p0);
    float* out = out_base + (size_t)p0 * ld;
    // 16-byte global accesses where the rows allow it (the LDS tile's odd row stride keeps its side at dwords)
    if constexpr (HALF) {                              // nc, ld multiples of 8, out_base 16-byte aligned (host-checked)
      _Float16* outh = reinterpret_cast<_Float16*>(out_base) + (size_t)p0 * ld;
      tile_walk(rows, nc >> 3, [&](uint32_t r, uint32_t c) {
        const float* t = tile + r * ldt + 8 * c;
        typedef _Float16 half8v __attribute__((ext_vector_type(8)));
        half8v h;
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = (_Float16)t[k];
        *reinterpret_cast<half8v*>(outh + (size_t)r * ld + 8 * c) = h;
      });
    } else if (((nc | ld) & 3u) == 0 && ((((uintptr_t)out_base) & 15u) == 0)) {
      tile_walk(rows, nc >> 2, [&](uint32_t r, uint32_t c) {
        const float* t = tile + r * ldt + 4 * c;
        *reinterpret_cast<float4*>(out + (size_t)r * ld + 4 * c) = make_float4(t[0], t[1], t[2], t[3]);
      });
    } else {
      tile_walk(rows, nc, [&](uint32_t r, uint32_t c) { out[(size_t)r * ld + c] = tile[r * ldt + c]; });
    }
    __syncthreads();
  };
  if (pe_out) {
    float* row = TILED ? trow : pe_out + (size_t)p * ld_pe;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t c0 = (TILED && pe_ph == 3u) ? 0u : a * n_bins;      // the axis' first tile / row column
      if (live) oneblob_axis_fwd(x[a], n_bins, row + c0);
      if (TILED && pe_ph == 3u) flush(col_ptr(pe_out, a * n_bins), ld_pe, n_bins);
    }
    if (TILED && pe_ph != 3u) flush(pe_out, ld_pe, pe_dim);
  }
  if (grid_out) {
    for (uint32_t ph = 0; ph < g_ph; ++ph) {
    if (live) {
      float* row = TILED ? trow - 2u * lpp * ph : grid_out + (size_t)p * ld_grid;     // (TILED: level l's pair at tile column 2 (l - lpp ph))
#pragma unroll 4
      for (uint32_t l = lpp * ph; l < lpp * (ph + 1u); ++l) grid_level(table, lv, l, x, row, dydx, P, p);
    }
    if (TILED) flush(col_ptr(grid_out, 2u * lpp * ph), ld_grid, 2u * lpp);
    }
  }
}
// The same encoding written in the SPLIT-ROW format of split_rows.hpp (and, optionally, as fp32 rows as well): what the MLP
// kernels of fused_step.MapStep / TrackStep read.  One lane = one point, outputs through the same two-phase LDS tile as
// encode_fwd_kernel<true> (max(pe_dim, g_dim) + 1 floats per point: LDS, not registers, limits the occupancy of this gather
// kernel).  The row's exponent needs max |row| over BOTH halves before the first value is converted:
//   A  OneBlob -> tile (fp32), its maximum; flushed as fp32 columns [0, pe_dim) when f32_out is wanted
//   B  grid gather -> tile (fp32), its maximum -> e = scale_exp(max) (bit for bit what mlp_split.hpp's x_row_max / scale_exp
//      derived from the fp32 row); fp32 flush; then the 2 L values as hi | lo pairs, flushed into the row's two planes
//   C  OneBlob evaluated a second time (the OneBlob half of this kernel is free: measured 99.7 vs 96.0 us with / without it),
//      converted with e and flushed.
// xs_out [P][ldxs] halfs: columns [0, K) hi, [K, 2K) lo (K = pe_dim + g_dim); hi_only: the lo plane is not written.
__global__ __launch_bounds__(128) void encode_fwd_split_kernel(const float* __restrict__ in, Bound6 bd, int normalise, uint32_t P,
                                                               uint32_t n_bins, const float2* __restrict__ table, GridLevels lv,
                                                               float* __restrict__ x_out, float* __restrict__ f32_out, uint32_t ld32,
                                                               uint32_t* __restrict__ xs_out, uint32_t ldxs_w, int32_t* __restrict__ xexp,
                                                               int hi_only, float2* __restrict__ dydx) {
  extern __shared__ float tile[];
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t pe_dim = 3 * n_bins, g_dim = 2 * lv.n_levels, K = pe_dim + g_dim;
  const uint32_t ldt = max(pe_dim, g_dim) + 1;
  const bool live = p < P;
  float x[3] = {0.f, 0.f, 0.f};
  if (live) load_point(in, bd, normalise != 0, p, x);
  if (live && x_out) {
    x_out[(size_t)p * 3 + 0] = x[0];
    x_out[(size_t)p * 3 + 1] = x[1];
    x_out[(size_t)p * 3 + 2] = x[2];
  }
  float* trow = tile + threadIdx.x * ldt;
  // tile columns [tc0, tc0 + nc) of the workgroup's rows -> columns [c0, c0 + nc) of the row-major `out` (32-bit words, leading
  // dimension ld); nc, c0, ld multiples of 4 and out 16-byte aligned (checked on the host): 16-byte global stores
  auto flush = [&](uint32_t* out_base, uint32_t ld, uint32_t c0, uint32_t nc, uint32_t tc0) {
    __syncthreads();
    const uint32_t p0 = blockIdx.x * blockDim.x;
    const uint32_t rows = min(blockDim.x, P - p0);
    uint32_t* out = out_base + (size_t)p0 * ld + c0;
    tile_walk(rows, nc >> 2, [&](uint32_t r, uint32_t c) {
      const uint32_t* t = reinterpret_cast<const uint32_t*>(tile) + r * ldt + tc0 + 4 * c;
      *reinterpret_cast<uint4*>(out + (size_t)r * ld + 4 * c) = make_uint4(t[0], t[1], t[2], t[3]);
    });
    __syncthreads();
  };
  // ---- A
  float rmax = 0.f;
  bool bad = false;                                       // fmaxf drops a NaN: a non-finite value must reach the exponent rule
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) oneblob_axis_fwd(x[a], n_bins, trow + a * n_bins);
    for (uint32_t c = 0; c < pe_dim; ++c) {
      rmax = fmaxf(rmax, fabsf(trow[c]));
      bad = bad || !(fabsf(trow[c]) < INFINITY);
    }
  }
  if (f32_out) flush(reinterpret_cast<uint32_t*>(f32_out), ld32, 0, pe_dim, 0);
  else __syncthreads();
  const bool plain = (hi_only & 2) != 0;                  // DNS_SPLIT_PLAIN: unscaled f16 values, no exponent
  // ---- B
  if (live) {
#pragma unroll 4
    for (uint32_t l = 0; l < lv.n_levels; ++l) {
      const float2 v = grid_level(table, lv, l, x, trow, dydx, P, p);
      rmax = fmaxf(rmax, fmaxf(fabsf(v.x), fabsf(v.y)));
      bad = bad || !(fabsf(v.x) < INFINITY) || !(fabsf(v.y) < INFINITY);
    }
  }
  const int e = plain ? 0 : sr::scale_exp(bad ? INFINITY : rmax);
  const float sc = ldexpf(1.0f, e);
  if (live && !plain) xexp[p] = e;
  if (f32_out) flush(reinterpret_cast<uint32_t*>(f32_out), ld32, pe_dim, g_dim, 0);
  // the lane's own row back out of the tile, as packed pairs: hi pairs at tile columns [0, n/2), lo pairs at [n/2, n)
  auto repack = [&](uint32_t n) {
    uint32_t* urow = reinterpret_cast<uint32_t*>(trow);
    uint32_t hi[32], lo[32];                               // n <= 64 values (host-checked)
#pragma unroll
    for (uint32_t i = 0; i < 32; ++i) {
      if (2 * i < n) sr::split_pair(trow[2 * i], trow[2 * i + 1], sc, hi[i], lo[i]);
    }
#pragma unroll
    for (uint32_t i = 0; i < 32; ++i) {
      if (2 * i < n) {
        urow[i] = hi[i];
        urow[n / 2 + i] = lo[i];
      }
    }
  };
  if (live) repack(g_dim);
  flush(xs_out, ldxs_w, pe_dim / 2, g_dim / 2, 0);
  if (!hi_only) flush(xs_out, ldxs_w, K / 2 + pe_dim / 2, g_dim / 2, g_dim / 2);
  // (plain rows: the OneBlob values need no row maximum, but the tile holds one half of the row at a time: evaluated again like
  //  the scaled form -- measured free beside the gather, 99.7 vs 96.0 us)
  // ---- C
  if (live) {
#pragma unroll
    for (int a = 0; a < 3; ++a) oneblob_axis_fwd(x[a], n_bins, trow + a * n_bins);
    repack(pe_dim);
  }
  flush(xs_out, ldxs_w, 0, pe_dim / 2, 0);
  if (!hi_only) flush(xs_out, ldxs_w, K / 2, pe_dim / 2, pe_dim / 2);
}

template <bool TILED>
__global__ __launch_bounds__(128) void encode_bwd_kernel(const float* __restrict__ xin, Bound6 bd, int scale_by_bound,
                                                         uint32_t P, uint32_t n_bins,
                                                         const float2* __restrict__ table, GridLevels lv,
                                                         const float* __restrict__ d_pe, uint32_t ld_dpe,
                                                         const float* __restrict__ d_grid, uint32_t ld_dgrid,
                                                         float* __restrict__ d_table, float* __restrict__ d_x,
                                                         const float2* __restrict__ dydx, uint32_t pe_ph, uint32_t g_ph) {
  extern __shared__ float tile[];
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t pe_dim = 3 * n_bins;
  const uint32_t lpp = g_ph ? lv.n_levels / g_ph : 0u;    // levels per grid phase (TILED; host: g_ph divides n_levels; 0: OneBlob columns only)
  // TILED: the workgroup's gradient rows come in through an LDS tile (coalesced row reads instead of one 320-byte-strided
  // row per lane), in TWO phases like the forward -- OneBlob columns, then grid columns -- so that the tile holds
  // max(pe_dim, g_dim) + 1 floats per point (25 KB, 12 waves per CU) instead of the whole row (41 KB, 6 waves): this
  // kernel is latency-bound (dependent LDS reads, 8-byte gathers), occupancy is what it lacked.
  // (round 5: pe_ph = 3 / g_ph = 2 phases -- one OneBlob axis / half the levels at a time, 17 floats per point: see encode_fwd_kernel)
  const uint32_t ldt = max(pe_dim / pe_ph, 2u * lpp) + 1;
  const bool live = p < P;
  auto stage = [&](uint32_t col0, uint32_t nc) {         // columns [col0, col0 + nc) of the workgroup's rows -> tile
    __syncthreads();
    const uint32_t p0 = blockIdx.x * blockDim.x;
    const uint32_t rows = min(blockDim.x, P - p0);
    const float* src = d_pe + (size_t)p0 * ld_dpe + col0;
    if (((nc | ld_dpe | col0) & 3u) == 0 && ((((uintptr_t)d_pe) & 15u) == 0)) {
      tile_walk(rows, nc >> 2, [&](uint32_t r, uint32_t c) {
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * ld_dpe + 4 * c);
        float* t = tile + r * ldt + 4 * c;
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
      });
    } else {
      tile_walk(rows, nc, [&](uint32_t r, uint32_t c) { tile[r * ldt + c] = src[(size_t)r * ld_dpe + c]; });
    }
    __syncthreads();
  };
  float x[3] = {0.f, 0.f, 0.f};
  if (live) {
    x[0] = xin[(size_t)p * 3 + 0];
    x[1] = xin[(size_t)p * 3 + 1];
    x[2] = xin[(size_t)p * 3 + 2];
  }
  const bool pe_split = TILED && pe_ph == 3u;
  if (TILED && !pe_split) stage(0, pe_dim);
  float dx[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (pe_split) stage(a * n_bins, n_bins);               // (uniform: every thread of the workgroup)
    if (live && d_pe && d_x) {
      // the axis' gradient columns: a whole row (tile or global), or the axis' own tile phase
      const float* grad = TILED ? tile + threadIdx.x * ldt + (pe_split ? 0u : a * n_bins) : d_pe + (size_t)p * ld_dpe + a * n_bins;
      oneblob_axis_bwd(x[a], n_bins, grad, dx[a]);
    }
  }
  for (uint32_t ph = 0; ph < (TILED ? g_ph : 1u); ++ph) {
  const uint32_t l_lo = TILED ? lpp * ph : 0u, l_hi = TILED ? lpp * (ph + 1u) : lv.n_levels;
  if (TILED) stage(pe_dim + 2u * l_lo, 2u * (l_hi - l_lo));
  if (live && d_grid && dydx && d_x && !d_table) {
    // the forward kept d(features)/dx: a streaming dot product, no gather (coalesced 8-byte reads, lane = point).
    // (Requesting all 48 values before the first staging barrier was measured: 96 more registers, 0.102 -> 0.113 ms.)
    const float* row = TILED ? tile + threadIdx.x * ldt - 2u * l_lo : d_grid + (size_t)p * ld_dgrid;
#pragma unroll 4
    for (uint32_t l = l_lo; l < l_hi; ++l) {
      const float g0 = row[2 * l], g1 = row[2 * l + 1];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float2 j = dydx[((size_t)l * 3 + a) * P + p];
        dx[a] += j.x * g0 + j.y * g1;
      }
    }
  } else if (live && d_grid) {
    const float* row = TILED ? tile + threadIdx.x * ldt - 2u * l_lo : d_grid + (size_t)p * ld_dgrid;
#pragma unroll 2
    for (uint32_t l = l_lo; l < l_hi; ++l) {
      const float g0 = row[2 * l], g1 = row[2 * l + 1];
      const float s = lv.scale[l];
      const uint32_t res = lv.resolution[l], size = lv.size[l], hashed = lv.hashed[l];
      const uint32_t off = lv.offset[l];
      float f[3];
      uint32_t g[3];
      grid_cell(x, s, g, f);
      uint32_t r[8];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        r[c] = off + grid_row(g[0] + (c & 1), g[1] + ((c >> 1) & 1), g[2] + ((c >> 2) & 1), res, size, hashed);
      if (d_table && (g0 != 0.f || g1 != 0.f)) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float w = corner_weight(f, (uint32_t)c);
          atomicAdd(d_table + 2 * (size_t)r[c], w * g0);
          atomicAdd(d_table + 2 * (size_t)r[c] + 1, w * g1);
        }
      }
      if (d_x) {
        float dot[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float2 v = table[r[c]];
          dot[c] = v.x * g0 + v.y * g1;
        }
        const float wx0 = 1.0f - f[0], wx1 = f[0], wy0 = 1.0f - f[1], wy1 = f[1], wz0 = 1.0f - f[2], wz1 = f[2];
        // d/dx: pairs (c, c|1);  d/dy: (c, c|2);  d/dz: (c, c|4)
        const float ddx = wy0 * wz0 * (dot[1] - dot[0]) + wy1 * wz0 * (dot[3] - dot[2]) +
                          wy0 * wz1 * (dot[5] - dot[4]) + wy1 * wz1 * (dot[7] - dot[6]);
        const float ddy = wx0 * wz0 * (dot[2] - dot[0]) + wx1 * wz0 * (dot[3] - dot[1]) +
                          wx0 * wz1 * (dot[6] - dot[4]) + wx1 * wz1 * (dot[7] - dot[5]);
        const float ddz = wx0 * wy0 * (dot[4] - dot[0]) + wx1 * wy0 * (dot[5] - dot[1]) +
                          wx0 * wy1 * (dot[6] - dot[2]) + wx1 * wy1 * (dot[7] - dot[3]);
        dx[0] += s * ddx;
        dx[1] += s * ddy;
        dx[2] += s * ddz;
      }
    }
  }
  }   // grid phases
  if (live && d_x) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float v = dx[a];
      if (scale_by_bound) v = (float)((double)v / (bd.b1[a] - bd.b0[a]));
      d_x[(size_t)p * 3 + a] = v;
    }
  }
}

__global__ __launch_bounds__(256) void hashgrid_indices_kernel(const float* __restrict__ xin, uint32_t P, GridLevels lv,
                                                               uint32_t* __restrict__ rows) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float x[3] = {xin[(size_t)p * 3], xin[(size_t)p * 3 + 1], xin[(size_t)p * 3 + 2]};
  for (uint32_t l = 0; l < lv.n_levels; ++l) {
    uint32_t g[3];
    float f[3];                                    // (not needed here)
    grid_cell(x, lv.scale[l], g, f);
#pragma unroll
    for (int c = 0; c < 8; ++c)
      rows[((size_t)p * lv.n_levels + l) * 8 + c] =
          lv.offset[l] + grid_row(g[0] + (c & 1), g[1] + ((c >> 1) & 1), g[2] + ((c >> 2) & 1), lv.resolution[l],
                                  lv.size[l], lv.hashed[l]);
  }
}

static Bound6 make_bound(const double* bound) {
  Bound6 b;
  for (int a = 0; a < 3; ++a) {
    b.b0[a] = bound ? bound[2 * a] : 0.0;
    b.b1[a] = bound ? bound[2 * a + 1] : 1.0;
    b.inv_unused[a] = 0.0;
  }
  return b;
}

// How many times the tiled encoder uses its LDS tile (encode_fwd_kernel): OneBlob in 1 or 3 phases, the grid in g_ph groups of
// levels.  The tile -- not the 68 registers -- sets this gather kernel's occupancy.  DNS_ENC_PHASES = "pe_ph,g_ph" (measurement knob).
struct EncPhasesEnv {
  uint32_t pe, g;                                // "pe_ph,g_ph": 1 or 3 (else 3), >= 1 (else 2)
  bool set;                                      // the variable exists at all
};
static const EncPhasesEnv& enc_phases_env() {
  static const EncPhasesEnv v = [] {
    EncPhasesEnv e;
    e.pe = env_u32("DNS_ENC_PHASES", 1, 1, 1, 3, 0, &e.set);
    e.g = env_u32("DNS_ENC_PHASES", 1, 0x7fffffff, 1, 2, ',');
    return e;
  }();
  return v;
}
static void encode_tile_phases(uint32_t n_bins, uint32_t n_levels, bool with_pe, uint32_t& pe_ph, uint32_t& g_ph) {
  const EncPhasesEnv& env = enc_phases_env();
  // default 3 + 2 phases (a 17-float tile row, 8.7 KB per workgroup, where one OneBlob phase + one grid phase needs 49 floats, 25 KB:
  // the registers then allow 14 workgroups per CU instead of the tile's 6): 262 144 points along rays 97.1 -> 91.3 us, uniformly
  // random points 155 -> 132 us, the cfg2 step 1.532 -> 1.526 ms (round 5; "3,8": 90.5 / 135.8, "1,2": 95.7 / 153)
  pe_ph = env.pe;
  g_ph = env.g;
  if (!with_pe) pe_ph = 1u;
  if (n_levels == 0u || n_levels % g_ph != 0u || ((2u * n_levels / g_ph) % 8u) != 0u) g_ph = 1u;   // (flush granularity: 8 columns)
  if (pe_ph == 3u && (n_bins % 8u) != 0u) pe_ph = 1u;
}

static int encode_init_attrs() {
  if (hipFuncSetAttribute((const void*)encode_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * (3 * 64 + 1) * (int)sizeof(float)) != hipSuccess ||
      hipFuncSetAttribute((const void*)encode_fwd_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * (3 * 64 + 1) * (int)sizeof(float)) != hipSuccess) {
    set_error("dns_init: hipFuncSetAttribute failed for the tiled encoder kernels");
    return DNS_E_LAUNCH;
  }
  return DNS_OK;
}
static AttrRegistrar encode_attr_registrar(encode_init_attrs);

}  // namespace dns

using namespace dns;

extern "C" int dns_encode_fwd(const float* in, const double* bound, uint32_t P, uint32_t n_bins, const float* table,
                              const DnsGridMeta* meta, float* x_out, float* pe_out, uint32_t ld_pe, float* grid_out,
                              uint32_t ld_grid, float* dy_dx, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(in != nullptr, "dns_encode_fwd: in is NULL");
  DNS_REQUIRE(!dy_dx || grid_out, "dns_encode_fwd: dy_dx needs the grid encoding");
  DNS_REQUIRE(!dy_dx || (((uintptr_t)dy_dx) & 7u) == 0, "dns_encode_fwd: dy_dx must be 8-byte aligned");
  if (pe_out) DNS_REQUIRE(n_bins >= 1 && n_bins <= 64 && ld_pe >= 3 * n_bins, "dns_encode_fwd: n_bins %u / ld_pe %u", n_bins, ld_pe);
  GridLevels lv = {};
  if (grid_out) {
    DNS_REQUIRE(meta && table, "dns_encode_fwd: grid requested without table/meta");
    DNS_REQUIRE(meta->n_features == 2, "dns_encode_fwd: n_features must be 2");
    DNS_REQUIRE(ld_grid >= 2 * meta->n_levels, "dns_encode_fwd: ld_grid %u too small", ld_grid);
    lv = to_levels(meta);
  }
  const uint32_t blocks = (P + 127) / 128;
  const uint32_t pe_dim = 3 * n_bins, g_dim = grid_out ? 2 * meta->n_levels : 0;
  // (OneBlob alone into rows of any width -- Decoder.merge's input rows -- also leaves through the LDS tile: direct row stores at
  //  a lane stride of a whole row cost 3.4x the bytes in HBM writes)
  const bool tiled = (pe_out && grid_out && ld_pe == pe_dim + g_dim && ld_grid == ld_pe && grid_out == pe_out + pe_dim) ||
                     (pe_out && !grid_out && pe_dim > 0);
  if (tiled) {
    uint32_t pe_ph, g_ph;
    encode_tile_phases(n_bins, grid_out ? meta->n_levels : 0, pe_out != nullptr, pe_ph, g_ph);
    const uint32_t w_pe = pe_out ? pe_dim / pe_ph : 0, w_g = grid_out ? g_dim / g_ph : 0;
    const size_t lds_bytes = (size_t)128 * ((w_pe > w_g ? w_pe : w_g) + 1) * sizeof(float);
    DNS_LAUNCH(encode_fwd_kernel<true>, dim3(blocks), dim3(128), lds_bytes, (hipStream_t)stream, in, make_bound(bound),
                       bound ? 1 : 0, P, n_bins, (const float2*)table, lv, x_out, pe_out, ld_pe, grid_out, ld_grid,
                       (float2*)dy_dx, pe_ph, g_ph);
  } else {
    DNS_LAUNCH(encode_fwd_kernel<false>, dim3(blocks), dim3(128), 0, (hipStream_t)stream, in, make_bound(bound),
                       bound ? 1 : 0, P, n_bins, (const float2*)table, lv, x_out, pe_out, ld_pe, grid_out, ld_grid,
                       (float2*)dy_dx, 1u, 1u);
  }
  return check_launch("dns_encode_fwd");
}

extern "C" int dns_encode_fwd_split(const float* in, const double* bound, uint32_t P, uint32_t n_bins, const float* table,
                                    const DnsGridMeta* meta, float* x_out, float* f32_out, uint32_t ld32, void* xs_out,
                                    uint32_t ldxs, int32_t* xexp, uint32_t flags, float* dy_dx, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE((flags & ~(DNS_SPLIT_HI_ONLY | DNS_SPLIT_PLAIN)) == 0, "dns_encode_fwd_split: unknown flags 0x%x", flags);
  const bool plain = (flags & DNS_SPLIT_PLAIN) != 0;       // half rows: unscaled f16, no exponents, hi plane only
  DNS_REQUIRE(in && table && meta && xs_out && (xexp || plain), "dns_encode_fwd_split: NULL argument");
  DNS_REQUIRE(meta->n_features == 2, "dns_encode_fwd_split: n_features must be 2");
  DNS_REQUIRE(!dy_dx || (((uintptr_t)dy_dx) & 7u) == 0, "dns_encode_fwd_split: dy_dx must be 8-byte aligned");
  const uint32_t pe_dim = 3 * n_bins, g_dim = 2 * meta->n_levels, K = pe_dim + g_dim;
  const bool hi_only = (flags & DNS_SPLIT_HI_ONLY) != 0 || plain;
  DNS_REQUIRE(n_bins >= 1 && (pe_dim % 8) == 0 && (g_dim % 8) == 0 && pe_dim <= 64 && g_dim <= 64,
              "dns_encode_fwd_split: OneBlob / grid widths %u / %u must be multiples of 8 and <= 64", pe_dim, g_dim);
  DNS_REQUIRE((ldxs % 8) == 0 && ldxs >= (hi_only ? K : 2 * K) && (((uintptr_t)xs_out) & 15u) == 0,
              "dns_encode_fwd_split: xs_out must be 16-byte aligned with ldxs %% 8 == 0 and ldxs >= %u", hi_only ? K : 2 * K);
  DNS_REQUIRE(!f32_out || ((ld32 % 4) == 0 && ld32 >= K && (((uintptr_t)f32_out) & 15u) == 0),
              "dns_encode_fwd_split: f32_out must be 16-byte aligned with ld32 %% 4 == 0 and ld32 >= %u", K);
  GridLevels lv = to_levels(meta);
  const uint32_t blocks = (P + 127) / 128;
  const size_t lds_bytes = (size_t)128 * ((pe_dim > g_dim ? pe_dim : g_dim) + 1) * sizeof(float);
  if (plain && !f32_out) {
    // half rows alone: the one-pass tiled encoder with an f16 flush (pe_out / grid_out / their strides in halfs)
    _Float16* xh = reinterpret_cast<_Float16*>(xs_out);
    uint32_t pe_ph, g_ph;
    encode_tile_phases(n_bins, meta->n_levels, true, pe_ph, g_ph);
    // the f16 flush writes HALF as many bytes per row and phase: the grid columns leave in ONE phase (64-byte row pieces; two phases
    // = 32-byte pieces cost 0.46 against 0.41 ms per cfg5_fp16 iteration -- the whole step 3.54 against 3.45 --, nothing at cfg2_fp16)
    if (!enc_phases_env().set) g_ph = 1u;
    const uint32_t w_pe = pe_dim / pe_ph, w_g = g_dim / g_ph;
    const size_t lds_plain = (size_t)128 * ((w_pe > w_g ? w_pe : w_g) + 1) * sizeof(float);
    DNS_LAUNCH((encode_fwd_kernel<true, true>), dim3(blocks), dim3(128), lds_plain, (hipStream_t)stream, in, make_bound(bound), bound ? 1 : 0, P,
               n_bins, (const float2*)table, lv, x_out, reinterpret_cast<float*>(xh), ldxs, reinterpret_cast<float*>(xh + pe_dim), ldxs,
               (float2*)dy_dx, pe_ph, g_ph);
    return check_launch("dns_encode_fwd_split");
  }
  DNS_LAUNCH(encode_fwd_split_kernel, dim3(blocks), dim3(128), lds_bytes, (hipStream_t)stream, in, make_bound(bound), bound ? 1 : 0, P,
             n_bins, (const float2*)table, lv, x_out, f32_out, ld32, (uint32_t*)xs_out, ldxs / 2, xexp, (hi_only ? 1 : 0) | (plain ? 2 : 0),
             (float2*)dy_dx);
  return check_launch("dns_encode_fwd_split");
}

extern "C" int dns_encode_bwd(const float* x, const double* bound, uint32_t P, uint32_t n_bins, const float* table,
                              const DnsGridMeta* meta, const float* d_pe, uint32_t ld_dpe, const float* d_grid,
                              uint32_t ld_dgrid, float* d_table, float* d_x, const float* dy_dx, float* ws, uint32_t flags,
                              uint32_t queue_cap, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(x != nullptr, "dns_encode_bwd: x is NULL");
  DNS_REQUIRE(!dy_dx || (((uintptr_t)dy_dx) & 7u) == 0, "dns_encode_bwd: dy_dx must be 8-byte aligned");
  DNS_REQUIRE((flags & ~(DNS_SCATTER_MASK | DNS_SCATTER_REPLAY | DNS_SCATTER_LISTS)) == 0, "dns_encode_bwd: unknown flags 0x%x", flags);
  GridLevels lv = {};
  if (d_grid) {
    DNS_REQUIRE(meta && table, "dns_encode_bwd: d_grid given without table/meta");
    DNS_REQUIRE(meta->n_features == 2, "dns_encode_bwd: n_features must be 2");
    lv = to_levels(meta);
  }
  if (d_pe) DNS_REQUIRE(n_bins >= 1 && n_bins <= 64 && ld_dpe >= 3 * n_bins, "dns_encode_bwd: n_bins %u / ld %u", n_bins, ld_dpe);
  hipStream_t st = (hipStream_t)stream;
  // table gradient: LDS-binned scatter unless the caller asks for the per-corner global atomics (or passes no workspace)
  const bool binned = d_table && d_grid && ws && meta->n_levels <= 16 &&   // measured faster at T=2^16 (17x) and T=2^20 (2.5x)
                      (flags & DNS_SCATTER_MASK) != DNS_SCATTER_ATOMIC;
  if (binned) {
    const int rc = ensure_ready(st, "dns_encode_bwd");
    if (rc != DNS_OK) return rc;
  }
  float* d_table_direct = binned ? nullptr : d_table;
  if (d_x || d_table_direct) {
    const uint32_t blocks128 = (P + 127) / 128;
    const bool tiled = d_pe && d_grid && d_x && ld_dpe == ld_dgrid && d_grid == d_pe + 3 * n_bins &&
                       ld_dpe == 3 * n_bins + 2 * lv.n_levels;
    // OneBlob columns only (Decoder.merge's relative points: 3 x P rows of a [., 48 + 64] matrix per cfg3 iteration): the same
    // tile staging without grid phases -- the direct form's lanes each walk their own 448-byte-strided row (190 us for 786 432
    // rows; through the tile: the rows' 192 bytes come in as coalesced runs)
    const bool tiled_pe = d_pe && !d_grid && d_x && !d_table_direct && 128u * (3u * n_bins + 1u) * sizeof(float) <= 64u * 1024u;
    if (tiled || tiled_pe) {
      uint32_t pe_ph, g_ph;
      encode_tile_phases(n_bins, tiled_pe ? 1u : lv.n_levels, true, pe_ph, g_ph);
      if (tiled_pe) g_ph = 0u;
      if ((n_bins % 4u) != 0u) pe_ph = 1u;              // (the staging reads 16 bytes at a time)
      const uint32_t w_pe = 3 * n_bins / pe_ph, w_g = g_ph ? 2 * lv.n_levels / g_ph : 0u;
      DNS_LAUNCH(encode_bwd_kernel<true>, dim3(blocks128), dim3(128), (size_t)128 * ((w_pe > w_g ? w_pe : w_g) + 1) * sizeof(float), st, x,
                         make_bound(bound), bound ? 1 : 0, P, n_bins, (const float2*)table, lv, d_pe, ld_dpe, d_grid, ld_dgrid,
                         d_table_direct, d_x, (const float2*)dy_dx, pe_ph, g_ph);
    } else {
      DNS_LAUNCH(encode_bwd_kernel<false>, dim3(blocks128), dim3(128), 0, st, x, make_bound(bound), bound ? 1 : 0, P,
                         n_bins, (const float2*)table, lv, d_pe, ld_dpe, d_grid, ld_dgrid, d_table_direct, d_x,
                         (const float2*)dy_dx, 1u, 1u);
    }
  }
  if (binned) {
    const ScatterPlan plan = scatter_plan(P, lv, flags, queue_cap, scatter_knobs_env());
    DNS_REQUIRE(!plan.n_replay || (((uintptr_t)ws) & 15u) == 0, "dns_encode_bwd: DNS_SCATTER_REPLAY needs a 16-byte aligned workspace");
    DNS_REQUIRE(plan.lds_ok, "dns_encode_bwd: the pair-list bins (%zu B: DNS_LIST_SHIFT=%u, %u lists) exceed the "
                "%d B of LDS a workgroup can have", (size_t)plan.list_bins.lds, plan.lp.chunk_shift, plan.lp.qoff[plan.lp.n], MAX_DYN_LDS);
    const int rc = launch_table_scatter(x, P, lv, d_grid, ld_dgrid, d_table, ws, plan, st);
    if (rc != DNS_OK) return rc;
  }
  return check_launch("dns_encode_bwd");
}

extern "C" int dns_hashgrid_indices(const float* x, uint32_t P, const DnsGridMeta* meta, uint32_t* rows, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(x && meta && rows, "dns_hashgrid_indices: NULL argument");
  DNS_LAUNCH(hashgrid_indices_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, P,
                     to_levels(meta), rows);
  return check_launch("dns_hashgrid_indices");
}

extern "C" uint64_t dns_encode_bwd_ws_floats(uint32_t P, const DnsGridMeta* meta, uint32_t flags, uint32_t queue_cap) {
  if (!meta) return 0;
  const GridLevels lv = to_levels(meta);
  return scatter_plan(P, lv, flags, queue_cap, scatter_knobs_env()).total;
}
