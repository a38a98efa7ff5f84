// Host arithmetic of dns_frame_codes (frame_codes.hip): the tiling of the points, the grid, the LDS plan and the workgroup-private
// slices of the global workspace.  No HIP in here: tools/frame_codes_plan_check.cpp walks it on the host under ASan + UBSan.
//
// A 256-thread workgroup owns tiles of tile_pts points (tile t of workgroup b: b, b + blocks, ...).  For one tile it holds, in ITS
// slice of the workspace, the Merge rows of all R views -- slot r * npts + pl, [R * tile_pts][n_in] floats -- followed by their
// latents, [R * tile_pts][hid] floats.  tile_pts is 128 (the MLP body's 4 waves x 32 slots) where the points fill every
// workgroup slot of the device four times over.  Below that a workgroup's time is the latency of ONE tile's chain of phases, which
// grows with the tile's R * tile_pts rows: the tile is the largest of 128, 64, 32 with at most 256 rows (measured at 47 000
// points, DESIGN 4.20: 128 for one view, 64 for three).
// The LDS is the MLP forward body's area (weight images + staging, mlp_lds bytes) followed by the OneBlob tile: PE_ROWS rows of n_pe + 1 floats (odd stride: conflict-free for lane = row).
#pragma once
#include <stdint.h>

namespace dns {
namespace fc {

constexpr uint32_t TILE_PTS = 128;            // most points per tile: the MLP body's 4 waves x 32 slots
constexpr uint32_t TILE_FILL = 4;             // tiles of 128 per workgroup slot from which the tile is 128 whatever R
constexpr uint32_t TILE_ROWS = 256;           // below that: the largest tile whose R views make at most this many rows
constexpr uint32_t THREADS = 256;
constexpr uint32_t PE_ROWS = 256;             // (point, view) pairs whose OneBlob columns are staged per pass: one per thread
constexpr uint32_t MAX_VIEWS = 64;            // R * TILE_PTS * n_in * 4 bytes stays far below the 2 GiB a buffer descriptor addresses
constexpr uint32_t LDS_LIMIT = 160u * 1024u;  // gfx950: LDS per CU, all of it available to one workgroup
constexpr uint32_t N_CU = 256;                // MI355X; a device with fewer runs the workgroups in turns
constexpr uint64_t MAX_POINTS = 1ull << 31;

struct Plan {
  bool ok;                                    // false: refused (no points or views, too many of either, LDS over the limit)
  uint32_t tile_pts, n_tiles, blocks;
  uint32_t tile_off, lds_bytes;               // byte offset of the OneBlob tile in the dynamic LDS; the launch's dynamic LDS
  uint32_t rows_floats;                       // floats of a slice's row block; the latents follow
  uint64_t slice_floats, ws_floats;           // floats per workgroup / in all (a multiple of 4 each: 16-byte aligned slices)
};

// tile_pts: 0 = chosen here; 32, 64 or 128 = the caller's (tests, tools)
inline Plan plan(uint64_t P, uint32_t R, uint32_t n_pe, uint32_t C, uint32_t hid, uint32_t mlp_lds, uint32_t tile_pts = 0) {
  Plan p = {};
  if (P == 0 || P >= MAX_POINTS || R == 0 || R > MAX_VIEWS) return p;
  if (n_pe == 0 || n_pe % 4 != 0 || C == 0 || C % 4 != 0 || n_pe + C > 128 || hid == 0 || hid % 4 != 0 || hid > 64) return p;
  if (mlp_lds == 0 || mlp_lds % 16 != 0 || mlp_lds > LDS_LIMIT) return p;
  if (tile_pts != 0 && tile_pts != 32 && tile_pts != 64 && tile_pts != 128) return p;
  const uint64_t lds = (uint64_t)mlp_lds + (uint64_t)PE_ROWS * (n_pe + 1u) * 4u;
  if (lds > LDS_LIMIT) return p;
  p.tile_off = mlp_lds;
  p.lds_bytes = (uint32_t)((lds + 15u) & ~15ull);
  if (p.lds_bytes > LDS_LIMIT) p.lds_bytes = LDS_LIMIT;
  const uint32_t per_cu = LDS_LIMIT / p.lds_bytes >= 2u ? 2u : 1u;
  const uint32_t cap = N_CU * per_cu;
  if (tile_pts == 0) {
    tile_pts = TILE_PTS;
    if (P < (uint64_t)TILE_PTS * TILE_FILL * cap)
      while (tile_pts > 32u && R * tile_pts > TILE_ROWS) tile_pts /= 2u;
  }
  p.tile_pts = tile_pts;
  p.n_tiles = (uint32_t)((P + tile_pts - 1u) / tile_pts);
  p.blocks = p.n_tiles < cap ? p.n_tiles : cap;
  p.rows_floats = R * tile_pts * (n_pe + C);
  p.slice_floats = (uint64_t)p.rows_floats + (uint64_t)R * tile_pts * hid;
  p.ws_floats = p.slice_floats * p.blocks;
  p.ok = true;
  return p;
}

// tile t: its first point and how many it holds
inline uint64_t tile_first(uint32_t t, uint32_t tile_pts) { return (uint64_t)t * tile_pts; }
inline uint32_t tile_points(uint64_t P, uint32_t t, uint32_t tile_pts) {
  const uint64_t p0 = tile_first(t, tile_pts);
  return p0 >= P ? 0u : (uint32_t)(P - p0 < tile_pts ? P - p0 : tile_pts);
}
// the slot of (view r, point pl of the tile) among the tile's R * npts rows
inline uint32_t pair_slot(uint32_t r, uint32_t pl, uint32_t npts) { return r * npts + pl; }

}  // namespace fc
}  // namespace dns
