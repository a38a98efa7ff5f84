// Host arithmetic of the fused tracker iteration's STEM form (track_fused.inc with DNS_TF_STEM, launched by track.hip): the
// workgroup-private slices of the 2-D branch's rows in the global workspace and the LDS plan.  No HIP in here:
// tools/track_stem_plan_check.cpp walks it on the host under ASan + UBSan.
//
// A workgroup owns rpw rays = up to rpw * S <= 128 points and, with R reference views, R * npts (point, view) rows; row (r, pl)
// sits at r * npts + pl (the order of dns_feature_gather_frames).  Its slice holds, in this order and each 256-byte aligned:
//   rows   [R * cap][n_pe + Cs]   Merge's input: OneBlob of the normalised relative point | the view's code
//   lat    [R * cap][hid]         Merge's output
//   dy     [R * cap][hid]         its gradient
//   dpe    [R * cap][n_pe]        the gradient of the OneBlob columns
//   xm     [R * cap][3]           the normalised relative point (OneBlob's backward reads it)
//   drel   [R * cap][3]           d(relative point)
// with cap = rpw * S.  The slices follow the kernel's other rows (`base` floats, a multiple of 64) workgroup after workgroup.
// LDS: [0, keep_off) is shared by the network phases (the largest of the four networks' areas) and the staging tiles -- the
// OneBlob tile of PE_ROWS rows of n_pe + 1 floats among them --, then the persistent region of keep_bytes, then the views'
// poses (VIEW_FLOATS each: the first three rows of w2c, the origin).
#pragma once
#include <stdint.h>

namespace dns {
namespace tfs {

constexpr uint32_t MAX_VIEWS = 8;             // following views are a bit mask; 8 * 128 rows * 128 floats stays far below 2 GiB
constexpr uint32_t VIEW_FLOATS = 16;          // w2c rows 0..2 (12) | origin (3) | pad
constexpr uint32_t VIEWS_BYTES = MAX_VIEWS * VIEW_FLOATS * 4u;
constexpr uint32_t PE_ROWS = 256;             // (point, view) rows whose OneBlob columns are staged per pass: one per thread
constexpr uint32_t WG_POINTS = 128;           // most points of a workgroup
constexpr uint32_t LDS_LIMIT = 160u * 1024u;  // gfx950: LDS per CU, all of it available to one workgroup

struct StemPlan {
  bool ok;
  uint32_t cap;                               // points a workgroup's slice is sized for (rpw * S)
  uint32_t n_wg;
  uint32_t rows, lat, dy, dpe, xm, drel;      // float offsets inside a slice
  uint32_t slice_floats;                      // a multiple of 64
  uint64_t base, total_floats;                // where the slices start; the whole workspace
  uint32_t tile_bytes, keep_off, views_off, lds_bytes;
};

inline uint32_t al64(uint32_t v) { return (v + 63u) & ~63u; }

// mlp_lds: LDS bytes of the largest network phase (a multiple of 16); keep_bytes: the persistent region; base: floats in front
inline StemPlan stem_plan(uint32_t N, uint32_t S, uint32_t rpw, uint32_t R, uint32_t n_pe, uint32_t Cs, uint32_t hid, uint32_t mlp_lds,
                          uint32_t keep_bytes, uint64_t base) {
  StemPlan p = {};
  if (N == 0 || S == 0 || rpw == 0 || rpw * S > WG_POINTS || R == 0 || R > MAX_VIEWS) return p;
  if (n_pe == 0 || n_pe % 4 != 0 || Cs == 0 || Cs % 4 != 0 || n_pe + Cs > 128 || hid == 0 || hid % 4 != 0 || hid > 64) return p;
  if (mlp_lds == 0 || mlp_lds % 16 != 0 || keep_bytes % 16 != 0 || base % 64 != 0) return p;
  p.cap = rpw * S;
  p.n_wg = (N + rpw - 1u) / rpw;
  const uint32_t nr = R * p.cap;
  uint32_t o = 0;
  p.rows = o; o = al64(o + nr * (n_pe + Cs));
  p.lat = o; o = al64(o + nr * hid);
  p.dy = o; o = al64(o + nr * hid);
  p.dpe = o; o = al64(o + nr * n_pe);
  p.xm = o; o = al64(o + nr * 3u);
  p.drel = o; o = al64(o + nr * 3u);
  p.slice_floats = o;
  p.base = base;
  p.total_floats = base + (uint64_t)p.n_wg * p.slice_floats;
  p.tile_bytes = PE_ROWS * (n_pe + 1u) * 4u;
  const uint32_t shared = mlp_lds > p.tile_bytes ? mlp_lds : p.tile_bytes;
  p.keep_off = (shared + 15u) & ~15u;
  p.views_off = p.keep_off + keep_bytes;
  const uint64_t lds = (uint64_t)p.views_off + VIEWS_BYTES;
  if (lds > LDS_LIMIT) return p;
  p.lds_bytes = (uint32_t)lds;
  p.ok = true;
  return p;
}

// the row of (view r, point pl) among a workgroup's R * npts rows
inline uint32_t pair_row(uint32_t r, uint32_t pl, uint32_t npts) { return r * npts + pl; }

}  // namespace tfs
}  // namespace dns
