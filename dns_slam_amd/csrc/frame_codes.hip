// The 2-D code of a rendered frame's samples, reference view by reference view, in ONE kernel: what the reference computes inside
// the chunk loops of frame_vis (slams/mapping.py:666-689) and novel_view_render (eval_2d.py:260-283) with feature_matching
// (utils/common.py:645-679) and Decoder.merge (models/decoder.py:67-77).  As launches (common.feature_matching: dns_feature_gather
// -> dns_encode_fwd -> torch.cat -> dns_mlp_fwd -> torch.mean) every (point, view) pair moves about 2 KB through HBM for the 128
// bytes per POINT that come out; here a workgroup makes, uses and drops its Merge rows in a private slice of a workspace.
//
// A 256-thread workgroup owns tiles of up to 128 points (frame_codes_plan.hpp: 32 or 64 where the points are few) and keeps the Merge weight images in its LDS for all of
// them (build_fwd_images, once).  Per tile:
//   A  for every view: project, gather, OneBlob.  16 lanes per (point, view) pair and one float4 of channels per lane, as
//      feature_gather4_kernel (feature.hip) on the functions of dev_feature.hpp; the OneBlob columns of rel = p - o_r, normalised with the scene bound
//      in fp64 (dev_encode.hpp: the encoder's functions), go through an LDS tile and leave as contiguous float4 runs.  Both land
//      in the workgroup's private slice of a global workspace (72 KB per view and 128 points; which cache holds it is not
//      measured, and at a full grid the slices exceed L2: DESIGN 4.20), the way track_fused.inc hands rows
//      between its phases.
//   B  mlp_fwd_body (mlp_split.hpp: the body dns_mlp_fwd runs) on the tile's R * npts rows -> their latents, same slice.
//   C  the R latents of a point added in ascending view order, divided by R, stored once as whole 128-byte lines.  A point
//      with keep == 0 gets a zero row (and had none of its taps read).
// No atomics: a point's bits depend on the point, the views and the weights alone.
//
// Contraction: feature.hip and encode.hip are compiled with -ffp-contract=off, mlp_split.hip is not, and this unit must give the
// bits of all three -- it is compiled like mlp_split.hip, and the normalisation carries the setting as a function-level pragma
// (the projection and the taps are dev_feature.hpp's functions, which carry their own, as dev_encode.hpp's do).
#include "mlp_split.hpp"
#include "dev_encode.hpp"
#include "dev_feature.hpp"
#include "frame_codes_plan.hpp"

namespace dns {
namespace fc {

// (explicit LDS pointers: see track_fused.inc -- a pointer into the dynamic LDS that went through arithmetic on a kernel
//  argument is a generic pointer to hipcc)
typedef __attribute__((address_space(3))) float* lds_fp;

struct Args {
  const float* pts;                          // [P,3]
  const float* w2c;                          // [R,16]
  const float* origin;                       // [R,3]
  Mat3 K;
  const float* feat;                         // [R,h,w,C]
  const uint8_t* keep;                       // [P] or NULL
  const float* params;                       // the Merge network's fp32 weights
  double b0[3], b1[3];                       // Merge's bound
  uint32_t P, R, C, n_bins, hid;
  int h, w, H, W;
  float* ws;
  uint32_t rows_floats, slice_floats, tile_off, n_tiles, tile_pts;
  float* out;
  uint32_t ld_out;
  uint32_t* err;
};

// (a pair's code and its normalised relative point: pair_code / pair_rel of dev_feature.hpp, shared with track_fused.inc)

namespace {

template <int NN, int NL>
__global__ __launch_bounds__(256) void frame_codes_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t pe = 3u * a.n_bins, ld = pe + a.C, hid = a.hid, R = a.R;
  float* __restrict__ rows = a.ws + (size_t)blockIdx.x * a.slice_floats;      // [R * npts][ld]
  float* __restrict__ lat = rows + a.rows_floats;                             // [R * npts][hid]
  lds_fp tile = (lds_fp)(lds + a.tile_off);                                    // [PE_ROWS][pe + 1]
  // the Merge weight images: once per workgroup, for all its tiles
  sp::build_fwd_images<NN, NL>(lds, a.params, ld, hid);
  __syncthreads();
  sp::FwdArgs fa = {};
  fa.x = rows; fa.ldx = ld; fa.seg = {nullptr, 0u, ld};
  fa.params = a.params;
  fa.n_in = ld; fa.n_in_w = ld; fa.n_out = hid;
  fa.y = lat; fa.ldy = hid;
  fa.tiles_per_block = R;                                                      // ceil(R npts / 128) <= R
  fa.err = a.err;
  const float den = (float)R;
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint32_t p0 = t * a.tile_pts, npts = min(a.tile_pts, a.P - p0), nrows = R * npts;
    // ---- A: the rows.  Codes: 16 pairs per pass of the workgroup
    {
      const uint32_t sub = tid & 15u;
#pragma unroll 1
      for (uint32_t i0 = 0; i0 < nrows; i0 += 16u) {
        const uint32_t i = i0 + (tid >> 4);
        if (i < nrows) {
          const uint32_t r = i / npts, pl = i - r * npts;
          const size_t p = (size_t)p0 + pl;
          const bool kept = a.keep == nullptr || a.keep[p] != 0;
          pair_code(a.w2c + 16 * r, a.K, a.feat + (size_t)r * a.h * a.w * a.C, a.C, a.h, a.w, a.H, a.W, a.pts[p * 3], a.pts[p * 3 + 1],
                    a.pts[p * 3 + 2], kept, sub, rows + (size_t)i * ld + pe);
        }
      }
    }
    // OneBlob: one pair per thread into the LDS tile, then out as contiguous float4 runs
    for (uint32_t i0 = 0; i0 < nrows; i0 += PE_ROWS) {
      const uint32_t i = i0 + tid;
      if (i < nrows) {
        const uint32_t r = i / npts, pl = i - r * npts;
        const size_t p = (size_t)p0 + pl;
        const float pt[3] = {a.pts[p * 3], a.pts[p * 3 + 1], a.pts[p * 3 + 2]};
        const float og[3] = {a.origin[r * 3], a.origin[r * 3 + 1], a.origin[r * 3 + 2]};
        float x[3];
        pair_rel(pt, og, a.b0, a.b1, x);
        lds_fp rowp = tile + tid * (pe + 1u);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) oneblob_axis_fwd(x[ax], a.n_bins, rowp + ax * a.n_bins);
      }
      __syncthreads();
      const uint32_t nq = pe / 4u, cnt = min(PE_ROWS, nrows - i0);
      for (uint32_t j = tid; j < cnt * nq; j += THREADS) {
        const uint32_t rr = j / nq, c = j - rr * nq;
        const lds_fp s = tile + rr * (pe + 1u) + 4u * c;
        *reinterpret_cast<float4*>(rows + (size_t)(i0 + rr) * ld + 4u * c) = make_float4(s[0], s[1], s[2], s[3]);
      }
      __syncthreads();
    }
    // ---- B: the Merge network on the tile's rows (the images are in place)
    fa.n_slots = nrows;
    sp::mlp_fwd_body<NN, NL, 3>(fa, 0u, lds, true);
    __syncthreads();
    // ---- C: mean over the views, in view order
    {
      const uint32_t qh = hid / 4u;
      for (uint32_t j = tid; j < npts * qh; j += THREADS) {
        const uint32_t pl = j / qh, q = j - pl * qh;
        const float* src = lat + (size_t)pl * hid + 4u * q;
        float4 s = *reinterpret_cast<const float4*>(src);
        for (uint32_t r = 1; r < R; ++r) {
          const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * npts * hid);
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        s.x /= den; s.y /= den; s.z /= den; s.w /= den;
        const size_t p = (size_t)p0 + pl;
        if (a.keep != nullptr && a.keep[p] == 0) s = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(a.out + p * a.ld_out + 4u * q) = s;
      }
    }
    // (the next tile's phase A writes the row block and the LDS tile, which phase C does not read; its barriers stand between
    //  this phase's reads of the latents and phase B's next stores to them)
  }
}

}  // namespace

static bool shape_ok(uint32_t nn, uint32_t nl) { return (nn == 32 && nl == 1) || (nn == 64 && nl == 2); }

static uint32_t mlp_lds(uint32_t n_in, uint32_t hid, uint32_t nn, uint32_t nl) {
  if (n_in < 8 || n_in > 128 || n_in % 8 != 0 || hid < 1 || hid > 64) return 0u;
  const uint32_t b = nn == 32 ? sp::FwdLds<32, 1>::total(n_in, hid, 4) : sp::FwdLds<64, 2>::total(n_in, hid, 4);
  return (b + 15u) & ~15u;
}

static int fc_init_attrs() {
  const bool ok =
      hipFuncSetAttribute((const void*)frame_codes_kernel<32, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess &&
      hipFuncSetAttribute((const void*)frame_codes_kernel<64, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess;
  if (!ok) {
    set_error("dns_init: hipFuncSetAttribute failed for the frame-code kernels");
    return DNS_E_LAUNCH;
  }
  return DNS_OK;
}
static AttrRegistrar fc_attr_registrar(fc_init_attrs);

}  // namespace fc
}  // namespace dns

using namespace dns;

extern "C" uint64_t dns_frame_codes_ws_floats(uint32_t P, uint32_t R, uint32_t n_bins, uint32_t C, uint32_t hid, uint32_t n_neurons,
                                              uint32_t n_hidden_layers, uint32_t tile_pts) {
  if (!fc::shape_ok(n_neurons, n_hidden_layers) || n_bins == 0 || n_bins > 42) return 0;
  const fc::Plan pl = fc::plan(P, R, 3u * n_bins, C, hid, fc::mlp_lds(3u * n_bins + C, hid, n_neurons, n_hidden_layers), tile_pts);
  return pl.ok ? pl.ws_floats : 0;
}

extern "C" int dns_frame_codes(const float* pts, uint32_t P, const float* w2c, const float* origin, uint32_t R, const float* K,
                               const float* feat, uint32_t C, int h, int w, int H, int W, const uint8_t* keep, const double* bound,
                               uint32_t n_bins, const float* params, uint32_t n_neurons, uint32_t n_hidden_layers, uint32_t hid,
                               float* ws, uint64_t ws_floats, float* out, uint32_t ld_out, uint32_t tile_pts, void* stream) {
  if (P == 0) return DNS_OK;
  DNS_REQUIRE(pts && w2c && origin && K && feat && bound && params && ws && out, "dns_frame_codes: NULL argument");
  DNS_REQUIRE(fc::shape_ok(n_neurons, n_hidden_layers), "dns_frame_codes: a Merge network of %u neurons x %u hidden layers (32 x 1 or 64 x 2)",
              n_neurons, n_hidden_layers);
  DNS_REQUIRE(n_bins >= 1 && n_bins <= 42 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "dns_frame_codes: bad dimensions");
  const fc::Plan pl = fc::plan(P, R, 3u * n_bins, C, hid, fc::mlp_lds(3u * n_bins + C, hid, n_neurons, n_hidden_layers), tile_pts);
  DNS_REQUIRE(pl.ok, "dns_frame_codes: refused shape: %u points, %u views, %u OneBlob + %u stem columns, %u outputs, tiles of %u", P, R, 3u * n_bins, C, hid, tile_pts);
  DNS_REQUIRE(ws_floats >= pl.ws_floats, "dns_frame_codes: workspace of %llu floats, %llu needed", (unsigned long long)ws_floats,
              (unsigned long long)pl.ws_floats);
  DNS_REQUIRE(ld_out >= hid && ld_out % 4 == 0, "dns_frame_codes: ld_out %u for %u outputs (a multiple of 4)", ld_out, hid);
  DNS_REQUIRE((((uintptr_t)feat | (uintptr_t)ws | (uintptr_t)out | (uintptr_t)params) & 15) == 0, "dns_frame_codes: feat, params, ws and out must be 16-byte aligned");
  DNS_REQUIRE((uint64_t)R * h * w * C < (1ull << 40), "dns_frame_codes: stem maps too large");
  const int rc = ensure_ready((hipStream_t)stream, "dns_frame_codes");
  if (rc != DNS_OK) return rc;
  fc::Args a = {};
  a.pts = pts; a.w2c = w2c; a.origin = origin; a.feat = feat; a.keep = keep; a.params = params;
  for (int i = 0; i < 9; ++i) a.K.k[i] = K[i];
  for (int k = 0; k < 3; ++k) {
    a.b0[k] = bound[2 * k];
    a.b1[k] = bound[2 * k + 1];
  }
  a.P = P; a.R = R; a.C = C; a.n_bins = n_bins; a.hid = hid;
  a.h = h; a.w = w; a.H = H; a.W = W;
  a.ws = ws; a.rows_floats = pl.rows_floats; a.slice_floats = (uint32_t)pl.slice_floats; a.tile_off = pl.tile_off; a.n_tiles = pl.n_tiles; a.tile_pts = pl.tile_pts;
  a.out = out; a.ld_out = ld_out;
  a.err = device_error_word();
  if (n_neurons == 32) DNS_LAUNCH((fc::frame_codes_kernel<32, 1>), dim3(pl.blocks), dim3(fc::THREADS), pl.lds_bytes, (hipStream_t)stream, a);
  else DNS_LAUNCH((fc::frame_codes_kernel<64, 2>), dim3(pl.blocks), dim3(fc::THREADS), pl.lds_bytes, (hipStream_t)stream, a);
  return check_launch("dns_frame_codes");
}
