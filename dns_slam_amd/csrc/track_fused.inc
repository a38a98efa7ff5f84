// The tracker's optimise iteration as ONE kernel per iteration (+ one small pose kernel): SURVEY section 7 step 6's whole-ray
// kernel, built where the path is latency-bound -- reference slams/tracking.py:313-340 (the loop), :128-186 (get_target_samples),
// :188-214 (renderer), :85-96 (losses), with the scene frozen (:120-124: pose-only Adam).  Included by track_fused_<NN>_<NL>.hip
// with DNS_BWD_NN / DNS_BWD_NL defined (the MLP bodies are the ones of mlp_split.hpp / mlp_split_bwd.inc).
//
// Round 4's TrackStep ran the iteration as 28 launches, 17 of them under 6 us (0.25 ms per iteration, 500 rays x 64 samples =
// 32 768 points: one tile per wave in every MLP launch).  Here a 256-thread workgroup OWNS rpw rays (rpw S <= 128 points) from
// the pixel draw to their share of the pose gradient:
//   1  ray generation, box clip, depth-guided z (wave-shuffle sort), pts = o + d z, fp64 normalisation, OneBlob + hash-grid
//      gather with d(feature)/dx kept (4 / rpw waves per ray: the levels are split over them)          utils/common.py:248-304,561-599
//   2  coarse network forward                                                                         models/decoder.py:80-94
//   3  feature block [latent | code x truncation mask]                                                slams/tracking.py:162-176
//   4  colour + logit networks forward                                                                models/decoder.py:97-125
//   5  compositing, the three masked ray losses, their gradients, compositing backward                utils/common.py:506-537, tracking.py:85-96
//   6  colour / logit / coarse networks backward (input gradients only)
//   7  OneBlob + grid input gradient, d pts, the rays' sums of dL/dR, dL/dT
// The phases hand their [points, .] rows over through global scratch that only this workgroup touches (L2-resident: 10 MB for
// the whole batch) behind workgroup barriers; each MLP phase copies its prepared operand images (dns_mlp_prepare) into LDS.
// What is GLOBAL in the reference's iteration is kept out of the kernel's critical path: max(gt_depth) of the draw does not
// depend on the pose (computed for all iterations of a frame up front, dns_track_fused_begin); the masked means' denominator
// n_valid scales EVERY term of the loss, so the workgroups work with n_valid = 1 and the pose kernel divides the summed
// gradient and loss by the summed count (one rounding instead of one per ray: the only arithmetic difference to TrackStep).
// The pose kernel (one workgroup) adds the workgroups' partial sums in a fixed order, forms the loss, keeps the best pose
// (tracking.py:326-335), runs the quaternion chain rule (utils/common.py:406-429) and Adam (torch.optim.Adam semantics, adam.hip).
#include <type_traits>
#ifdef DNS_TF_STEM
#define DNS_RN_NO_CONTRACT                   // dev_rn.hpp: sampling and grid cells round as sample.hip's / encode.hip's do
#define DNS_TF_FP _Pragma("clang fp contract(off)")
#else
#define DNS_TF_FP
#endif
#define DNS_BWD_BODY_ONLY
#include "mlp_split_bwd.inc"
#include "dev_sample.hpp"
#include "dev_encode.hpp"
#include "dev_composite.hpp"
#include "track_fused.hpp"
#ifdef DNS_TF_STEM
#include "dev_feature.hpp"
#include "track_stem_plan.hpp"
#endif

namespace dns {
namespace tf {

#define NN DNS_BWD_NN
#define NL DNS_BWD_NL

// (explicit LDS pointers: a pointer into the dynamic LDS that went through arithmetic on a kernel argument is a GENERIC
//  pointer to hipcc -- flat_load / flat_store, which also count in vmcnt and force vmcnt(0) waits around them)
typedef __attribute__((address_space(3))) float* lds_fp;
struct RayLds {
  lds_fp z;
  lds_fp w;
  lds_fp dsem;
  lds_fp m;                                  // o[0..2] d[3..5] dir[6..8] gtc[9..11] gd[12] valid[13] label[14]
  lds_fp loss;
  lds_fp pose;
};
__device__ __forceinline__ RayLds ray_lds(lds_fp keep, uint32_t r) {
  lds_fp b = keep + r * TF_RAY_FLOATS;
  return {b, b + 64, b + 128, b + 192, b + 208, b + 212};
}

// (anonymous namespace: every translation unit instantiates track_fused_kernel<MTL> for ITS network shape -- with external
//  linkage the two instantiations share one mangled name and the linker keeps one of them for both launchers)
namespace {

// The STEM form (DNS_TF_STEM, track_fused_stem_*.hip; DESIGN 4.23): the 2-D branch of a stem-trained map -- feature_matching +
// Decoder.merge on the iteration's points (slams/tracking.py:162-165), which depends on the pose and so cannot be finished ahead
// of the loop -- runs inside the kernel.  With R reference views the workgroup owns R npts (point, view) rows, row (r, pl) at
// r npts + pl, in a private slice of the workspace (track_stem_plan.hpp).  Added phases:
//   3a  per row: projection, bilinear taps, code (pair_code, dev_feature.hpp: frame_codes.hip's phase A) and the OneBlob columns
//       of rel = p - o_r normalised with Merge's bound (pair_rel), through the LDS staging tile.  A pair outside its view, or of
//       a sample outside the truncation band (its code is multiplied by 0 below and receives no gradient), is a zero code
//       and reads no tap.  A FOLLOWING view (slams/tracking.py:316-319) takes its pose from (quat, trans) at kernel entry.
//   3b  Merge forward on the rows (tiles_per_block = R)
//   3c  inside phase 3: the code = the views' sum in ascending view order x 1 / R x truncation mask (dns_feature_block_split's order)
//   6a  behind the colour / logit backward: d_lat(r, p) = d_code(p) trunc(p) / R (dns_merge_dy), Merge backward (input gradient of
//       the first segment only: DNS_MLP_DX_FIRST's form), OneBlob backward, d rel = d x / (b1 - b0) in fp64
//   7   d pts += the views' d rel in ascending view order (dns_add_ref_sum), behind the encoder's share
// No atomics, fixed orders.  NCHM: Merge's input width in 32-column chunks (3 or 4).
#ifdef DNS_TF_STEM
template <int MTL, int NCHO, int NCHM>
__global__ __launch_bounds__(256, 1) void track_fused_kernel(TrackArgs a, StemArgs sa) {
#else
template <int MTL, int NCHO>
__global__ __launch_bounds__(256, 1) void track_fused_kernel(TrackArgs a) {
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr uint32_t NCHC = 3, MTC = 2;                       // coarse: 65..96 inputs, 33..64 outputs; colour / logit: NCHO = 3 (65..96) or 4 (97..128)
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t wg = blockIdx.x;
  const uint32_t N = a.N, S = a.S, P = N * S, rpw = a.rpw, wpr = 4u / rpw;
  const uint32_t pe = 3u * a.n_bins, L = a.lv.n_levels, ld = pe + 2u * L;
  const uint32_t hid = a.hid, nf = a.nf, C = a.C, ldf = 4u + nf;
  const uint32_t n0 = wg * rpw, n1 = min(n0 + rpw, N);          // the workgroup's rays
  const uint32_t p0 = n0 * S, npts = (n1 - n0) * S;             // ... and points
  const uint32_t it = min(a.iter[0], a.n_iters - 1u);                                   // the frame's it-th draws
  const int64_t* __restrict__ pix = a.pix + (size_t)it * N;
  const float* __restrict__ t_surf = a.t_surf + (size_t)it * a.ns;
  const float* __restrict__ t_zero = a.t_zero + (size_t)it * a.ns;
  lds_fp tile = (lds_fp)lds;                                      // [points of the workgroup][ld + 1] staging tile of phases 1 and 7
  lds_fp keep = (lds_fp)(lds + a.keep_off);                       // persists across the MLP phases (they use [0, keep_off))
  lds_fp dxp = keep + 4 * TF_RAY_FLOATS;
#ifdef DNS_TF_STEM
  // the views' poses (first three rows of w2c | origin) in LDS behind the persistent region: a following view's from the pose
  // this iteration's rays are cast from (refer_poses_kernel's arithmetic, dev_feature.hpp), the others' as stored.  Read from
  // phase 3a on, behind phase 1's barriers.
  lds_fp views = (lds_fp)(lds + sa.views_off);
  if (threadIdx.x < sa.R) {
    const uint32_t r = threadIdx.x;
    lds_fp v = views + r * tfs::VIEW_FLOATS;
    if ((sa.follow >> r) & 1u) {
      double A[9], t[3];
      pose_from_quat(a.quat, a.trans, A, t);
      pose_inverse<true>(A, t, v, v + 12);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] = sa.w2c[16u * r + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[12 + k] = sa.origin[3u * r + k];
    }
  }
#endif

  // ---- 1: rays, samples, encoding ---------------------------------------------------------------------------------------
  {
    DNS_TF_FP                                  // (stem form: d, pts and their normalisation round as raygen_sample_kernel / load_point do)
    const uint32_t r = wave / wpr, part = wave - r * wpr, n = n0 + r;
    if (n < n1) {
      int row, col;
      float dir[3];
      pixel_dir(pix[n], a.H0, a.W0, a.wwin, a.cam, row, col, dir);
      const size_t pixi = (size_t)row * a.W + col;
      float R[9];
      quat_to_R(a.quat, R);
      float o[3], d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        o[k] = a.trans[k];
        d[k] = DNS_FADD(DNS_FADD(DNS_FMUL(dir[0], R[3 * k]), DNS_FMUL(dir[1], R[3 * k + 1])), DNS_FMUL(dir[2], R[3 * k + 2]));
      }
      const float gd = a.depth[pixi];
      double far = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double t0 = (a.bd.b[2 * k] - (double)o[k]) / (double)d[k];
        const double t1 = (a.bd.b[2 * k + 1] - (double)o[k]) / (double)d[k];
        const double m = max_nan(t0, t1);
        far = (k == 0) ? m : min_nan(far, m);
      }
      const bool in = far >= (double)gd;
      far += 0.01;
      uint32_t key[1];
      sample_and_sort<1>(gd, far, __uint_as_float(a.dmax[it]), a.t_uniform, t_surf, t_zero, a.nu, a.ns, lane, key);
      if (a.n_phases == 11u) return;                  // (tools: behind ray generation + sort)
      RayLds rl = ray_lds(keep, r);
      if (part == 0u && lane == 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          rl.m[k] = o[k];
          rl.m[3 + k] = d[k];
          rl.m[6 + k] = dir[k];
          rl.m[9 + k] = a.color[pixi * 3 + k];
        }
        rl.m[12] = gd;
        rl.m[13] = (gd > 0.01f && in) ? 1.f : 0.f;             // slams/tracking.py:171-172
        rl.m[14] = __int_as_float((int)a.label[pixi]);
      }
      if (lane < S) {
        const float zv = key2f(key[0]);
        const uint32_t p = n * S + lane;
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float pt = DNS_FADD(o[k], DNS_FMUL(d[k], zv));
          x[k] = (float)(((double)pt - a.b6.b0[k]) / (a.b6.b1[k] - a.b6.b0[k]));
        }
        // the point's row goes to an LDS tile (row stride ld + 1: conflict-free for lane = point; the MLP phases' LDS is free
        // here) and leaves below as one contiguous, coalesced run -- per-lane row stores at a 320-byte stride touched 64 cache
        // lines per instruction, ~130 instructions per lane
        lds_fp rowp = tile + (p - p0) * (ld + 1u);
        // Work split of a ray's waves (measured: one OneBlob axis ~2 us, one grid level ~0.75 us at one wave per SIMD): with two
        // waves per ray the first takes two axes and 3/8 of the levels, the second one axis, 5/8 of the levels and the clears
        const int ax0 = wpr == 2u ? (part == 0u ? 0 : 2) : 0, ax1 = wpr == 2u ? (part == 0u ? 2 : 3) : 3;
        if (part == 0u) {
          rl.z[lane] = zv;
          a.z[p] = zv;
          a.x3[(size_t)p * 3 + 0] = x[0];
          a.x3[(size_t)p * 3 + 1] = x[1];
          a.x3[(size_t)p * 3 + 2] = x[2];
        }
        // (OneBlob, like the grid levels below, is dev_encode.hpp's: the encoder kernels' arithmetic, never contracted)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
          if (ax >= ax0 && ax < ax1) oneblob_axis_fwd(x[ax], a.n_bins, rowp + ax * a.n_bins);
        if (part + 1u == wpr) {
          // the rows' grid columns of d_buf are only ever ADDED to (by the coarse network's backward): cleared here
          float* dg = a.d_buf + (size_t)p * ld + pe;
          for (uint32_t c = 0; c < 2u * L; c += 4) *reinterpret_cast<float4*>(dg + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (a.n_phases == 12u) return;                // (tools: behind OneBlob)
        const uint32_t l0 = wpr == 2u ? (part == 0u ? 0u : (3u * L) / 8u) : L * part / wpr;
        const uint32_t l1 = wpr == 2u ? (part == 0u ? (3u * L) / 8u : L) : L * (part + 1u) / wpr;
#pragma unroll 4
        for (uint32_t l = l0; l < l1; ++l) grid_level<true, true>(a.table, a.lv, l, x, rowp + pe, a.dydx, P, p);
        if (a.n_phases == 13u) return;                // (tools: behind the grid levels)
      }
    }
  }
  __syncthreads();
  {
    // tile -> buf rows [p0, p0 + npts): contiguous in memory
    const uint32_t nq = ld / 4u;
    float* out = a.buf + (size_t)p0 * ld;
    for (uint32_t i = threadIdx.x; i < npts * nq; i += blockDim.x) {
      const uint32_t r = i / nq, c = i - r * nq;
      const lds_fp t = tile + r * (ld + 1u) + 4u * c;
      *reinterpret_cast<float4*>(out + (size_t)r * ld + 4u * c) = make_float4(t[0], t[1], t[2], t[3]);
    }
  }
  __syncthreads();

  if (a.n_phases == 1u) return;
  // ---- 2: coarse network forward ------------------------------------------------------------------------------------------
  sp::FwdArgs fa = {};
  fa.ldx = ld;
  fa.n_slots = npts;
  fa.tiles_per_block = 1;
  fa.err = a.err;
  {
    fa.x = a.buf + (size_t)p0 * ld;
    fa.seg = {nullptr, 0u, ld};
    fa.n_in = ld; fa.n_in_w = ld; fa.n_out = hid + 1u;
    fa.y = a.lat + (size_t)p0 * (hid + 1u); fa.ldy = hid + 1u;
    fa.prep = a.w_coarse;
    __builtin_assume(fa.prep != nullptr);
    sp::mlp_fwd_body<NN, NL, 3>(fa, 0u, lds);
  }
  __syncthreads();

  if (a.n_phases == 2u) return;
#ifdef DNS_TF_STEM
  // ---- 3a: the (point, view) rows of the 2-D branch: code | OneBlob of the normalised relative point -------------------------
  float* __restrict__ slice = sa.ws + (size_t)wg * sa.slice_floats;
  float* __restrict__ mrows = slice + sa.rows;
  float* __restrict__ mlat = slice + sa.lat;
  float* __restrict__ mdy = slice + sa.dy;
  float* __restrict__ mdpe = slice + sa.dpe;
  float* __restrict__ mxm = slice + sa.xm;
  float* __restrict__ mdrel = slice + sa.drel;
  const uint32_t pe_m = 3u * sa.n_bins, ldm = pe_m + sa.Cs, R = sa.R, nrows = R * npts;
  // the point of row i's sample (phase 1's expression) and whether its code is kept (truncation mask != 0)
  auto row_point = [&](uint32_t pl, float (&pt)[3]) __attribute__((always_inline)) -> bool {
    DNS_TF_FP
    const uint32_t rr = pl / S;
    const RayLds rl = ray_lds(keep, rr);
    const float zv = rl.z[pl - rr * S], gd = rl.m[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] = DNS_FADD(rl.m[k], DNS_FMUL(rl.m[3 + k], zv));
    return !(zv < gd * 0.95f) && !(zv > gd * 1.05f) && gd > 0.f;
  };
  {
    Mat3 Km;
#pragma unroll
    for (int k = 0; k < 9; ++k) Km.k[k] = sa.K[k];
    const uint32_t sub = threadIdx.x & 15u;
    const size_t map_floats = (size_t)sa.h * sa.w * sa.Cs;
    // codes: 16 lanes per pair, 16 pairs per pass of the workgroup (frame_codes.hip phase A)
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < nrows; i0 += 16u) {
      const uint32_t i = i0 + (threadIdx.x >> 4);
      if (i < nrows) {
        const uint32_t r = i / npts, pl = i - r * npts;
        float pt[3], m[12];
        const bool kept = row_point(pl, pt);
        const lds_fp v = views + r * tfs::VIEW_FLOATS;
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = v[k];
        pair_code(m, Km, sa.maps + (size_t)r * map_floats, sa.Cs, sa.h, sa.w, a.H, a.W, pt[0], pt[1], pt[2], kept, sub,
                  mrows + (size_t)i * ldm + pe_m);
      }
    }
    // OneBlob: one row per thread into the LDS tile, then out as contiguous float4 runs
    for (uint32_t i0 = 0; i0 < nrows; i0 += tfs::PE_ROWS) {
      const uint32_t i = i0 + threadIdx.x;
      if (i < nrows) {
        const uint32_t r = i / npts, pl = i - r * npts;
        float pt[3], x[3];
        row_point(pl, pt);
        const lds_fp v = views + r * tfs::VIEW_FLOATS;
        const float og[3] = {v[12], v[13], v[14]};
        pair_rel(pt, og, sa.b0, sa.b1, x);
        mxm[(size_t)i * 3 + 0] = x[0];
        mxm[(size_t)i * 3 + 1] = x[1];
        mxm[(size_t)i * 3 + 2] = x[2];
        lds_fp rowp = tile + threadIdx.x * (pe_m + 1u);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) oneblob_axis_fwd(x[ax], sa.n_bins, rowp + ax * sa.n_bins);
      }
      __syncthreads();
      const uint32_t nq = pe_m / 4u, cnt = min(tfs::PE_ROWS, nrows - i0);
      for (uint32_t j = threadIdx.x; j < cnt * nq; j += blockDim.x) {
        const uint32_t rr = j / nq, c = j - rr * nq;
        const lds_fp s = tile + rr * (pe_m + 1u) + 4u * c;
        *reinterpret_cast<float4*>(mrows + (size_t)(i0 + rr) * ldm + 4u * c) = make_float4(s[0], s[1], s[2], s[3]);
      }
      __syncthreads();
    }
  }
  if (a.n_phases == 31u) return;
  // ---- 3b: Merge forward on the rows ------------------------------------------------------------------------------------------
  {
    sp::FwdArgs fm = {};
    fm.x = mrows; fm.ldx = ldm;
    fm.seg = {nullptr, 0u, ldm};
    fm.n_in = ldm; fm.n_in_w = ldm; fm.n_out = hid;
    fm.y = mlat; fm.ldy = hid;
    fm.n_slots = nrows; fm.tiles_per_block = R;
    fm.err = a.err;
    fm.prep = sa.w_merge;
    __builtin_assume(fm.prep != nullptr);
    sp::mlp_fwd_body<NN, NL, 3>(fm, 0u, lds);
  }
  __syncthreads();
  if (a.n_phases == 32u) return;
#endif
  // ---- 3: feature block [latent | code x truncation mask], raw[:, 3] = occupancy ---------------------------------------------
  // Without a 2-D code (nf == hid: the colour / logit images are those of the LIVE network, DNS_MLP_LIVE_IN(pe + hid)) there is
  // no block to build: the two networks read the latent straight out of the coarse network's output rows (second input
  // segment = lat + 1, row stride hid + 1: 16-byte loads from 4-byte aligned addresses -- the memory pipeline runs in
  // unaligned-access mode under the HSA ABI) and phase 5 copies the occupancy column itself.
  const bool direct = a.code == nullptr && nf == hid;
  if (!direct) {
    const uint32_t qn = nf / 4u, qh = hid / 4u;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < npts * qn; i += blockDim.x) {
      const uint32_t pl = i / qn, q = i - pl * qn, p = p0 + pl;
      const float* f = a.lat + (size_t)p * (hid + 1u);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < qh) {
        v = make_float4(f[1 + 4 * q], f[2 + 4 * q], f[3 + 4 * q], f[4 + 4 * q]);
        if (q == 0u) a.raw[(size_t)p * 4 + 3] = f[0];
#ifdef DNS_TF_STEM
      } else if (4u * (q - qh) < hid) {
        // 3c: the code = Merge's latents summed over the views in ascending view order, x 1 / R, x truncation mask
        const uint32_t rr = pl / S;
        const RayLds rl = ray_lds(keep, rr);
        const float d = rl.m[12], zz = rl.z[pl - rr * S];
        const float front = zz < d * 0.95f ? 1.f : 0.f, back = zz > d * 1.05f ? 1.f : 0.f, pos = d > 0.f ? 1.f : 0.f;
        const float t = (1.f - front) * (1.f - back) * pos;
        const float inv_ref = R > 1u ? 1.0f / (float)R : 1.0f;
        const float* c0 = mlat + (size_t)pl * hid + 4u * (q - qh);
        float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t r = 0; r < R; ++r) {
          const float4 u = *reinterpret_cast<const float4*>(c0 + (size_t)r * npts * hid);
          cv.x += u.x; cv.y += u.y; cv.z += u.z; cv.w += u.w;
        }
        if (R > 1u) { cv.x *= inv_ref; cv.y *= inv_ref; cv.z *= inv_ref; cv.w *= inv_ref; }
        v = make_float4(cv.x * t, cv.y * t, cv.z * t, cv.w * t);
#endif
      } else if (a.code && 4u * (q - qh) < a.code_dim) {
        const uint32_t rr = pl / S;
        const RayLds rl = ray_lds(keep, rr);
        const float d = rl.m[12], zz = rl.z[pl - rr * S];
        const float front = zz < d * 0.95f ? 1.f : 0.f, back = zz > d * 1.05f ? 1.f : 0.f, pos = d > 0.f ? 1.f : 0.f;
        const float t = (1.f - front) * (1.f - back) * pos;
        const float4 cv = *reinterpret_cast<const float4*>(a.code + (size_t)p * a.code_dim + 4u * (q - qh));
        v = make_float4(cv.x * t, cv.y * t, cv.z * t, cv.w * t);
      }
      *reinterpret_cast<float4*>(a.feat + (size_t)p * nf + 4u * q) = v;
    }
  }
  __syncthreads();

  if (a.n_phases == 3u) return;
  // ---- 4: colour and logit networks forward ---------------------------------------------------------------------------------
  {
    fa.x = a.buf + (size_t)p0 * ld;
    fa.seg = {direct ? a.lat + (size_t)p0 * (hid + 1u) + 1 : a.feat + (size_t)p0 * nf, direct ? hid + 1u : nf, pe};
    fa.n_in = pe + nf; fa.n_in_w = pe + nf; fa.n_out = 3u;
    fa.y = a.raw + (size_t)p0 * 4; fa.ldy = 4u;
    fa.prep = a.w_color;
    __builtin_assume(fa.prep != nullptr);
    sp::mlp_fwd_body<NN, NL, 3>(fa, 0u, lds);
    fa.n_out = C;
    fa.y = a.logit + (size_t)p0 * C; fa.ldy = C;
    fa.prep = a.w_logit;
    __builtin_assume(fa.prep != nullptr);
    sp::mlp_fwd_body<NN, NL, 3>(fa, 0u, lds);
  }
  __syncthreads();

  if (a.n_phases == 4u) return;
  // ---- 5: compositing, ray losses, their gradients, compositing backward (one wave per ray) -------------------------------
  if (wave < n1 - n0) {
    const uint32_t r = wave, n = n0 + r;
    RayLds rl = ray_lds(keep, r);
    if (direct && lane < S) a.raw[((size_t)n * S + lane) * 4 + 3] = a.lat[((size_t)n * S + lane) * (hid + 1u)];   // occupancy
    RayState<1> st;
    ray_forward<1>(a.raw, a.z, n, S, lane, st);
    const uint32_t s = lane;
    const bool ok = s < S;
    float col[3] = {0.f, 0.f, 0.f};
    if (ok) {
      const float* rw = a.raw + ((size_t)n * S + s) * 4;
      col[0] = sigmoid1c(rw[0]); col[1] = sigmoid1c(rw[1]); col[2] = sigmoid1c(rw[2]);   // models/decoder.py:124
    }
    const float t = st.z[0] - st.depth;
    const float var = wave_sum(st.w[0] * t * t);
    float rgb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[k] = wave_sum(ok ? st.w[0] * col[k] : 0.f);
    rl.w[lane] = st.w[0];
    // sem[c] = sum_s w_s logit[s, c] -- class c in lane c.  Few classes: every lane takes ITS sample's row (C loads in flight
    // per lane) and the classes are reduced across the wave; many: lanes over classes, walking the samples
    float sem = 0.f;
    float lrow[16];
    if (C <= 16u) {
#pragma unroll
      for (uint32_t c = 0; c < 16u; ++c) lrow[c] = (c < C && ok) ? a.logit[((size_t)n * S + s) * C + c] : 0.f;
#pragma unroll
      for (uint32_t c = 0; c < 16u; ++c) {
        if (c < C) {                               // uniform
          const float t2 = wave_sum(st.w[0] * lrow[c]);
          sem = lane == c ? t2 : sem;
        }
      }
    } else if (lane < C) {
      const float* lp = a.logit + (size_t)n * S * C + lane;
      for (uint32_t ss = 0; ss < S; ++ss) sem += rl.w[ss] * lp[(size_t)ss * C];
    }
    // the three masked terms with n_valid = 1 (the pose kernel divides by the count) and their gradients
    const bool valid = rl.m[13] != 0.f;
    const float gd = rl.m[12];
    float spv = 0.f, gc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float e = rl.m[9 + k] - rgb[k];
      spv += e * e;
      gc[k] = valid ? -(a.lambda_p * 2.f / 3.f) * e : 0.f;
    }
    const float e = gd - st.depth;
    const float sv = sqrtf(var + 1e-10f);
    const float sdv = fabsf(e) / sv;
    const float sg = e > 0.f ? -1.f : (e < 0.f ? 1.f : 0.f);
    const float gD = valid ? a.lambda_d * sg / sv : 0.f;
    const float gV = valid ? a.lambda_d * fabsf(e) * (-0.5f) / (sv * sv * sv) : 0.f;
    float slv = 0.f, dsem = 0.f;
    if (C) {
      float mx = lane < C ? sem : -INFINITY;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      const float ex = lane < C ? expf(sem - mx) : 0.f;
      const float se = wave_sum(ex);
      const int lab = __float_as_int(rl.m[14]);
      const float ll = wave_sum((lab >= 0 && (uint32_t)lab == lane && lane < C) ? sem : 0.f);
      slv = (mx + logf(se)) - ll;
      dsem = (valid && lane < C) ? a.lambda_l * (ex / se - ((int)lane == lab ? 1.f : 0.f)) : 0.f;
    }
    rl.dsem[lane] = dsem;
    if (lane == 0u) {
      rl.loss[0] = valid ? spv : 0.f;
      rl.loss[1] = valid ? sdv : 0.f;
      rl.loss[2] = valid ? slv : 0.f;
      rl.loss[3] = valid ? 1.f : 0.f;
    }
    // compositing backward (composite_bwd_kernel<1> with the colour sigmoid folded in)
    float g = 0.f;
    if (ok) {
      g = gc[0] * col[0] + gc[1] * col[1] + gc[2] * col[2] + gD * st.z[0] + gV * t * t;
      if (C) {
        float dot = 0.f;
        if (C <= 16u) {
#pragma unroll
          for (uint32_t c = 0; c < 16u; ++c) dot += c < C ? rl.dsem[c] * lrow[c] : 0.f;
        } else {
          const float* lp = a.logit + ((size_t)n * S + s) * C;
          for (uint32_t c = 0; c < C; ++c) dot += rl.dsem[c] * lp[c];
        }
        g += dot;
      }
    }
    const float gbar = wave_sum(st.w[0] * g);
    const float du = (g - gbar) / st.sumu;
    const float after = wave_suffix_excl_sum(du * st.u[0], lane);
    const float dalpha = du * st.T[0] - after / st.om[0];
    if (ok) {
      const size_t p = (size_t)n * S + s;
      float4 o4;
      o4.x = st.w[0] * gc[0] * (1.f - col[0]) * col[0];
      o4.y = st.w[0] * gc[1] * (1.f - col[1]) * col[1];
      o4.z = st.w[0] * gc[2] * (1.f - col[2]) * col[2];
      o4.w = 0.f;
      *reinterpret_cast<float4*>(a.d_col + p * 4) = o4;
      a.d_featx[p * ldf + 3] = 10.0f * st.alpha[0] * (1.0f - st.alpha[0]) * dalpha;
    }
    if (C && C <= 16u) {
      if (ok) {
        float* lp = a.d_logit + ((size_t)n * S + s) * C;
#pragma unroll
        for (uint32_t c = 0; c < 16u; ++c)
          if (c < C) lp[c] = st.w[0] * rl.dsem[c];
      }
    } else if (C) {
      for (uint32_t c = lane; c < C; c += 64) {
        const float gs = rl.dsem[c];
        float* lp = a.d_logit + (size_t)n * S * C + c;
        for (uint32_t ss = 0; ss < S; ++ss) lp[(size_t)ss * C] = rl.w[ss] * gs;
      }
    }
  }
  __syncthreads();

  if (a.n_phases == 5u) return;
  // ---- 6: the three networks' backward (input gradients only: the scene is frozen) ---------------------------------------------
  {
    sp::BwdArgs ba = {};
    ba.x = a.buf + (size_t)p0 * ld; ba.ldx = ld;
    ba.n_slots = npts; ba.tiles_per_block = 1; ba.n_waves = 4; ba.err = a.err;
    ba.dx = a.d_buf + (size_t)p0 * ld; ba.lddx = ld;
    // colour: overwrites d_buf[:, 0:pe] and the feature block's gradient
    ba.seg = {direct ? a.lat + (size_t)p0 * (hid + 1u) + 1 : a.feat + (size_t)p0 * nf, direct ? hid + 1u : nf, pe};
    ba.dy = a.d_col + (size_t)p0 * 4; ba.lddy = 4u;
    ba.n_in = pe + nf; ba.n_in_w = pe + nf; ba.n_out = 3u;
    ba.dseg = {a.d_featx + (size_t)p0 * ldf + 4, ldf, 0u, 0u, 0u};
    ba.prep = a.w_color + a.fwdb_color;
    __builtin_assume(ba.prep != nullptr);
    sp::mlp_bwd_body<NCHO, 1, 3, false, false, false, 4>(ba, 0u, lds);
    // logit: adds to both
    ba.dy = a.d_logit + (size_t)p0 * C; ba.lddy = C; ba.n_out = C;
    ba.dseg.acc1 = 1u; ba.dseg.acc2 = 1u;
    ba.prep = a.w_logit + a.fwdb_logit;
    __builtin_assume(ba.prep != nullptr);
    sp::mlp_bwd_body<NCHO, MTL, 3, false, false, false, 4>(ba, 0u, lds);
#ifdef DNS_TF_STEM
    // ---- 6a: Merge backward: d code -> the rows' d latent -> d OneBlob -> d(relative point) ------------------------------------
    __syncthreads();
    {
      // d_lat(r, p) = d_code(p) trunc(p) / R for every view (merge_dy_kernel's expression)
      const uint32_t qh = hid / 4u;
      const float inv = 1.0f / (float)R;
      for (uint32_t i = threadIdx.x; i < npts * qh; i += blockDim.x) {
        const uint32_t pl = i / qh, q = i - pl * qh, rr = pl / S;
        const RayLds rl = ray_lds(keep, rr);
        const float d = rl.m[12], zz = rl.z[pl - rr * S];
        const float front = zz < d * 0.95f ? 1.f : 0.f, back = zz > d * 1.05f ? 1.f : 0.f, pos = d > 0.f ? 1.f : 0.f;
        const float t = (1.f - front) * (1.f - back) * pos * inv;
        float4 g = *reinterpret_cast<const float4*>(a.d_featx + (size_t)(p0 + pl) * ldf + 4u + hid + 4u * q);
        g.x *= t; g.y *= t; g.z *= t; g.w *= t;
        float* dst = mdy + (size_t)pl * hid + 4u * q;
        for (uint32_t r = 0; r < R; ++r) *reinterpret_cast<float4*>(dst + (size_t)r * npts * hid) = g;
      }
    }
    __syncthreads();
    {
      // input gradient only, first segment only: the two-segment input with no second gradient segment (DNS_MLP_DX_FIRST's form);
      // the hidden activations are recomputed from the rows of 3a
      sp::BwdArgs bm = {};
      bm.x = mrows; bm.ldx = ldm;
      bm.seg = {mrows + pe_m, ldm, pe_m};
      bm.dy = mdy; bm.lddy = hid;
      bm.n_in = ldm; bm.n_in_w = ldm; bm.n_out = hid;
      bm.dx = mdpe; bm.lddx = pe_m;
      bm.dseg = {nullptr, 0u, 0u, 0u, 0u};
      bm.n_slots = nrows; bm.tiles_per_block = R; bm.n_waves = 4; bm.err = a.err;
      bm.prep = sa.w_merge + sa.fwdb_merge;
      __builtin_assume(bm.prep != nullptr);
      sp::mlp_bwd_body<NCHM, 1, 3, false, false, false, 4>(bm, 0u, lds);
    }
    __syncthreads();
    // OneBlob backward: the rows' d OneBlob -> tile (coalesced), one row per thread, d rel = d x / (b1 - b0) in fp64
    for (uint32_t i0 = 0; i0 < nrows; i0 += tfs::PE_ROWS) {
      const uint32_t nq = pe_m / 4u, cnt = min(tfs::PE_ROWS, nrows - i0);
      for (uint32_t j = threadIdx.x; j < cnt * nq; j += blockDim.x) {
        const uint32_t rr = j / nq, c = j - rr * nq;
        const float4 v = *reinterpret_cast<const float4*>(mdpe + (size_t)(i0 + rr) * pe_m + 4u * c);
        const lds_fp t = tile + rr * (pe_m + 1u) + 4u * c;
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
      }
      __syncthreads();
      const uint32_t i = i0 + threadIdx.x;
      if (i < nrows) {
        const lds_fp g = tile + threadIdx.x * (pe_m + 1u);
        const float x[3] = {mxm[(size_t)i * 3], mxm[(size_t)i * 3 + 1], mxm[(size_t)i * 3 + 2]};
        float dxm[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) oneblob_axis_bwd(x[ax], sa.n_bins, g + ax * sa.n_bins, dxm[ax]);
#pragma unroll
        for (int k = 0; k < 3; ++k) mdrel[(size_t)i * 3 + k] = (float)((double)dxm[k] / (sa.b1[k] - sa.b0[k]));
      }
      __syncthreads();
    }
    if (a.n_phases == 61u) return;
#endif
    // coarse: dY = [d occupancy | d latent] = d_featx[:, 3 : 4 + hid]; adds to all ld columns of d_buf
    ba.seg = {nullptr, 0u, ld};
    ba.dy = a.d_featx + (size_t)p0 * ldf + 3; ba.lddy = ldf; ba.n_out = hid + 1u;
    ba.n_in = ld; ba.n_in_w = ld;
    ba.dseg = {nullptr, 0u, 1u, 0u, 0u};
    ba.prep = a.w_coarse + a.fwdb_coarse;
    __builtin_assume(ba.prep != nullptr);
    sp::mlp_bwd_body<NCHC, MTC, 3, false, false, false, 4>(ba, 0u, lds);
  }
  __syncthreads();

  if (a.n_phases == 6u) return;
  // ---- 7: encoding backward -> d pts, the rays' sums for the pose -------------------------------------------------------------
  {
    DNS_TF_FP                                  // (stem form: the grid's dot products round as encode_bwd_kernel's, compiled without contraction)
    {
      // the workgroup's d_buf rows (contiguous) -> tile, coalesced; the lanes then read THEIR row from LDS
      const uint32_t nq = ld / 4u;
      const float* src = a.d_buf + (size_t)p0 * ld;
      for (uint32_t i = threadIdx.x; i < npts * nq; i += blockDim.x) {
        const uint32_t r = i / nq, c = i - r * nq;
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * ld + 4u * c);
        const lds_fp t = tile + r * (ld + 1u) + 4u * c;
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
      }
    }
    __syncthreads();
    const uint32_t r = wave / wpr, part = wave - r * wpr, n = n0 + r;
    float dx[3] = {0.f, 0.f, 0.f};
    if (n < n1 && lane < S) {
      const uint32_t p = n * S + lane;
      const lds_fp g = tile + (p - p0) * (ld + 1u);
      if (part == 0u) {
        const float x[3] = {a.x3[(size_t)p * 3], a.x3[(size_t)p * 3 + 1], a.x3[(size_t)p * 3 + 2]};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) oneblob_axis_bwd(x[ax], a.n_bins, g + ax * a.n_bins, dx[ax]);
      }
      const uint32_t l0 = L * part / wpr, l1 = L * (part + 1u) / wpr;        // (any split: the parts' sums are added)
#pragma unroll 4
      for (uint32_t l = l0; l < l1; ++l) {
        const float g0 = g[pe + 2 * l], g1 = g[pe + 2 * l + 1];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float2 j = a.dydx[((size_t)l * 3 + k) * P + p];
          dx[k] += j.x * g0 + j.y * g1;
        }
      }
    }
    lds_fp mine = dxp + (wave * 64u + lane) * 3u;
    mine[0] = dx[0]; mine[1] = dx[1]; mine[2] = dx[2];
    __syncthreads();
    if (part == 0u && n < n1) {
      RayLds rl = ray_lds(keep, r);
      float go[3] = {0.f, 0.f, 0.f}, gdv[3] = {0.f, 0.f, 0.f};
      if (lane < S) {
        const float zv = rl.z[lane];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float v = 0.f;
          for (uint32_t q = 0; q < wpr; ++q) v += dxp[((wave + q) * 64u + lane) * 3u + k];
          v = (float)((double)v / (a.b6.b1[k] - a.b6.b0[k]));       // d pts = d x / (b1 - b0) (fp64, encode_bwd_kernel)
#ifdef DNS_TF_STEM
          {
            // + Merge's share: the views' d rel in ascending view order (add_ref_sum_kernel)
            const float* src = mdrel + (size_t)((n - n0) * S + lane) * 3u + k;
            float s = 0.f;
            for (uint32_t q = 0; q < R; ++q) s += src[(size_t)q * npts * 3u];
            v += s;
          }
#endif
          go[k] = v;
          gdv[k] = v * zv;
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        go[k] = wave_sum(go[k]);
        gdv[k] = wave_sum(gdv[k]);
      }
      if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
          for (int b = 0; b < 3; ++b) rl.pose[3 * k + b] = gdv[k] * rl.m[6 + b];   // dL/dR[k][b] = dL/dd[k] dir[b]
          rl.pose[9 + k] = go[k];
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 16u) {
      float v = 0.f;
      for (uint32_t rr = 0; rr < n1 - n0; ++rr) {
        const RayLds rl = ray_lds(keep, rr);
        v += threadIdx.x < 12u ? rl.pose[threadIdx.x] : rl.loss[threadIdx.x - 12u];
      }
      a.part[(size_t)wg * 16 + threadIdx.x] = v;
    }
  }
}

}  // namespace

// ---- pose kernel: the workgroups' sums -> loss, keep-best, quaternion chain rule, Adam (one workgroup) ----------------------
static __global__ __launch_bounds__(1024) void track_pose_kernel(PoseArgs a) {
  __shared__ float red[16][16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // fixed-order sums over the workgroups' rows: thread (group = t >> 4, e = t & 15) takes rows group, group + 64, ... -- at most a
  // handful per thread, all requested before the first add (a rolled loop of dependent loads was most of this kernel's 10 us)
  const uint32_t e = threadIdx.x & 15u, grp = threadIdx.x >> 4, ngrp = blockDim.x >> 4;
  float s = 0.f;
  for (uint32_t w0 = grp; w0 < a.n_wg; w0 += 4u * ngrp) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = w0 + (uint32_t)k * ngrp;
      v[k] = w < a.n_wg ? a.part[(size_t)w * 16 + e] : 0.f;
    }
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 32);
  if (lane < 16u) red[wave][lane] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  // every input of the serial part is requested here, in one batch (the chain below would otherwise pay a memory round trip
  // at each first use: quat, moments, step count, best loss)
  float q_in[4], t_in[3], m_in[8], v_in[8];
  for (int k = 0; k < 4; ++k) q_in[k] = a.quat[k];
  for (int k = 0; k < 3; ++k) t_in[k] = a.trans[k];
  for (int k = 0; k < 8; ++k) { m_in[k] = a.m[k]; v_in[k] = a.v[k]; }
  const float step_in = a.state[0], best_in = a.best_loss[0];
  const uint32_t iter_in = a.iter[0];
  float G[16];
  for (int k = 0; k < 16; ++k) {
    float t = 0.f;
    for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) t += red[w][k];
    G[k] = t;
  }
  const float nv = G[15];
  const float p = G[12] / (3.f * nv), d = G[13] / nv, l = G[14] / nv;          // 0/0 -> NaN like torch's mean of an empty selection
  const float loss = a.lambda_p * p + a.lambda_d * d + a.lambda_l * l;
  a.out[0] = p; a.out[1] = d; a.out[2] = l; a.out[3] = loss; a.out[4] = nv;
  // keep-best: the camera that PRODUCED the loss (slams/tracking.py:326-335); a NaN loss compares false
  if (loss < best_in) {
    a.best_loss[0] = loss;
    for (int i = 0; i < 4; ++i) a.best_cam[i] = q_in[i];
    for (int i = 0; i < 3; ++i) a.best_cam[4 + i] = t_in[i];
  }
  for (int k = 0; k < 12; ++k) G[k] /= nv;
  // quaternion chain rule (raygen_bwd_pose_kernel; utils/common.py:406-429)
  const float r = q_in[0], i = q_in[1], j = q_in[2], k = q_in[3];
  const float nrm = r * r + i * i + j * j + k * k;
  const float two_s = 2.0f / nrm;
  const float M[9] = {-(j * j + k * k), i * j - k * r, i * k + j * r, i * j + k * r, -(i * i + k * k),
                      j * k - i * r,    i * k - j * r, j * k + i * r, -(i * i + j * j)};
  float gm = 0.f;
  for (int q = 0; q < 9; ++q) gm += G[q] * M[q];
  const float dr = -k * G[1] + j * G[2] + k * G[3] - i * G[5] - j * G[6] + i * G[7];
  const float di = j * (G[1] + G[3]) + k * (G[2] + G[6]) - 2.f * i * (G[4] + G[8]) + r * (G[7] - G[5]);
  const float dj = -2.f * j * (G[0] + G[8]) + i * (G[1] + G[3]) + r * (G[2] - G[6]) + k * (G[5] + G[7]);
  const float dk = -2.f * k * (G[0] + G[4]) + r * (G[3] - G[1]) + i * (G[2] + G[6]) + j * (G[5] + G[7]);
  const float c = two_s * two_s * gm;
  const float gq[4] = {two_s * dr - c * r, two_s * di - c * i, two_s * dj - c * j, two_s * dk - c * k};
  const float gt[3] = {G[9], G[10], G[11]};
  for (int q = 0; q < 4; ++q) a.g_quat[q] = gq[q];
  for (int q = 0; q < 3; ++q) a.g_trans[q] = gt[q];
  // Adam (adam_tick_kernel + adam_step_kernel's arithmetic)
  const float t = step_in + 1.0f;
  const float bc1 = 1.0f - powf(a.beta1, t), bc2 = 1.0f - powf(a.beta2, t);
  a.state[0] = t; a.state[1] = bc1; a.state[2] = bc2;
  const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
  const float ob1 = 1.0f - a.beta1, ob2 = 1.0f - a.beta2;
  auto upd = [&](float* pp, const float* p_in, const float* gg, int off, int n, float lr) {
    const float step_size = lr / bc1;
    for (int q = 0; q < n; ++q) {
      const float mi = a.beta1 * m_in[off + q] + ob1 * gg[q];
      const float vi = a.beta2 * v_in[off + q] + ob2 * gg[q] * gg[q];
      a.m[off + q] = mi;
      a.v[off + q] = vi;
      const float denom = sqrtf(vi) * inv_sqrt_bc2 + a.eps;
      pp[q] = p_in[q] - step_size * (mi / denom);
    }
  };
  upd(a.trans, t_in, gt, 4, 3, a.lr_t);
  upd(a.quat, q_in, gq, 0, 4, a.lr_q);
  a.iter[0] = iter_in + 1u;
}

// ---- frame begin: for every iteration of the frame, the forced mid sample of its surface jitter (utils/common.py:572-574) and
// max(gt_depth) over its pixel draw (:581,591) -- neither depends on the pose.  grid = n_iters, one workgroup per iteration
static __global__ __launch_bounds__(256) void track_begin_kernel(const int64_t* __restrict__ pix, uint32_t N, uint32_t n_iters,
                                                          const float* __restrict__ depth, int W, int H0, int W0, int wwin,
                                                          float* __restrict__ t_surf, uint32_t ns, uint32_t half_idx,
                                                          uint32_t* __restrict__ dmax) {
  __shared__ float red[4];
  const uint32_t it = blockIdx.x;
  if (threadIdx.x < 64u) {
    float* t = t_surf + (size_t)it * ns;
    bool any = false;
    for (uint32_t i = threadIdx.x; i < ns; i += 64u) any = any || t[i] == 0.5f;
    if (!__any(any) && threadIdx.x == 0 && half_idx < ns) t[half_idx] = 0.5f;
  }
  float m = 0.f;
  for (uint32_t n = threadIdx.x; n < N; n += blockDim.x) {
    const int64_t q = pix[(size_t)it * N + n];
    const int row = H0 + (int)(q / wwin), col = W0 + (int)(q % wwin);
    const float d = depth[(size_t)row * W + col];
    m = fmaxf(m, d > 0.f ? d : 0.f);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) dmax[it] = __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}


#ifdef DNS_TF_STEM
template <int MTL, int NCHO>
static bool tf_attr() {
  return hipFuncSetAttribute((const void*)track_fused_kernel<MTL, NCHO, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess &&
         hipFuncSetAttribute((const void*)track_fused_kernel<MTL, NCHO, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess;
}
#else
template <int MTL, int NCHO>
static bool tf_attr() {
  return hipFuncSetAttribute((const void*)track_fused_kernel<MTL, NCHO>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess;
}
#endif
static int tf_init_attrs() {
  if (!tf_attr<1, 3>() || !tf_attr<2, 3>() || !tf_attr<1, 4>() || !tf_attr<2, 4>()) {
    set_error("dns_init: hipFuncSetAttribute failed for the fused tracker kernel");
    return DNS_E_LAUNCH;
  }
  return DNS_OK;
}
static AttrRegistrar tf_attr_registrar(tf_init_attrs);

#define DNS_TF_CAT(a, b, c) a##b##_##c
#define DNS_TF_NAME(pfx, nn, nl) DNS_TF_CAT(pfx, nn, nl)
#ifdef DNS_TF_STEM
// LDS bytes of the network phases of the stem form: the largest of the four networks' needs (Merge: n_in_merge -> hid, forward and
// input-gradient backward), 0 = unsupported shape
uint32_t DNS_TF_NAME(track_fused_stem_mlp_lds_, DNS_BWD_NN, DNS_BWD_NL)(uint32_t n_in_out, uint32_t mtl, uint32_t n_in_merge, uint32_t hid) {
  using namespace sp;
  if (n_in_out <= 64u || n_in_out > 128u || mtl < 1u || mtl > 2u || n_in_merge <= 64u || n_in_merge > 128u || hid < 1u || hid > 32u) return 0u;
  uint32_t m = FwdLds<NN, NL>::total(n_in_out, mtl * 32u, 4);
  const uint32_t b1 = n_in_out <= 96u ? (mtl == 1u ? BwdLds<3, 1>::total(true, 4) : BwdLds<3, 2>::total(true, 4))
                                      : (mtl == 1u ? BwdLds<4, 1>::total(true, 4) : BwdLds<4, 2>::total(true, 4));
  const uint32_t b2 = BwdLds<3, 2>::total(true, 4);
  const uint32_t f3 = FwdLds<NN, NL>::total(n_in_merge, hid, 4);
  const uint32_t b3 = n_in_merge <= 96u ? BwdLds<3, 1>::total(true, 4) : BwdLds<4, 1>::total(true, 4);
  m = m > b1 ? m : b1;
  m = m > b2 ? m : b2;
  m = m > f3 ? m : f3;
  m = m > b3 ? m : b3;
  return (m + 15u) & ~15u;
}
int DNS_TF_NAME(launch_track_fused_stem_, DNS_BWD_NN, DNS_BWD_NL)(const TrackArgs& a, const StemArgs& s, const PoseArgs& p, uint32_t n_wg, uint32_t mtl,
                                                                  hipStream_t st) {
  const size_t lds_bytes = (size_t)s.views_off + tfs::VIEWS_BYTES;
  const bool narrow = 3u * a.n_bins + a.nf <= 96u;             // colour / logit input width: three or four 32-column chunks
  const bool narrow_m = 3u * s.n_bins + s.Cs <= 96u;           // Merge's
#define DNS_TF_GO(MTL_, NCHO_)                                                                                              \
  {                                                                                                                         \
    if (narrow_m) DNS_LAUNCH((track_fused_kernel<MTL_, NCHO_, 3>), dim3(n_wg), dim3(256), lds_bytes, st, a, s);            \
    else DNS_LAUNCH((track_fused_kernel<MTL_, NCHO_, 4>), dim3(n_wg), dim3(256), lds_bytes, st, a, s);                     \
  }
  if (narrow) {
    if (mtl == 1u) DNS_TF_GO(1, 3)
    else DNS_TF_GO(2, 3)
  } else {
    if (mtl == 1u) DNS_TF_GO(1, 4)
    else DNS_TF_GO(2, 4)
  }
#undef DNS_TF_GO
  DNS_LAUNCH(track_pose_kernel, dim3(1), dim3(1024), 0, st, p);
  return check_launch("dns_track_fused_iter");
}
#else
uint32_t DNS_TF_NAME(track_fused_mlp_lds_, DNS_BWD_NN, DNS_BWD_NL)(uint32_t n_in_out, uint32_t mtl) {
  using namespace sp;
  if (n_in_out <= 64u || n_in_out > 128u || mtl < 1u || mtl > 2u) return 0u;
  uint32_t m = FwdLds<NN, NL>::total(n_in_out, mtl * 32u, 4);
  const uint32_t b1 = n_in_out <= 96u ? (mtl == 1u ? BwdLds<3, 1>::total(true, 4) : BwdLds<3, 2>::total(true, 4))
                                      : (mtl == 1u ? BwdLds<4, 1>::total(true, 4) : BwdLds<4, 2>::total(true, 4));
  const uint32_t b2 = BwdLds<3, 2>::total(true, 4);
  m = m > b1 ? m : b1;
  m = m > b2 ? m : b2;
  return (m + 15u) & ~15u;
}
int DNS_TF_NAME(launch_track_fused_, DNS_BWD_NN, DNS_BWD_NL)(const TrackArgs& a, const PoseArgs& p, uint32_t n_wg, uint32_t mtl, hipStream_t st) {
  const size_t lds_bytes = (size_t)a.keep_off + TF_KEEP_BYTES;
  const bool narrow = 3u * a.n_bins + a.nf <= 96u;             // colour / logit input width: three or four 32-column chunks
  if (narrow) {
    if (mtl == 1u) DNS_LAUNCH((track_fused_kernel<1, 3>), dim3(n_wg), dim3(256), lds_bytes, st, a);
    else DNS_LAUNCH((track_fused_kernel<2, 3>), dim3(n_wg), dim3(256), lds_bytes, st, a);
  } else {
    if (mtl == 1u) DNS_LAUNCH((track_fused_kernel<1, 4>), dim3(n_wg), dim3(256), lds_bytes, st, a);
    else DNS_LAUNCH((track_fused_kernel<2, 4>), dim3(n_wg), dim3(256), lds_bytes, st, a);
  }
  DNS_LAUNCH(track_pose_kernel, dim3(1), dim3(1024), 0, st, p);
  return check_launch("dns_track_fused_iter");
}
#endif  // DNS_TF_STEM
#ifdef DNS_TF_WITH_BEGIN
int launch_track_begin(const int64_t* pix, uint32_t N, uint32_t n_iters, const float* depth, int W, int H0, int W0, int wwin,
                       float* t_surf, uint32_t ns, uint32_t half_idx, uint32_t* dmax, hipStream_t st) {
  DNS_LAUNCH(track_begin_kernel, dim3(n_iters), dim3(256), 0, st, pix, N, n_iters, depth, W, H0, W0, wwin, t_surf, ns, half_idx, dmax);
  return check_launch("dns_track_fused_begin");
}
#endif

#undef NN
#undef NL

}  // namespace tf
}  // namespace dns
