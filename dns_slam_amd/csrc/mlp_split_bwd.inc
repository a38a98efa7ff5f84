// Backward kernel of the split-operand MLP for ONE (n_neurons, n_hidden_layers) pair: included by mlp_split_bwd_*.hip with
// DNS_BWD_NN / DNS_BWD_NL defined (one translation unit each, so the instantiations compile in parallel).
//
// One kernel per network produces the input gradient, dW_hidden and dW_out and leaves dH_1 (256 B per point) for the
// streaming kernel that forms dW_in = dH_1^T X (mlp_split.hip); hidden activations are recomputed (two layers of f16
// matrix instructions cost less than reading 512 B per point back from HBM).  Keeping dW_in here as well was tried: its
// 96-128 accumulator registers on top of dW_hidden / dW_out and the tile's working set do not fit a wave's registers.
//
// Per 32-point tile of a wave (1 wave per SIMD, 4 per workgroup, one workgroup per CU -- the weight images in both
// orientations take ~100 KB of LDS):
//   A  X -> H1 -> H2                       forward images (W_in NAT, W_h CHAIN)
//   B  dH_last = W_out^T dY (.) relu'      A = W_out^T (rows = hidden units, K = outputs, NAT)
//   C  dW_out += dY^T-form x H_last^T-form (K axis = the tile's 32 points)
//   D  dH_1 = W_h^T dH_2 (.) relu',  dW_h += dH_2 x H_1
//   E  dH_1 -> workspace [slot][n_neurons];  dX = W_in^T dH_1, stored row-coalesced, optionally added in place / in two
//      segments
// A product that sums over the POINT axis needs both operands with the point index on the K elements, i.e. transposed
// with respect to the accumulator layout (lane = point): accumulator tiles go through a wave-private 32 x 36-float LDS
// tile (16 ds_write_b32, 4 ds_read_b128), dY is re-read column-wise from L1.
//
// Register discipline (what made this kernel fit: hipcc's first attempt spilled 870 registers):
//   * NCH (32-column input chunks) and MT (32-row output tiles) are template parameters: K-steps past n_in / n_out run on
//     zero columns instead of sitting behind `if (k < n)` -- a uniform branch around an accumulation makes the compiler
//     copy the accumulator tiles at every merge point;
//   * the persistent dW accumulators are zeroed at ONE place (the start of a run of tiles of one weight set), then only ever
//     written by matrix instructions, and flushed at one place (the end of the run): any conditional reset or rescaling in
//     the tile loop costs a second copy of every accumulator.  Their products (K axis = points) use the scale-free
//     three-part bf16 format of mlp_split.hpp for the same reason.
#include <type_traits>
#include "mlp_split.hpp"

namespace dns {
namespace sp {

#define NN DNS_BWD_NN
#define NL DNS_BWD_NL
// Waves per workgroup: template parameter NW of the kernel.  4 with weight gradients (one wave per SIMD: 192-256 registers of
// persistent accumulators); 8 -- TWO per SIMD on one set of weight images -- for the frozen-scene form (no accumulators), where
// hiding each other's LDS / memory latency is worth 1.28-1.37x (round 4, tools/time_mlp_nodw.py: 96.5 -> 75.4 us at
// 80 -> 64 x 2 -> 33, bit-identical dX).

namespace {

template <int NCH, int MT>
struct BwdLds {
  static constexpr uint32_t NT = NN / 32;
  static constexpr uint32_t img_in = 0;                                          // [NT][2 NCH] fragments pairs of 2 KB
  static constexpr uint32_t img_h = img_in + NT * 2 * NCH * 2048u;
  static constexpr uint32_t img_outT = img_h + (NL - 1) * NT * (NN / 16) * 2048u;  // [NT][2 MT]
  static constexpr uint32_t img_hT = img_outT + NT * 2 * MT * 2048u;
  static constexpr uint32_t img_inT = img_hT + (NL - 1) * NT * (NN / 16) * 2048u;  // [NCH][NN / 16] (only with dX)
  static __host__ __device__ uint32_t misc(bool need_dx) { return img_inT + (need_dx ? NCH * (NN / 16) * 2048u : 0u); }
  static __host__ __device__ uint32_t stage(bool need_dx) { return misc(need_dx) + 256u; }
  static __host__ __device__ uint32_t total(bool need_dx, uint32_t nw) { return stage(need_dx) + nw * BWD_WAVE_FLOATS * 4u; }
};

// the backward kernel's prologue: the weight matrices of one weight set in both orientations -> operand images in LDS
template <int NCH, int MT>
__device__ __forceinline__ void build_bwd_images(unsigned char* lds, const float* __restrict__ pw, uint32_t n_in, uint32_t n_out,
                                                 bool need_dx, uint32_t n_in_w = 0) {
  if (n_in_w == 0) n_in_w = n_in;
  constexpr int NT = NN / 32;
  constexpr uint32_t NS0 = 2 * NCH, NSO = 2 * MT;
  using L = BwdLds<NCH, MT>;
  _Float16* img_in = reinterpret_cast<_Float16*>(lds + L::img_in);
  _Float16* img_h = reinterpret_cast<_Float16*>(lds + L::img_h);
  _Float16* img_outT = reinterpret_cast<_Float16*>(lds + L::img_outT);
  _Float16* img_hT = reinterpret_cast<_Float16*>(lds + L::img_hT);
  _Float16* img_inT = reinterpret_cast<_Float16*>(lds + L::img_inT);
  int* wexp = reinterpret_cast<int*>(lds + L::misc(need_dx));
  float* red = reinterpret_cast<float*>(lds + L::misc(need_dx) + 64);
  const float* wh = pw + NN * n_in_w;
  const float* wout = wh + (NL - 1) * NN * NN;
  ImgQuads<NN * NCH * 32 / 4 / 256> q_in;                        // NN x (32 NCH) / 4 / 256 threads
  ImgQuads<NN * NN / 4 / 256> q_h;
  ImgQuads<MT * 32 * NN / 4 / 256> q_out;
  const float m_in = image_load(q_in, pw, NN, n_in, n_in_w);
  const float m_h = (NL == 2) ? image_load(q_h, wh, NN, NN) : 0.f;
  const float m_out = image_load(q_out, wout, n_out, NN);
  lds_zero16(lds, L::misc(need_dx));
  block_scale_exps(m_in, m_h, m_out, red, wexp);
  const float s_in = pow2f(wexp[0]), s_h = pow2f(wexp[1]), s_out = pow2f(wexp[2]);
  image_scatter(q_in, img_in, NN, n_in, false, NT, NS0, K_NAT, s_in);
  if (need_dx) image_scatter(q_in, img_inT, NN, n_in, true, NCH, NN / 16, K_CHAIN, s_in);
  if constexpr (NL == 2) {
    image_scatter(q_h, img_h, NN, NN, false, NT, NN / 16, K_CHAIN, s_h);
    image_scatter(q_h, img_hT, NN, NN, true, NT, NN / 16, K_CHAIN, s_h);
  }
  image_scatter(q_out, img_outT, n_out, NN, true, NT, NSO, K_NAT, s_out);
}

// dns_mlp_prepare: grid (n_sets, 2) -- blockIdx.y = 0 builds a weight set's FORWARD images, 1 its backward images (always with
// the dX image: without dX the backward kernel copies the prefix that precedes it); each writes [image area | exponents]
template <int NCH, int MT>
__global__ __launch_bounds__(256) void mlp_prepare_kernel(const float* __restrict__ params, uint32_t param_stride, uint32_t n_in,
                                                          uint32_t n_out, unsigned char* __restrict__ blob, uint32_t fwd_bytes,
                                                          uint32_t blob_stride, uint32_t n_in_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const float* pw = params + (size_t)blockIdx.x * param_stride;
  unsigned char* dst = blob + (size_t)blockIdx.x * blob_stride;
  if (blockIdx.y == 0) {
    using LF = FwdLds<NN, NL>;
    build_fwd_images<NN, NL>(lds, pw, n_in, n_out, n_in_w);
    __syncthreads();
    images_copy_out(lds, dst, LF::misc(n_in, n_out), reinterpret_cast<const int*>(lds + LF::misc(n_in, n_out)));
    dst += LF::misc(n_in, n_out) + 16u;
  } else {
    using L = BwdLds<NCH, MT>;
    build_bwd_images<NCH, MT>(lds, pw, n_in, n_out, true, n_in_w);
    __syncthreads();
    images_copy_out(lds, dst + fwd_bytes, L::misc(true), reinterpret_cast<const int*>(lds + L::misc(true)));
    dst += fwd_bytes + L::misc(true) + 16u;
  }
  // a lone last output column (tail_shape): W_out's last row in fp32 behind the exponents, for the tail-column kernels
  if (tail_shape(n_out) && threadIdx.x < (uint32_t)NN)
    reinterpret_cast<float*>(dst)[threadIdx.x] = pw[NN * n_in_w + (NL - 1) * NN * NN + (n_out - 1u) * NN + threadIdx.x];
}

// SH: the hidden activations come from what the forward kept (a.h_saved) instead of being recomputed from x (phase A)
// XS: x arrives in the split-row format (split_rows.hpp): phase A's operand fragments come straight from memory
// (a __device__ body so that the fused tracker iteration, track_fused.inc, can run it as one of its phases: vb = the workgroup's
//  index in this launch's grid, lds = the workgroup's dynamic LDS)
// TAIL = 1: n_out = 32 MT + 1 (tail_shape; MT = 0 or 1).  MT output tiles run on the matrix pipe as before, the last column
// ("tail column", mlp_split.hpp) on the vector ALU: its dY is one dword per point, its share of dH_last one FMA per hidden
// unit on the fp32 accumulators, its row of dW_out 16 NT per-lane partial sums over the lane's points -- persistent like
// acc_out (zeroed and flushed at the same two places), reduced over the 32 point lanes once per run.  The LDS image area and the
// prepared blob keep the layout of the MT + 1 tiles the column used to cost; its tile of them is not read.
template <int NCH, int MT, int PREC, bool WITH_DW, bool SH = false, bool XS = false, int NW = 4, int TAIL = 0>
__device__ __forceinline__ void mlp_bwd_body(const BwdArgs& a, uint32_t vb, unsigned char* lds) {
  static_assert(NW == 4 || !WITH_DW, "the weight-gradient reduction (flush_tile) is written for 4 waves");
  static_assert(MT >= 1 || TAIL == 1, "no output column");
  constexpr uint32_t BT_SLOTS = 32u * NW;        // point slots per workgroup tile
  constexpr int NT = NN / 32;
  constexpr int MA = MT > 0 ? MT : 1;            // array extents (MT = 0: the arrays are unused)
  constexpr uint32_t NS0 = 2 * NCH, NSO = 2 * (MT + TAIL);     // (K-steps of the W_out^T image AS LAID OUT; 2 MT of them are run)
  using L = BwdLds<NCH, MT + TAIL>;
  // the wave index as a SCALAR: everything derived from it (slot numbers, the staging tile's address) stays out of the vector
  // registers and the vector ALU
  const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t n_in = a.n_in, n_out = a.n_out;
  const bool need_dx = a.dx != nullptr;
  const uint32_t n_btiles = (a.n_slots + BT_SLOTS - 1u) / BT_SLOTS;
  const uint32_t bt0 = vb * a.tiles_per_block;
  const uint32_t bt1 = min(bt0 + a.tiles_per_block, n_btiles);
  _Float16* img_in = reinterpret_cast<_Float16*>(lds + L::img_in);
  _Float16* img_h = reinterpret_cast<_Float16*>(lds + L::img_h);
  _Float16* img_outT = reinterpret_cast<_Float16*>(lds + L::img_outT);
  _Float16* img_hT = reinterpret_cast<_Float16*>(lds + L::img_hT);
  _Float16* img_inT = reinterpret_cast<_Float16*>(lds + L::img_inT);
  int* wexp = reinterpret_cast<int*>(lds + L::misc(need_dx));
  float* stg_base = reinterpret_cast<float*>(lds + L::stage(need_dx));
  float* stg = stg_base + wave * BWD_WAVE_FLOATS;
  int* rows_all = reinterpret_cast<int*>(stg + STG_FLOATS);
  float* rmax = stg + STG_FLOATS + STG_ROWS;
  uint32_t* offs = reinterpret_cast<uint32_t*>(stg + STG_WAVE_FLOATS);   // the tile's row offsets in dy | d_x | d_x2 (bytes)
  float* w_tail = reinterpret_cast<float*>(lds + L::total(need_dx, NW));  // (TAIL) 2^wexp[2] * W_out's last row, fp32 (exact)
  const uint32_t n_out_mat = n_out - (uint32_t)TAIL;                       // output columns on the matrix pipe
  // buffer descriptors of everything the tile loop loads or stores behind a row / column guard (mlp_split.hpp)
  const rsrc_t r_dy = buf_make(a.dy), r_dh1 = buf_make(a.dh1), r_ri = buf_make(a.row_index);
  DxIo io;
  io.r1 = buf_make(a.dx);
  io.r2 = buf_make(a.dseg.dx2);
  io.two = a.dseg.dx2 != nullptr ? 1u : 0u;
  io.acc1 = a.dseg.acc1;
  io.acc2 = a.dseg.acc2;
  io.n_in1 = a.seg.n_in1;
  io.col_lo = a.dseg.col_lo;
  // rows whose byte offset in the widest of dy / d_x / d_x2 would pass BUF_LIMIT are refused (only a row TABLE can name one:
  // slot-ordered rows are checked by the launcher)
  uint32_t ld_max = a.lddy;
  if (a.dx) ld_max = max(ld_max, a.lddx);
  if (a.dseg.dx2) ld_max = max(ld_max, a.dseg.lddx2);
  const uint32_t row_limit = BUF_LIMIT / (4u * max(ld_max, 1u));
  uint32_t bad_rows = 0;
  // the row of slot slot0 + (lane & 31) (-1: a padding slot); with a row table the load is in flight when this returns
  // (the value is not touched before rows_commit: a select right behind the load would wait for it -- and, vmcnt being in
  //  order, for every store in front of it)
  auto row_fetch = [&](uint32_t slot0) -> int {
    const uint32_t slot = slot0 + (lane & 31u);
    int row = (int)slot;
    if (a.row_index) row = (int)__builtin_amdgcn_raw_buffer_load_b32(r_ri, (int)(slot < a.n_slots ? slot * 4u : BUF_OOB), 0, 0);
    return row;
  };
  auto rows_commit = [&](int* rows_lds, int row, uint32_t slot0) {
    if (lane < 32u) rows_lds[lane] = (slot0 + lane < a.n_slots) ? row : -1;
    wave_lds_fence();
  };

  // weight-gradient accumulators of the wave (rows = dW rows in the 16 registers, lanes = dW columns)
  f32x16 acc_out[WITH_DW ? MA : 1][WITH_DW ? NT : 1];     // [row tile of n_out][column tile of the hidden width]
  f32x16 part[WITH_DW && TAIL ? NT : 1];                   // (TAIL) the lane's partial sums of dW_out's last row: dy_tail * H_last
  f32x16 acc_h[WITH_DW && NL == 2 ? NT : 1][WITH_DW && NL == 2 ? NT : 1];
  XChunk xc[(SH || XS) ? 1 : NCH];              // the tile's input chunks (recompute)
  XsTile xt;                                    // (XS) the tile's input fragments
  XChunk hc1[SH ? NN / 32 : 1], hc2[SH && NL == 2 ? NN / 32 : 1];   // (SH) the tile's saved hidden activations
  auto group_of = [&](uint32_t t) -> int { return a.tile_group ? a.tile_group[t] : 0; };

  // runs of consecutive 128-slot tiles that share a weight set: images built, accumulators zeroed / flushed once per run
  for (uint32_t run0 = bt0; run0 < bt1;) {
    const int grp = group_of(run0);
    uint32_t run1 = run0 + 1;
    while (run1 < bt1 && group_of(run1) == grp) ++run1;
    if (grp < 0) {                              // padding tiles of an empty weight set
      run0 = run1;
      continue;
    }
    __syncthreads();
    DNS_TR_RUN(0);
    uint32_t cur_buf = 0;
#ifdef DNS_BWD_TRACE
    uint32_t tr_tile = 0;
#endif
    // The run's first tile: its rows and inputs are requested here -- IN FRONT of the weight images' copy-in / build (independent
    // of it: a one-tile launch otherwise pays the rows' memory latency behind the images') --, every later tile's while the tile in front of it runs
    // (below, in front of E).  ONE request site inside the loop: with a second one at the top of the loop body ("not requested
    // yet") the two definitions met in a copy of all input registers behind s_waitcnt vmcnt(0) at every tile start -- a wait
    // for every store of the previous tile (round 4's kernel; found in the ISA in round 5).
    int row_next = row_fetch(run0 * BT_SLOTS + wave * 32u);
    rows_commit(rows_all, row_next, run0 * BT_SLOTS + wave * 32u);
    if constexpr (SH) {
#pragma unroll
      for (int t = 0; t < NT; ++t) h_chunk_issue(hc1[t], a.h_saved, NN, run0 * BT_SLOTS + wave * 32u, a.n_slots, t, lane);
      if constexpr (NL == 2) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          h_chunk_issue(hc2[t], a.h_saved + (size_t)a.n_slots * NN, NN, run0 * BT_SLOTS + wave * 32u, a.n_slots, t, lane);
      }
    } else if constexpr (XS) {
      xs_issue<PREC>(xt, a.xs, n_in >> 4, rows_all, lane);
    } else {
#pragma unroll
      for (int c = 0; c < NCH; ++c) x_chunk_issue(xc[c], a.x, a.ldx, a.seg, n_in, rows_all, c, lane);
    }
    if (a.prep) {
      // prepared with the dX image last: without dX the image area is the prefix in front of it; the exponents sit behind
      // the FULL area in the blob
      const unsigned char* src = a.prep + (size_t)grp * a.prep_stride;
      images_copy_in(lds, src, L::misc(need_dx), src + L::misc(true), wexp);
      if (TAIL && threadIdx.x < (uint32_t)NN)
        w_tail[threadIdx.x] = ldexpf(reinterpret_cast<const float*>(src + L::misc(true) + 16u)[threadIdx.x], reinterpret_cast<const int*>(src + L::misc(true))[2]);
    } else {
      const float* pw = a.params + (size_t)grp * a.param_stride;
      build_bwd_images<NCH, MT + TAIL>(lds, pw, n_in, n_out, need_dx, a.n_in_w);     // (wexp is final behind the barrier of its block_scale_exps)
      if (TAIL && threadIdx.x < (uint32_t)NN)
        w_tail[threadIdx.x] = ldexpf(pw[NN * a.n_in_w + (NL - 1) * NN * NN + (n_out - 1u) * NN + threadIdx.x], wexp[2]);
    }
    __syncthreads();
    DNS_TR_RUN(1);
    if constexpr (WITH_DW) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc_out[i][j] = zero16();
      if constexpr (TAIL != 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) part[j] = zero16();
      }
      if constexpr (NL == 2) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc_h[i][j] = zero16();
      }
    }
    for (uint32_t bt = run0; bt < run1; ++bt, cur_buf ^= 1u) {
    const uint32_t slot0 = bt * BT_SLOTS + wave * 32u;
    DNS_TR(0);
    const int* rows_lds = rows_all + 32u * cur_buf;
    // the NEXT tile's rows (a row table is a dependent load in front of the next tile's x): requested a whole tile ahead
    if (bt + 1 < run1) row_next = row_fetch((bt + 1) * BT_SLOTS + wave * 32u);
    tile_offs_publish(offs, rows_lds, a.lddy, a.lddx, a.dseg.lddx2, row_limit, bad_rows, lane);
    // dY of the tile: requested now, used after the recompute
    DyChunk dyc[MA];
#pragma unroll
    for (int c = 0; c < MT; ++c) dy_chunk_issue_buf(dyc[c], r_dy, offs, n_out_mat, c, lane);
    // (TAIL) the point's dY in the last column: one dword, the same in both lane halves; a padding slot reads zero
    float dy_tail = 0.f;
    if constexpr (TAIL != 0) dy_tail = buf_load1(r_dy, offs[lane & 31u] + 4u * (n_out - 1u));

    // ---- A: the hidden activations: recomputed from x, or (SH) read back as the forward kept them ----------------------
    int k0 = 0, k1 = 0;
    f32x16 h1[NT];
    f32x16 h2[NT];
    if constexpr (SH) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        x_chunk_commit(hc1[t], stg, lane);
        h1[t] = acc_tile_read(stg, lane);
      }
      if constexpr (NL == 2) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          x_chunk_commit(hc2[t], stg, lane);
          h2[t] = acc_tile_read(stg, lane);
        }
      }
    } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) h1[t] = zero16();
    if constexpr (XS) {
      // K-steps past n_in exist only when n_in is not a multiple of 32 (NS0 = 2 NCH): their image columns are zero, and
      // xs_issue loads only steps below n_in / 16 -- the remaining fragments are skipped here (uniform)
      const uint32_t ns_live = n_in >> 4;
      k0 = xs_align<PREC>(xt, a.xs, ns_live) + wexp[0];
      layer_first_xs<PREC, NT>(xt, ns_live, img_in, NS0, lane, h1);
    } else {
    x_row_max<NCH>(xc, NCH, rmax, lane);
    k0 = scale_exp(rmax[lane & 31u]);
    const float sx = pow2f(k0);
    k0 += wexp[0];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float xs[16];
      x_chunk_commit(xc[c], stg, lane);
      x_chunk_read(xs, stg, lane);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xs[8 * s + j];
        const Frag b = split8(v, sx);
#pragma unroll
        for (int t = 0; t < NT; ++t) h1[t] = mma<PREC>(load_frag<PREC>(img_in, NS0, t, 2 * c + s, lane), b, h1[t]);
      }
    }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) h1[t][r] = relu(h1[t][r]);
    if constexpr (NL == 2) {
      const int kf = scale_exp(tile_max<NT>(h1));
      layer_chain<PREC, NT, NT>(h1, pow2f(kf), img_h, lane, h2);
      k1 = k0 + kf + wexp[1];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h2[t][r] = relu(h2[t][r]);
    }
    }
    f32x16(&hl)[NT] = (NL == 2) ? h2 : h1;
    const int khl = (NL == 2) ? k1 : k0;      // hl holds 2^khl * H_last (per lane)

    DNS_TR(1);
    // ---- B: dH_last = W_out^T dY (.) relu' ----------------------------------------------------------------------
    float dys[MA][16];
    float dyt[WITH_DW ? MA : 1][16];           // the same tile column-wise (lane = output column): phase C's operand
    float dymax = fabsf(dy_tail);              // (0 without a tail column)
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      dy_chunk_commit(dyc[c], stg, lane);
      if constexpr (WITH_DW) stage_read_cols(dyt[c], stg, lane);   // while the tile sits in LDS: no second trip to L1 / L2
      x_chunk_read(dys[c], stg, lane);        // row-wise: the point's columns 16 s + 8 h + j; fences after the reads
#pragma unroll
      for (int e = 0; e < 16; ++e) dymax = fmaxf(dymax, fabsf(dys[c][e]));
    }
    dymax = max_halves(dymax);
    const int kdy = scale_exp(dymax);
    f32x16 dl[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dl[t] = zero16();
    {
      const float sdy = pow2f(kdy);
#pragma unroll
      for (int c = 0; c < MT; ++c) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = dys[c][8 * s + j];
          const Frag b = split8(v, sdy);
#pragma unroll
          for (int t = 0; t < NT; ++t) dl[t] = mma<PREC>(load_frag<PREC>(img_outT, NSO, t, 2 * c + s, lane), b, dl[t]);
        }
      }
    }
    const int kdl = kdy + wexp[2];            // dl holds 2^kdl * dH_last
    if constexpr (TAIL != 0) {
      // the tail column's share, at dl's exponent: (2^wexp[2] w)(2^kdy dy) -- both factors exact (below 2^14 in magnitude, as
      // the matrix operands are; the row is kept scaled in LDS), one rounding for the FMA
      const float dts = dy_tail * pow2f(kdy);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        float w[16];
        tail_weights(w, w_tail, t, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) dl[t][r] = fmaf(w[r], dts, dl[t][r]);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dl[t][r] = hl[t][r] > 0.f ? dl[t][r] : 0.f;

    DNS_TR(2);
    // ---- C: dW_out += dY x H_last (sum over the tile's points) ---------------------------------------------------
    if constexpr (WITH_DW && TAIL != 0) {
      // the tail column's row of dW_out: the lane's point contributes dy_tail * H_last to its 16 NT hidden units (true scale:
      // the exponent of hl is undone exactly); one FMA rounding per tile, the cross-lane sum waits for the end of the run
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[t][r] = fmaf(dy_tail, ldexpf(hl[t][r], -khl), part[t][r]);
    }
    if constexpr (WITH_DW && MT > 0) {
      // dY^T-form: lane = output column, elements = 8 consecutive points -- taken from the staged tile in phase B (round 2
      // first re-read it from L1 as dwords here: a full memory latency exposed per tile at one wave per SIMD)
      Frag3 fa[MA][2];
#pragma unroll
      for (int c = 0; c < MT; ++c)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = dyt[c][8 * s + j];
          fa[c][s] = split8_bf3(v);
        }
      // Software-pipelined over the hidden tiles: tile tn+1's transposition (staging write, LDS round trip, read, bf16 split)
      // sits BESIDE tile tn's matrix instructions -- the read and the ~100 conversion instructions of the split are
      // independent of them and in one scheduling region with them, so the matrix pipe works under the vector work instead
      // of behind it (round 4: transposition, then 24 matrix instructions back to back, per tile)
      Frag3 fb[2][2];
      transpose_frags(hl[0], khl, fb[0], stg, lane);
#pragma unroll
      for (int tn = 0; tn < NT; ++tn) {
        TrRaw raw;
        if (tn + 1 < NT) {
          transpose_write(hl[tn + 1], khl, stg, lane);
          transpose_read(raw, stg, lane);
        }
#pragma unroll
        for (int c = 0; c < MT; ++c)
#pragma unroll
          for (int s = 0; s < 2; ++s) acc_out[c][tn] = mma_pt<PREC>(fa[c][s], fb[tn & 1][s], acc_out[c][tn]);
        if (tn + 1 < NT) {
          transpose_split(raw, fb[(tn + 1) & 1]);
          wave_lds_fence();
        }
      }
    }

    DNS_TR(3);
    // ---- D: dH_1 = W_h^T dH_2 (.) relu', dW_h += dH_2 x H_1 --------------------------------------------------------
    f32x16 d1[NT];
    int kd1 = kdl;
    if constexpr (NL == 2) {
      float m = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(dl[t][r]));
      m = max_halves(m);
      const int kf = scale_exp(m);
      layer_chain<PREC, NT, NT>(dl, pow2f(kf), img_hT, lane, d1);
      kd1 = kdl + kf + wexp[1];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) d1[t][r] = h1[t][r] > 0.f ? d1[t][r] : 0.f;
      if constexpr (WITH_DW) {
        Frag3 fa[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t) transpose_frags(dl[t], kdl, fa[t], stg, lane);
        Frag3 fb[2][2];                          // (pipelined like phase C)
        transpose_frags(h1[0], k0, fb[0], stg, lane);
#pragma unroll
        for (int tn = 0; tn < NT; ++tn) {
          TrRaw raw;
          if (tn + 1 < NT) {
            transpose_write(h1[tn + 1], k0, stg, lane);
            transpose_read(raw, stg, lane);
          }
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) acc_h[t][tn] = mma_pt<PREC>(fa[t][s], fb[tn & 1][s], acc_h[t][tn]);
          if (tn + 1 < NT) {
            transpose_split(raw, fb[(tn + 1) & 1]);
            wave_lds_fence();
          }
        }
      }
    }
    f32x16(&df)[NT] = (NL == 2) ? d1 : dl;   // 2^kd1 * dH_1 (per lane)

    // E's first read-add-write operand: requested in front of the next tile's x rows, so that waiting for it does not wait for them
    // (d_x / d_x2 rows of any 4-byte alignment: the 16-byte buffer accesses need dword alignment only -- the HSA ABI runs the
    //  memory pipeline in unaligned-access mode; round 4's separate dword path for rows that are not 16-byte aligned is gone)
    // DNS_MLP_DX_FIRST (two-segment input, no d_x2): only the first segment's columns have a gradient consumer
    const uint32_t dx_cols = (a.seg.x2 != nullptr && a.dseg.dx2 == nullptr) ? a.seg.n_in1 : n_in;
    const uint32_t it_lo = a.dseg.col_lo >> 5;             // (DNS_MLP_DX_FROM) whole tiles of columns nobody reads are skipped
    const uint32_t it_hi = min((uint32_t)NCH, (dx_cols + 31u) >> 5);   // chunks past n_in exist only as zero padding
    // the next tile of the same weight set: its rows are requested now and arrive during E
    if (bt + 1 < run1) {
      int* nrows_lds = rows_all + 32u * (cur_buf ^ 1u);
      rows_commit(nrows_lds, row_next, (bt + 1) * BT_SLOTS + wave * 32u);
      if constexpr (SH) {
        const uint32_t nslot0 = (bt + 1) * BT_SLOTS + wave * 32u;
#pragma unroll
        for (int t = 0; t < NT; ++t) h_chunk_issue(hc1[t], a.h_saved, NN, nslot0, a.n_slots, t, lane);
        if constexpr (NL == 2) {
#pragma unroll
          for (int t = 0; t < NT; ++t) h_chunk_issue(hc2[t], a.h_saved + (size_t)a.n_slots * NN, NN, nslot0, a.n_slots, t, lane);
        }
      } else if constexpr (XS) {
        xs_issue<PREC>(xt, a.xs, n_in >> 4, nrows_lds, lane);
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c) x_chunk_issue(xc[c], a.x, a.ldx, a.seg, n_in, nrows_lds, c, lane);
      }
    }

    DNS_TR(4);
    // ---- E: dH_1 -> workspace (for the dW_in kernel); dX = W_in^T dH_1 --------------------------------------------
    if constexpr (WITH_DW) {
      if (a.dh1) {
        const uint32_t nrows = slot0 < a.n_slots ? min(32u, a.n_slots - slot0) : 0u;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x16 v;
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = ldexpf(df[t][r], -kd1);
          store_tile_staged_buf(r_dh1, slot0 * (uint32_t)(NN * 4), NN, t * 32, nrows, v, stg, lane);
        }
      }
    }
    DNS_TR(5);
    if (need_dx) {
      float dfmax = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dfmax = fmaxf(dfmax, fabsf(df[t][r]));
      dfmax = max_halves(dfmax);
      const int kf = scale_exp(dfmax);
      const float fdf = pow2f(kf);
      const int kxo = kd1 + kf + wexp[0];
      // Order of the vector-memory instructions of a column tile: [what the NEXT tile's store adds to] then [this tile's
      // stores] -- vmcnt counts loads and stores in issue order, so a load that follows a store cannot be waited for without
      // waiting for the store's round trip as well (round 4's kernel: every store of a tile behind the one in front of it)
      // Read-add-write launches (acc) and overwriting ones run the column tiles through two COPIES of the code, picked by one
      // uniform branch: the waits hipcc inserts follow the control-flow graph, not the values of conditions -- with the
      // requests under `if (acc)` in one place and their consumers under `if (acc)` in another it sees a path on which
      // requested values are never consumed, and waits for them (and for every store in front of them) at the next tile's top.
      auto dx_tiles = [&](auto acc_c) {
        constexpr bool ACC = decltype(acc_c)::value;
        DxOld old_cur;
        if constexpr (ACC) dx_old_issue_buf(old_cur, io, offs, it_lo * 32u, min(32u, dx_cols - it_lo * 32u), lane);
        auto dx_tile = [&](uint32_t it0, bool has_next) {
          const uint32_t col0 = it0 * 32u;
          const uint32_t ncols = min(32u, dx_cols - col0);
          f32x16 o[1];
          layer_chain<PREC, 1, NT>(df, fdf, img_inT + (size_t)it0 * (NN / 16) * 1024u, lane, o);
#pragma unroll
          for (int r = 0; r < 16; ++r) o[0][r] = ldexpf(o[0][r], -kxo);
          store_tile_rows_buf(io, offs, col0, ncols, o[0], old_cur, ACC, has_next, has_next ? min(32u, dx_cols - col0 - 32u) : 0u, stg, lane);
        };
        // a real loop (unrolled, the tiles' live ranges overlap and spill) over all column tiles but the last, each of which
        // requests what the NEXT one adds to; the last one is peeled: it requests nothing, so nothing is in flight behind it
        for (uint32_t it0 = it_lo; it0 + 1u < it_hi; ++it0) dx_tile(it0, true);
        dx_tile(it_hi - 1u, false);
      };
      if (it_lo < it_hi) {
        const bool acc_any = io.acc1 != 0u || (io.two != 0u && io.acc2 != 0u);
        if (acc_any) dx_tiles(std::true_type{});
        else dx_tiles(std::false_type{});
      }
    }
    DNS_TR(6);
#ifdef DNS_BWD_TRACE
    ++tr_tile;
#endif
    }   // tiles of the run
    // the run's weight gradients: the four waves' copies are added in LDS, then 128-byte row segments of float atomics
    DNS_TR_RUN(2);
    __syncthreads();
    if constexpr (WITH_DW) {
      if (a.d_params) {
        float* dW_h = a.d_params + (size_t)grp * a.param_stride + (size_t)NN * a.n_in_w;
        float* dW_out = dW_h + (size_t)(NL - 1) * NN * NN;
        if constexpr (NL == 2) {
#pragma unroll
          for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              flush_tile<BWD_WAVE_FLOATS>(acc_h[i][j], dW_h + (size_t)(32 * i) * NN + 32 * j, NN, 32u, 32u, stg_base, wave, lane);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            flush_tile<BWD_WAVE_FLOATS>(acc_out[i][j], dW_out + (size_t)(32 * i) * NN + 32 * j, NN, n_out_mat > 32u * i ? n_out_mat - 32u * i : 0u, 32u,
                       stg_base, wave, lane);
        if constexpr (TAIL != 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j)
            flush_tail<BWD_WAVE_FLOATS>(part[j], dW_out + (size_t)(n_out - 1u) * NN + 32 * j, stg_base, stg_base + STG_FLOATS + STG_ROWS, wave, lane);
        }
      }
    }
    DNS_TR_RUN(3);
    run0 = run1;
  }   // runs
  if (bad_rows != 0u && a.err) atomicOr(a.err, DNS_DEVERR_MLP_RANGE);
}

template <int NCH, int MT, int PREC, bool WITH_DW, bool SH = false, bool XS = false, int NW = 4, int TAIL = 0>
__global__ __launch_bounds__(64 * NW, 1) void mlp_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  mlp_bwd_body<NCH, MT, PREC, WITH_DW, SH, XS, NW, TAIL>(a, blockIdx.x, lds);
}

#if defined(DNS_BWD_DEV_ONE)
// tools build (hipcc -S of ONE instance in seconds instead of the file's 78: tools/isa_one.sh): nothing else is instantiated
template __global__ void mlp_bwd_kernel<DNS_BWD_DEV_ONE>(BwdArgs);
#elif !defined(DNS_BWD_BODY_ONLY)            // (BODY_ONLY: track_fused.inc wants BwdLds + mlp_bwd_body, no launchers)
template <int NCH, int MT, int TAIL>
bool set_attrs() {
  bool ok = true;
  auto set = [&](const void* f) { ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_DYN_LDS) == hipSuccess; };
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, true, false, false, 4, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, false, false, false, 4, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, true, true, false, 4, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, false, false, false, 8, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, true, false, true, 4, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, false, false, true, 4, TAIL>);
  set((const void*)mlp_bwd_kernel<NCH, MT, 3, false, false, true, 8, TAIL>);
  if constexpr (TAIL == 0) {                     // the fp16-operand arithmetic and the image builder have no tail-column form
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, true>);
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, false>);
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, true, false, true>);
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, false, false, true>);
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, false, false, false, 8>);
    set((const void*)mlp_bwd_kernel<NCH, MT, 1, false, false, true, 8>);
    set((const void*)mlp_prepare_kernel<NCH, MT>);
  }
  return ok;
}

// (tail-column instances exist for up to 96 input columns: with four input chunks the <4, 1, TAIL> weight-gradient instance
//  spills 54 registers where <4, 2> spills 2, and no network of the project has that shape)
template <int NCH>
bool set_attrs_nch() {
  bool ok = set_attrs<NCH, 1, 0>() && set_attrs<NCH, 2, 0>();
  if constexpr (NCH < 4) ok = ok && set_attrs<NCH, 0, 1>() && set_attrs<NCH, 1, 1>();
  return ok;
}

int init_attrs() {
  const bool ok = set_attrs_nch<1>() && set_attrs_nch<3>() && set_attrs_nch<4>();
  if (!ok) {
    set_error("dns_init: hipFuncSetAttribute failed for the MLP backward kernels");
    return DNS_E_LAUNCH;
  }
  return DNS_OK;
}
AttrRegistrar attr_registrar(init_attrs);

// TAIL = 1 (fp32-grade arithmetic only): the LDS of the MT + 1 tile layout plus W_out's last row
template <int NCH, int MT, int TAIL = 0>
void launch(const BwdArgs& a, uint32_t blocks, bool fp16_single, hipStream_t st) {
  const bool xs = a.xs.s1.rows != nullptr;
  constexpr size_t tail_bytes = TAIL ? NN * 4u : 0u;
#define DNS_BWD_GO(PREC_, DW_, SH_, XS_, NW_, lds_)                                                                             \
  {                                                                                                                             \
    if constexpr (TAIL == 0 || PREC_ == 3)                                                                                      \
      DNS_LAUNCH((mlp_bwd_kernel<NCH, MT, PREC_, DW_, SH_, XS_, NW_, TAIL>), dim3(blocks), dim3(64 * NW_), lds_, st, a);       \
  }
  if (a.n_waves == 8u) {                         // frozen-scene form, two waves per SIMD (mlp_split.hip picks it: no d_params, no groups)
    const size_t lds8 = BwdLds<NCH, MT + TAIL>::total(a.dx != nullptr, 8u) + tail_bytes;
    if (xs) {
      if (fp16_single) DNS_BWD_GO(1, false, false, true, 8, lds8)
      else DNS_BWD_GO(3, false, false, true, 8, lds8)
    } else {
      if (fp16_single) DNS_BWD_GO(1, false, false, false, 8, lds8)
      else DNS_BWD_GO(3, false, false, false, 8, lds8)
    }
    return;
  }
  const size_t lds_bytes = BwdLds<NCH, MT + TAIL>::total(a.dx != nullptr, 4u) + tail_bytes;
  if (xs) {
    if (a.d_params) {
      if (fp16_single) DNS_BWD_GO(1, true, false, true, 4, lds_bytes)
      else DNS_BWD_GO(3, true, false, true, 4, lds_bytes)
    } else {
      if (fp16_single) DNS_BWD_GO(1, false, false, true, 4, lds_bytes)
      else DNS_BWD_GO(3, false, false, true, 4, lds_bytes)
    }
    return;
  }
  if (a.d_params) {
    if (fp16_single) DNS_BWD_GO(1, true, false, false, 4, lds_bytes)
    else if (a.h_saved) DNS_BWD_GO(3, true, true, false, 4, lds_bytes)
    else DNS_BWD_GO(3, true, false, false, 4, lds_bytes)
  } else {
    if (fp16_single) DNS_BWD_GO(1, false, false, false, 4, lds_bytes)
    else DNS_BWD_GO(3, false, false, false, 4, lds_bytes)
  }
#undef DNS_BWD_GO
}

#endif  // DNS_BWD_DEV_ONE / DNS_BWD_BODY_ONLY
}  // namespace

#if !defined(DNS_BWD_DEV_ONE) && !defined(DNS_BWD_BODY_ONLY)
#define DNS_CAT3(a, b, c) a##b##_##c
#define DNS_LAUNCH_NAME(nn, nl) DNS_CAT3(launch_bwd_, nn, nl)
int DNS_LAUNCH_NAME(DNS_BWD_NN, DNS_BWD_NL)(const BwdArgs& a, uint32_t blocks, bool fp16_single, hipStream_t st) {
  const uint32_t nch = a.n_in <= 32u ? 1u : (a.n_in <= 96u ? 3u : 4u), mt = a.n_out <= 32u ? 1u : 2u;
  // a lone last output column (n_out = 1, 33) runs on the vector ALU: one matrix tile less (DESIGN 4.22).  fp32 rows and split
  // rows alike (their results are bit-identical: tests/test_gpu_split_rows.py); the fp16-operand arithmetic and n_in > 96 keep
  // their instances
  const bool tail = tail_shape(a.n_out) && !fp16_single && nch != 4u;
#define DNS_BWD_PICK(NCH_)                                          \
  {                                                                 \
    if (tail && mt == 1u) launch<NCH_, 0, 1>(a, blocks, false, st);  \
    else if (tail) launch<NCH_, 1, 1>(a, blocks, false, st);         \
    else if (mt == 1u) launch<NCH_, 1>(a, blocks, fp16_single, st);  \
    else launch<NCH_, 2>(a, blocks, fp16_single, st);                \
  }
  if (nch == 1u) DNS_BWD_PICK(1)
  else if (nch == 3u) DNS_BWD_PICK(3)
  else if (mt == 1u) launch<4, 1>(a, blocks, fp16_single, st);
  else launch<4, 2>(a, blocks, fp16_single, st);
#undef DNS_BWD_PICK
  return check_launch("dns_mlp_bwd");
}

#define DNS_PREP_NAME(nn, nl) DNS_CAT3(prepare_, nn, nl)
#define DNS_PREPB_NAME(nn, nl) DNS_CAT3(prepared_bwd_bytes_, nn, nl)
// bytes of one weight set's prepared backward images (image area with the dX image + 16 bytes of exponents)
uint32_t DNS_PREPB_NAME(DNS_BWD_NN, DNS_BWD_NL)(uint32_t n_in, uint32_t n_out) {
  const uint32_t nch = n_in <= 32u ? 1u : (n_in <= 96u ? 3u : 4u), mt = n_out <= 32u ? 1u : 2u;
  uint32_t b;
  if (nch == 1u) b = mt == 1u ? BwdLds<1, 1>::misc(true) : BwdLds<1, 2>::misc(true);
  else if (nch == 3u) b = mt == 1u ? BwdLds<3, 1>::misc(true) : BwdLds<3, 2>::misc(true);
  else b = mt == 1u ? BwdLds<4, 1>::misc(true) : BwdLds<4, 2>::misc(true);
  return b + 16u + (tail_shape(n_out) ? NN * 4u : 0u);
}
int DNS_PREP_NAME(DNS_BWD_NN, DNS_BWD_NL)(const float* params, uint32_t param_stride, uint32_t n_in, uint32_t n_out, uint32_t n_sets,
                                          unsigned char* blob, uint32_t fwd_bytes, uint32_t blob_stride, hipStream_t st, uint32_t n_in_w) {
  const uint32_t nch = n_in <= 32u ? 1u : (n_in <= 96u ? 3u : 4u), mt = n_out <= 32u ? 1u : 2u;
#define DNS_PREP_GO(NCH_, MT_)                                                                                        \
  {                                                                                                                   \
    const size_t lb = BwdLds<NCH_, MT_>::stage(true), lf = FwdLds<NN, NL>::stage(n_in, n_out);                        \
    const size_t lds_bytes = lb > lf ? lb : lf;                                                                       \
    DNS_LAUNCH((mlp_prepare_kernel<NCH_, MT_>), dim3(n_sets, 2), dim3(256), lds_bytes, st, params, param_stride, n_in,  \
               n_out, blob, fwd_bytes, blob_stride, n_in_w);                                                          \
  }
  if (nch == 1u) {
    if (mt == 1u) DNS_PREP_GO(1, 1) else DNS_PREP_GO(1, 2)
  } else if (nch == 3u) {
    if (mt == 1u) DNS_PREP_GO(3, 1) else DNS_PREP_GO(3, 2)
  } else {
    if (mt == 1u) DNS_PREP_GO(4, 1) else DNS_PREP_GO(4, 2)
  }
#undef DNS_PREP_GO
  return check_launch("dns_mlp_prepare");
}

#endif  // DNS_BWD_DEV_ONE
#undef NN
#undef NL

}  // namespace sp
}  // namespace dns
