/*
 * dns_hip.h -- C ABI of libdns_hip.so, the MI355X (gfx950) implementation of the
 * DNS-SLAM volumetric-rendering hot path.
 *
 * Drop-in boundary.  The reference is pure Python; the only native
 * code on its path is the third-party CUDA package `tinycudann`, reached through
 *   tcnn.Encoding(...)  reference models/pos_encoding.py:16,34,50,63,76,88
 *   tcnn.Network(...)   reference models/decoder.py:58,84,101,110, slams/mapping.py:737
 * plus stock torch ops in utils/common.py.  Each entry point below names the reference
 * interface it replaces.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked [host];
 *   - the caller owns all buffers (the library never allocates or frees device memory);
 *   - every launch goes to the caller's stream `stream` (a hipStream_t passed as void*);
 *     no entry point synchronises the device;
 *   - gradient outputs marked (+=) are ACCUMULATED into caller-initialised buffers;
 *   - return 0 on success, a negative DNS_E_* code on failure; dns_last_error() then holds
 *     a thread-local message.  No C++ exception crosses this boundary.
 *   - row-major tensors; `ld*` = leading dimension in elements.
 */
#ifndef DNS_HIP_H
#define DNS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNS_ABI_VERSION 29
#define DNS_MAX_LEVELS 32

#define DNS_OK 0
#define DNS_E_ARG (-1)      /* bad argument / unsupported shape */
#define DNS_E_LAUNCH (-2)   /* HIP launch error */
#define DNS_E_STATE (-3)    /* call refused in the current state (first use on a device inside a stream capture) */

/* Multi-resolution hash-grid level table (tcnn GridEncoding constructor; reference call site
 * models/pos_encoding.py:31-46).  Built once on the host by dns_grid_meta_init and passed by
 * pointer [host] to every grid entry point. */
typedef struct DnsGridMeta {
  uint32_t n_levels;
  uint32_t n_features;            /* features per level; this build supports 2 */
  uint32_t log2_hashmap_size;
  uint32_t base_resolution;
  uint32_t total_rows;            /* sum of size[] */
  float per_level_scale;
  float scale[DNS_MAX_LEVELS];    /* exp2f(l*log2f(pls))*base - 1 */
  uint32_t resolution[DNS_MAX_LEVELS];
  uint32_t size[DNS_MAX_LEVELS];  /* rows in the level */
  uint32_t offset[DNS_MAX_LEVELS];/* first row of the level */
  uint32_t hashed[DNS_MAX_LEVELS];/* 1 = coherent-prime hash, 0 = dense index */
} DnsGridMeta;

int dns_abi_version(void);
const char* dns_last_error(void);

/* One-time set-up of the CURRENT device: raises the dynamic-LDS limit of every kernel that stages more than 64 KB
 * (hipFuncSetAttribute -- a context-level call that is illegal while a stream is being captured and pointless per launch).
 * Idempotent and thread-safe.  Entry points call it implicitly on their first use on a device; inside a stream capture
 * that first use is refused with DNS_E_STATE instead, so a caller that captures hipGraphs (the reference's loops
 * slams/mapping.py:881-910, slams/tracking.py:313-340 replayed from a graph) calls dns_init() once after selecting the
 * device. */
int dns_init(void);

/* Measurement aid (bench.py's roofline): dns_kernel_timing(1) clears the record and brackets every kernel the library
 * launches from then on with an event pair on its launch stream (never inside a stream capture); dns_kernel_timing(0)
 * stops.  dns_kernel_timing_count() = spans recorded so far; dns_kernel_timing_get(i, ...) waits for span i and returns
 * the kernel's name and its duration in milliseconds. */
int dns_kernel_timing(int enable);
int dns_kernel_timing_count(void);
int dns_kernel_timing_get(int i, char* name, int name_cap, float* ms);

/* [host] fills *meta.  per_level_scale is the float64 value reference pos_encoding.py:33 computes. */
int dns_grid_meta_init(DnsGridMeta* meta, uint32_t n_levels, uint32_t n_features,
                       uint32_t log2_hashmap_size, uint32_t base_resolution, double per_level_scale);

/* ---- ray generation + depth-guided sampling ------------------------------------------------
 * Replaces, for K stacked target frames of n_per_frame rays each:
 *   get_rotation_from_quad  utils/common.py:447 (quat -> R, in-kernel)
 *   get_sample_uv/select_uv utils/common.py:266-293 (pixel gather; indices are an INPUT)
 *   get_rays_from_uv        utils/common.py:248-264
 *   box far clip            slams/mapping.py:519-527, slams/tracking.py:148-156 (fp64)
 *   sample_along_rays       utils/common.py:561-599 (per-frame max depth, per-ray sort)
 * pix_idx: flat index inside the window [H0,H1)x[W0,W1).  color [K,H,W,3], depth [K,H,W],
 * label [K,H,W] fp32.  quat [K,4] (w,x,y,z), trans [K,3].  cam = fx,fy,cx,cy [host].
 * bound [host] = 6 doubles b0x,b1x,b0y,b1y,b0z,b1z.  t_uniform [n_uniform] = linspace(0,1),
 * t_surf / t_zero the two jitter draws (t_surf already holds the forced 0.5): jitter_stride = 0 -> [n_surface], one
 * pair shared by the K frames; jitter_stride >= n_surface -> [K, jitter_stride], frame f reads its own row (the reference
 * calls sample_along_rays once per frame with fresh draws, slams/mapping.py:530).
 * depth_max_ws: K uint32 (bit patterns of the per-frame max sampled depth): scratch when depth_max_given == 0; when
 * depth_max_given != 0 the caller has filled it (multi-GPU: the max over ALL ranks' rays of the frame).  Outputs: rays_o,rays_d,gt_color [n,3], gt_depth [n],
 * gt_label [n] int64, inside [n] uint8 (far_bb >= depth, before the +0.01), z [n, n_uniform+n_surface]
 * ascending. */
int dns_raygen_sample(const int64_t* pix_idx, const float* color, const float* depth, const float* label,
                      const float* quat, const float* trans, const double* cam, const double* bound,
                      int H, int W, int H0, int H1, int W0, int W1, int n_frames, int n_per_frame,
                      const float* t_uniform, const float* t_surf, const float* t_zero,
                      int n_uniform, int n_surface, int jitter_stride, uint32_t* depth_max_ws, int depth_max_given,
                      float* rays_o, float* rays_d, float* gt_color, float* gt_depth, int64_t* gt_label,
                      uint8_t* inside, float* z, float* pts /* [n,S,3] = o + d*z (slams/mapping.py:531), NULL = skip */,
                      void* stream);

/* The free functions get_samples / get_samples_by_class / get_samples_by_uniq_class (utils/common.py:296-304,353-403:
 * the gather of select_uv / select_by_class :266-338 + get_rays_from_uv :248-264) and get_all_rays (:540-559), which take
 * the rotation as a MATRIX: n rays from the window [H0,H1)x[W0,W1) of ONE image.  pix_idx [n] window-flat indices (NULL:
 * ray r = pixel r, the whole-window order of get_all_rays); image [H,W,C] fp32 (C <= 8: rgb | depth | label; NULL with
 * sample NULL); R [9] row-major, T [3] on the DEVICE; cam [host] fx,fy,cx,cy.  Outputs rays_o, rays_d [n,3], sample [n,C]
 * (NULL = skip), ij [n,2] = (column, row) as fp32 like the reference's i, j (NULL = skip). */
int dns_rays_from_pixels(const int64_t* pix_idx, const float* image, int C, const float* R, const float* T,
                         const double* cam, int H, int W, int H0, int H1, int W0, int W1, int n,
                         float* rays_o, float* rays_d, float* sample, float* ij, void* stream);

/* Stand-alone sample_along_rays(gt_depth, n_samples, n_surface, far_bb, device) (utils/common.py:561-599):
 * gt_depth [n] fp32, far_bb [n] fp64 (already carrying the +0.01), batch-global max depth taken over the n
 * rays.  depth_max_ws: 1 uint32 scratch.  z [n, n_uniform+n_surface] ascending. */
int dns_sample_along_rays(const float* gt_depth, const double* far_bb, int n_rays, const float* t_uniform,
                          const float* t_surf, const float* t_zero, int n_uniform, int n_surface,
                          uint32_t* depth_max_ws, float* z, void* stream);

/* Backward of the ray generation w.r.t. the pose (autograd of pts = o + d*z, get_rays_from_uv and
 * quad2rotation, utils/common.py:248-264,406-429): d_quat [K,4] (+=), d_trans [K,3] (+=) from d_pts [n,S,3]
 * and/or direct d_rays_o / d_rays_d [n,3] (each may be NULL).  ws: dns_raygen_bwd_ws_floats(K, n_per_frame) floats of scratch
 * (one [12] partial sum per workgroup: no atomics, nothing to clear). */
int dns_raygen_bwd(const int64_t* pix_idx, const float* quat, const double* cam,
                   int H0, int H1, int W0, int W1, int n_frames, int n_per_frame, int S,
                   const float* z, const float* d_pts, const float* d_rays_o, const float* d_rays_d,
                   float* ws, float* d_quat, float* d_trans, void* stream);
uint64_t dns_raygen_bwd_ws_floats(int n_frames, int n_per_frame);

/* ---- point encoding: OneBlob + hash grid ---------------------------------------------------
 * Replaces Pos_Encoding.forward (models/decoder.py:45-48) = tcnn OneBlob (pos_encoding.py:61-71)
 * + tcnn HashGrid (pos_encoding.py:31-46), optionally preceded by the fp64 normalisation
 * (pts - b0)/(b1 - b0) of slams/mapping.py:608 / slams/tracking.py:190 when bound != NULL.
 * in [P,3]; if bound != NULL [host, 6 doubles] `in` holds world points and x_out [P,3] receives the
 * normalised fp32 coordinates (may be NULL).  pe_out [P, ld_pe] gets 3*n_bins channels (NULL = skip),
 * grid_out [P, ld_grid] gets n_levels*n_features channels (NULL = skip).  table [total_rows, F].
 * dy_dx (NULL = skip): [n_levels, 3, P, 2] floats, 8-byte aligned -- d(grid features)/d(normalised coordinate), what tcnn's
 * kernel_grid keeps when the input needs a gradient; handed to dns_encode_bwd it replaces the second gather of
 * the 8 corners per level by a streaming dot product. */
int dns_encode_fwd(const float* in, const double* bound, uint32_t P, uint32_t n_bins,
                   const float* table, const DnsGridMeta* meta,
                   float* x_out, float* pe_out, uint32_t ld_pe, float* grid_out, uint32_t ld_grid,
                   float* dy_dx, void* stream);

/* ---- split rows: the activation format between the encoders and the MLP kernels (ABI v9) ---------------------------
 * Replaces, on the fixed launch sequence of dns_slam_amd/fused_step.py, the fp32 [P, K] rows that tcnn hands from its encodings
 * to its networks (models/decoder.py:45-48 -> :93-94, :123-124).  A row of K values travels as K halfs hi[j] = f16(v[j] 2^e)
 * followed by K halfs lo[j] = f16(v[j] 2^e - hi[j]) plus ONE int32 exponent e per row (e puts max |row| into [2^13, 2^14)):
 * exactly the operand parts the MLP kernels otherwise derive from the fp32 row in every launch that reads it (row maximum,
 * scale, two conversions per value, an LDS transpose) -- the rows of a mapping iteration are read by ~15 launches.  The
 * bytes per row are those of the fp32 row; DNS_SPLIT_HI_ONLY (half-width mode, with DNS_MLP_FP16 consumers: tcnn's own fp16
 * activations, models/decoder.py:58-64,94) writes the hi plane only: half the bytes.
 *   rows: 16-byte aligned, ld halfs per row (ld % 8 == 0); hi plane at columns [0, K), lo plane at [lo_off, lo_off + K)
 *   (lo_off = 0: no lo plane); exps [rows] int32.  The kernels that take the format need K % 16 == 0. */
typedef struct DnsSplitRows {
  const void* rows;
  const int32_t* exps;
  uint32_t ld;
  uint32_t lo_off;
} DnsSplitRows;
#define DNS_SPLIT_HI_ONLY 1u
/* DNS_SPLIT_PLAIN (ABI v12): HALF ROWS -- the row is written as K plain f16 values, no scale, no exponent (xexp may be NULL), no lo
 * plane: tcnn's own activation format (its networks round their fp32 inputs to half precision, models/decoder.py:93-94,123-125),
 * what dns_mlp_fwd_half / dns_mlp_bwd_half read.  160 bytes per [OneBlob | grid] row instead of 320. */
#define DNS_SPLIT_PLAIN 2u
/* dns_encode_fwd with the (OneBlob | grid) row written in the split-row format: xs_out [P, ldxs] halfs (ldxs >= 2 K, or >= K
 * with DNS_SPLIT_HI_ONLY; K = 3 n_bins + 2 n_levels, both parts multiples of 8), xexp [P]; f32_out (NULL = skip) [P, ld32]
 * additionally receives the fp32 row (the streaming dW_in kernel dns_mlp_dwin reads fp32 rows).  x_out, dy_dx, bound as in
 * dns_encode_fwd.  The exponent is scale_exp(max |row|) -- bit for bit what the MLP kernels derive from the fp32 row, so a
 * one-segment network gives IDENTICAL results on either input form. */
int dns_encode_fwd_split(const float* in, const double* bound, uint32_t P, uint32_t n_bins, const float* table,
                         const DnsGridMeta* meta, float* x_out, float* f32_out, uint32_t ld32, void* xs_out, uint32_t ldxs,
                         int32_t* xexp, uint32_t flags, float* dy_dx, void* stream);

/* Backward.  x [P,3] normalised coordinates.  d_pe / d_grid may be NULL.  d_table (+=) [total_rows,F]
 * (NULL = skip), d_x [P,3] (overwritten; NULL = skip) = dL/dx of the NORMALISED coordinate; if
 * bound != NULL it is scaled by 1/(b1-b0) so it is dL/d(world point).  dy_dx: NULL, or what dns_encode_fwd wrote for the
 * same points and table (then the grid part of d_x needs no table access).  ws: 8-byte aligned scratch of
 * dns_encode_bwd_ws_floats(P, meta, flags, queue_cap) floats for the LDS-binned table scatter (NULL = per-corner atomics).
 * flags selects the form of the table scatter (tcnn kernel_grid_backward).  DNS_SCATTER_AUTO: HASHED levels of more than 8192 rows
 * and DENSE levels of at least six 8192-row chunks through pair lists (ABI v10, below: 64-bit fixed-point LDS bins, exact
 * order-independent sums per workgroup), the other levels through the LDS-bin sweep (FLOAT64 bins, ds_add_f64: sums good to ~1e-16
 * of the terms but dependent on their order; dense levels keep a cell's 8 x 2 sums in registers while consecutive points stay in
 * the cell).  Whatever the form, a chunk's sums reach d_table by float atomics, so d_table is not bit-reproducible from run to run.
 * _ATOMIC = one float atomic per corner (tcnn's form; order-dependent fp32 sums); _BINNED = the sweep for every level; _QUEUES =
 * per-chunk queues of {row, w g0, w g1} for every multi-chunk level (rounds 1-3's form for large tables; fixed-point bins); neither
 * uses lists unless DNS_SCATTER_LISTS is added.  queue_cap: 0, or the entry capacity of each queue and hashed list (what does
 * not fit falls back to float atomics) -- same value in both calls.  A NaN / Inf in d_grid gives a non-finite d_table in
 * every form. */
#define DNS_SCATTER_AUTO 0u
#define DNS_SCATTER_ATOMIC 1u
#define DNS_SCATTER_BINNED 2u
#define DNS_SCATTER_QUEUES 3u
#define DNS_SCATTER_MASK 3u
/* | DNS_SCATTER_REPLAY (ABI v9): hashed levels of at most 2^16 rows handled by the LDS-bin form keep the 8 corner rows of every point
 * (eight 16-bit values, written once per call beside the level-major gradient copy: 16 more bytes of workspace per point and
 * level, counted by dns_encode_bwd_ws_floats with the same flags) and the 8 chunk visits of a level replay them instead of
 * hashing the 8 corners again.  Same sums. */
#define DNS_SCATTER_REPLAY 0x10u
/* | DNS_SCATTER_LISTS (ABI v10; implied by _AUTO, may be added to _BINNED / _QUEUES): PAIR LISTS.  Pass 1 hashes each point-level
 * once and appends one 32-bit word {point, x-pair of corners} to the list of the pair's 4096-row chunk (16 bytes per point-level
 * instead of the 8 chunk visits of the sweep or the 192 bytes of the queues; workspace counted by dns_encode_bwd_ws_floats with
 * the same flags), pass 2 gives every lane one entry, re-forms its two rows and weights from the point and adds into the chunk's
 * 64-bit fixed-point LDS bins.  Hashed levels (2^14 .. 2^20 rows): fixed-capacity lists (uniform hash), a fixed number of jobs per
 * list.  Dense levels: the lists fill by where the rays are -- they are sized EXACTLY (a counting sweep, a one-workgroup scan that
 * places every chunk's list inside the level's 8 P-word region, a writing sweep) and cut into jobs of 8192 entries from the actual
 * counts.  P < 2^30. */
#define DNS_SCATTER_LISTS 0x20u
int dns_encode_bwd(const float* x, const double* bound, uint32_t P, uint32_t n_bins,
                   const float* table, const DnsGridMeta* meta,
                   const float* d_pe, uint32_t ld_dpe, const float* d_grid, uint32_t ld_dgrid,
                   float* d_table, float* d_x, const float* dy_dx, float* ws, uint32_t flags, uint32_t queue_cap,
                   void* stream);
uint64_t dns_encode_bwd_ws_floats(uint32_t P, const DnsGridMeta* meta, uint32_t flags, uint32_t queue_cap);

/* Debug / parity: absolute table rows of the 8 corners of every level, [P, n_levels, 8] uint32. */
int dns_hashgrid_indices(const float* x, uint32_t P, const DnsGridMeta* meta, uint32_t* rows, void* stream);

/* ---- bias-free ReLU MLP (tcnn CutlassMLP; decoder.py:58-64,84-90,101-116, mapping.py:737-743) ----
 * params: flat fp32 [n_neurons*n_in | (n_hidden_layers-1)*n_neurons^2 | out_pad*n_neurons], row-major
 * matrices, out_pad = next multiple of 16 of n_out.  n_neurons in {32,64}; n_hidden_layers in {1,2};
 * n_in a multiple of 8 and <= 128; n_out <= 64; x 16-byte aligned with ldx % 4 == 0.
 * Arithmetic: every fp32 operand is split into two f16 parts (power-of-two scaled per matrix / per point) and a product
 * is three v_mfma_f32_32x32x16_f16 with fp32 accumulation -- error below an fp32 fma chain's;
 * DNS_MLP_FP16 keeps the leading part only (tcnn's own precision: fp16 operands, fp32 accumulate).
 * Two-segment input (x2 != NULL): input columns [0, n_in1) are read from x, columns [n_in1, n_in) from
 * x2[row*ldx2 + (col - n_in1)] -- the torch.cat((pe, features), -1) inputs of decoder.py:73,93,123-124 without
 * the copy.  n_in1 % 4 == 0; x2 16-byte aligned, ldx2 % 4 == 0 -- dns_mlp_fwd alone takes an x2 of any 4-byte alignment and any
 * ldx2 >= n_in - n_in1 (a column slice of another matrix, e.g. the latent columns fine[:, 1:] of the [P, 33] rows of the fine
 * decoders: the forward-only frame render builds no packed copy).  x2 == NULL: one segment (ldx2, n_in1 ignored).
 * A workgroup handles 128 consecutive point SLOTS.  row_index (NULL = identity) maps slot -> row of x / x2 / y /
 * dy / d_x / d_x2, -1 = padding slot (computes on zeros, stores nothing).  tile_group (NULL = one net) gives, per
 * 128-slot tile, the weight set: params + tile_group[t]*param_stride (-1 = skip the tile) -- the per-class
 * fine decoders of slams/mapping.py:590-601 without gathering activations. */
#define DNS_MLP_FP16 0x100u   /* flags of dns_mlp_fwd; bit 8 of accumulate_dx of dns_mlp_bwd */
/* DNS_MLP_PREPARED (flags of dns_mlp_fwd, bit 9 of accumulate_dx of dns_mlp_bwd): `params` points to what dns_mlp_prepare wrote
 * for the same (n_in, n_out, n_neurons, n_hidden_layers) -- the scaled, split operand images of the kernels' LDS prologue --
 * instead of to the fp32 matrices: every workgroup then copies its weight set's images in (L2 hits) instead of loading,
 * reducing, splitting and scattering the matrices itself.  Results are bit-identical.  The weights change once per optimiser
 * step and are used by ~10 launches of hundreds of workgroups each; param_stride keeps its meaning (fp32 floats per weight
 * set: it still addresses d_params), the prepared sets are dns_mlp_prepared_floats(...) floats apart.
 * dns_mlp_prepare: params [n_sets, param_stride] -> prepared [n_sets, dns_mlp_prepared_floats] (16-byte aligned). */
#define DNS_MLP_PREPARED 0x200u
/* DNS_MLP_NO_DWIN (bit 10 of accumulate_dx of dns_mlp_bwd): the backward kernel leaves dH_1 in ws as always, but the second,
 * streaming kernel (dW_in = dH_1^T x) is NOT launched: the caller launches it with dns_mlp_dwin -- same x / ws / d_params /
 * slot arguments -- possibly on ANOTHER stream: it is memory-bound and independent of everything that follows in the
 * backward pass except d_params, so it runs beside the next network's (vector-bound) backward kernel (fused_step.MapStep). */
#define DNS_MLP_NO_DWIN 0x400u
/* DNS_MLP_DX_FIRST (bit 11 of accumulate_dx of dns_mlp_bwd, two-segment input only): only d_x -- the gradient of input columns
 * [0, n_in1) -- is produced; d_x2 may be NULL and the products of the second segment's columns are skipped (Decoder.merge: the
 * OneBlob columns carry the pose gradient, the looked-up image code has none, models/decoder.py:70-74). */
#define DNS_MLP_DX_FIRST 0x800u
/* DNS_MLP_LIVE_IN(n) (bits 16-23 of the flags of dns_mlp_fwd / dns_mlp_dwin and of accumulate_dx of dns_mlp_bwd; ABI v9): input
 * columns [n, n_in) are IDENTICALLY ZERO for every row of this call -- the reference's colour / logit networks when no 2-D feature
 * code is attached (slams/mapping.py:553-557 multiplies a zero code: BASELINE configs 1, 2, 4, 5).  The kernels then run as an
 * n-input network on the same parameter tensor (W_in keeps its row stride n_in): the zero columns are not read (x2 needs only
 * n - n_in1 columns), their K-steps are skipped, no d_x / d_x2 is produced for them and their columns of dW_in receive nothing
 * (their exact gradient is zero).  n: a multiple of 8 with n_in1 < n <= n_in.  Same results as the full-width call on rows padded
 * with zeros up to fp32 rounding (W_in's power-of-two operand scale is taken over its live columns). */
#define DNS_MLP_LIVE_IN(n) ((uint32_t)(n) << 16)
/* DNS_MLP_DX_FROM(c) (bits 24-30 of accumulate_dx of dns_mlp_bwd): the input gradient of columns [0, c) has no consumer -- it is
 * neither formed (whole 32-column tiles) nor stored.  The smoothness lattice's coarse network (slams/mapping.py:129-159) needs
 * the hash-grid columns' gradient only: its points carry no pose.  c: a multiple of 4 below n_in. */
#define DNS_MLP_DX_FROM(c) ((uint32_t)(c) << 24)
int dns_mlp_dwin(const float* x, uint32_t ldx, const float* x2, uint32_t ldx2, uint32_t n_in1, uint32_t n_in, uint32_t n_neurons,
                 uint32_t n_hidden_layers, float* d_params, const float* ws, uint32_t n_slots, const int32_t* row_index,
                 const int32_t* tile_group, uint32_t param_stride, uint32_t flags, void* stream);
uint64_t dns_mlp_prepared_floats(uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers);
/* (ABI v11: `flags` = DNS_MLP_LIVE_IN(n) or 0.  With a live width the images are built -- and the blob is laid out:
 * dns_mlp_prepared_floats(n, ...) floats per weight set -- for the n-input network on the same parameter tensor; dns_mlp_fwd /
 * dns_mlp_bwd then take DNS_MLP_PREPARED | DNS_MLP_LIVE_IN(n) together.) */
int dns_mlp_prepare(const float* params, uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers,
                    uint32_t n_sets, uint32_t param_stride, float* prepared, uint32_t flags, void* stream);
int dns_mlp_fwd(const float* x, uint32_t ldx, const float* x2, uint32_t ldx2, uint32_t n_in1,
                const float* params, uint32_t n_in, uint32_t n_out,
                uint32_t n_neurons, uint32_t n_hidden_layers, float* y, uint32_t ldy, uint32_t n_slots,
                const int32_t* row_index, const int32_t* tile_group, uint32_t param_stride,
                float* h_save /* NULL, or [n_hidden_layers, n_slots, n_neurons]: also write the hidden activations (inspection, or
                                 to hand them to dns_mlp_bwd as h_saved; the backward does not NEED them) */,
                uint32_t flags /* 0 or DNS_MLP_FP16 */, void* stream);

/* Backward.  Hidden activations are RECOMPUTED from x, or -- with h_saved = what dns_mlp_fwd wrote to h_save for the same slots,
 * fp32-grade mode with d_params only -- read back (bit-identical results; trades the recompute's vector work for 512 B of traffic
 * per point each way).  One kernel produces d_x, dW_hidden
 * and dW_out and leaves dH_1 in ws; a second, streaming kernel forms dW_in = dH_1^T x.  d_x [rows, lddx] (columns
 * [0, n_in1)) and, with a two-segment input, d_x2 [rows, lddx2] (columns [n_in1, n_in)) are written for valid slots (d_x NULL
 * = skip both); d_params (+=) same layout as params (+ group*param_stride), NULL = skip (no weight-gradient work at all:
 * the tracker's frozen scene).  ws: 16-byte aligned workspace of dns_mlp_bwd_ws_floats(...) floats (needed with d_params).
 * accumulate_dx: bit 0 -> d_x += instead of =, bit 1 -> d_x2 += (several networks reading one input add their input
 * gradients in place instead of through separate buffers and an add); | DNS_MLP_FP16: as in the forward (weight gradients
 * then use two bf16 parts, 16 significant bits). */
int dns_mlp_bwd(const float* x, uint32_t ldx, const float* x2, uint32_t ldx2, uint32_t n_in1,
                const float* dy, uint32_t lddy, const float* params,
                uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers,
                float* d_x, uint32_t lddx, float* d_x2, uint32_t lddx2, float* d_params, float* ws, uint32_t n_slots,
                const int32_t* row_index, const int32_t* tile_group, uint32_t param_stride, const float* h_saved,
                int accumulate_dx, void* stream);
uint64_t dns_mlp_bwd_ws_floats(uint32_t n_slots, uint32_t n_neurons, uint32_t n_hidden_layers);
/* The same two entry points reading their input in the split-row format (above): x [host] describes the rows of input columns
 * [0, n_in1) (or all n_in columns when x2 == NULL), x2 [host] those of columns [n_in1, n_in); n_in, n_in1 multiples of 16.  The
 * operand fragments go from memory straight into the matrix instruction (one 16-byte load per part, lane and K-step).  With
 * DNS_MLP_FP16 only the hi planes are read (lo_off may be 0).  Everything else as in dns_mlp_fwd / dns_mlp_bwd, except:
 * dns_mlp_bwd_split never launches the streaming dW_in kernel (DNS_MLP_NO_DWIN is implied): the caller runs dns_mlp_dwin on fp32
 * rows or dns_mlp_dwin_split on the same split rows. */
int dns_mlp_fwd_split(const DnsSplitRows* x, const DnsSplitRows* x2, uint32_t n_in1, const float* params, uint32_t n_in,
                      uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers, float* y, uint32_t ldy, uint32_t n_slots,
                      const int32_t* row_index, const int32_t* tile_group, uint32_t param_stride, uint32_t flags, void* stream);
int dns_mlp_bwd_split(const DnsSplitRows* x, const DnsSplitRows* x2, uint32_t n_in1, const float* dy, uint32_t lddy,
                      const float* params, uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers,
                      float* d_x, uint32_t lddx, float* d_x2, uint32_t lddx2, float* d_params, float* ws, uint32_t n_slots,
                      const int32_t* row_index, const int32_t* tile_group, uint32_t param_stride, int accumulate_dx,
                      void* stream);

/* ---- the same network in tcnn's OWN arithmetic: HALF ROWS (ABI v12) -------------------------------------------------------
 * Replaces tcnn.Network{CutlassMLP} as the reference runs it (models/decoder.py:58-64,84-90,101-116 construct half-precision
 * networks; :94 `.float()`s their output): f16 activations, f16 weight operands, fp32 accumulation in v_mfma_f32_32x32x16_f16, a
 * STATIC loss scale on the gradients (tcnn's default: 128).  BASELINE configs[4].  No row maxima, no per-point exponents, no hi / lo
 * parts: x / x2 are plain f16 rows (DNS_SPLIT_PLAIN: dns_encode_fwd_split, dns_feature_block_split), [rows, ldx] halfs, 16-byte
 * aligned, ldx % 8 == 0; n_in (the live width) % 16 == 0, n_in1 % 8 == 0; params / d_params: the fp32 master weights in the layout
 * of dns_mlp_fwd (rounded to f16 when a workgroup builds its LDS images -- ONE image per matrix, read row-wise for W and with
 * ds_read_b64_tr_b16 for W^T).  y, dy, d_x, d_x2 stay fp32 rows (the compositing / loss / encoder-backward kernels' format).
 * row_index / tile_group / param_stride as in dns_mlp_fwd.  flags: DNS_MLP_LIVE_IN(n) (n % 16 == 0) or 0.
 * dns_mlp_bwd_half: ONE kernel produces d_x (/ d_x2) and ALL weight gradients, dW_in included (no workspace, no dns_mlp_dwin);
 * hidden activations are recomputed.  dY is multiplied by loss_scale before it is rounded to f16, every hidden gradient is f16
 * at that scale, d_x and d_params receive 1 / loss_scale times the fp32 sums.  accumulate_dx: bits 0 / 1 (d_x / d_x2 +=),
 * DNS_MLP_DX_FIRST, DNS_MLP_LIVE_IN(n), DNS_MLP_DX_FROM(c) as in dns_mlp_bwd. */
int dns_mlp_fwd_half(const void* x, uint32_t ldx, const void* x2, uint32_t ldx2, uint32_t n_in1, const float* params, uint32_t n_in,
                     uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers, float* y, uint32_t ldy, uint32_t n_slots,
                     const int32_t* row_index, const int32_t* tile_group, uint32_t param_stride, uint32_t flags, void* stream);
int dns_mlp_bwd_half(const void* x, uint32_t ldx, const void* x2, uint32_t ldx2, uint32_t n_in1, const float* dy, uint32_t lddy,
                     const float* params, uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers, float* d_x,
                     uint32_t lddx, float* d_x2, uint32_t lddx2, float* d_params, uint32_t n_slots, const int32_t* row_index,
                     const int32_t* tile_group, uint32_t param_stride, int accumulate_dx, float loss_scale, void* stream);

/* ---- occupancy compositing (raw2nerf_color, utils/common.py:506-537, + the logit composite of
 * slams/mapping.py:633 / slams/tracking.py:212) ----------------------------------------------
 * raw [N,S,4] (rgb, occ), z [N,S], logits [N,S,C] (C may be 0).  Outputs depth,var [N], rgb [N,3],
 * weights [N,S], sem [N,C]. */
int dns_composite_fwd(const float* raw, const float* z, const float* logits, uint32_t N, uint32_t S, uint32_t C,
                      float* depth, float* var, float* rgb, float* weights, float* sem, void* stream);
/* d_weights may be NULL.  d_raw [N,S,4], d_logits [N,S,C] overwritten. */
int dns_composite_bwd(const float* raw, const float* z, const float* logits, uint32_t N, uint32_t S, uint32_t C,
                      const float* d_depth, const float* d_var, const float* d_rgb, const float* d_weights,
                      const float* d_sem, float* d_raw, float* d_logits, void* stream);

/* The same pair with the colour network's output activation folded in (ABI v9): DNS_COMPOSITE_RGB_LOGITS -- raw[..., 0:3] holds
 * the colour network's LOGITS; the kernels apply sigmoid (models/decoder.py:124) on the fly, and the backward's d_raw[..., 0:3] is
 * the gradient w.r.t. those logits (d colour * s (1 - s)), i.e. directly the colour network's output gradient: no separate
 * sigmoid pass over [P,4] forward, none backward. */
#define DNS_COMPOSITE_RGB_LOGITS 1u
int dns_composite_fwd_ex(const float* raw, const float* z, const float* logits, uint32_t N, uint32_t S, uint32_t C, float* depth,
                         float* var, float* rgb, float* weights, float* sem, uint32_t flags, void* stream);
int dns_composite_bwd_ex(const float* raw, const float* z, const float* logits, uint32_t N, uint32_t S, uint32_t C,
                         const float* d_depth, const float* d_var, const float* d_rgb, const float* d_weights, const float* d_sem,
                         float* d_raw, float* d_logits, uint32_t flags, void* stream);

/* ---- fused loss reductions --------------------------------------------------------------------
 * Mapper: photometric / depth / label / latent losses (slams/mapping.py:110-126) + get_opacity_loss
 * (utils/common.py:769-802) and their weighted sum (mapping.py:906-907); tracker = 1: the three masked losses of
 * slams/tracking.py:85-96 (depth term divided by sqrt(var + 1e-10)).
 * lambdas [host, 8 floats] = lambda_p, lambda_d, lambda_l, lambda_lt, lambda_fs, lambda_opacity, truncation, sigma.
 * Rays: pred_color [N,3], pred_depth [N], pred_var [N] (tracker), pred_logits [N,C], gt_color [N,3], gt_depth [N],
 * gt_label [N] int64, valid [N] uint8 (NULL = all rays count).  Points (mapper): fine, coarse [N*S, L], z [N,S].
 * Three calls: dns_loss_sums fills sums[0..15] (numerators and counts; multi-GPU callers all-reduce those 16 here;
 * the buffer must hold DNS_LOSS_SUMS_FLOATS floats, the rest is reduction workspace),
 * dns_loss_finalize turns it into out[16] = {p, d, l, lt, fs, op, total, -, coefficients...},
 * dns_loss_bwd writes d(total * g_total)/d(inputs): d_color, d_depth, d_var (tracker; may be NULL), d_logits,
 * d_fine, d_coarse (overwritten; both NULL in mapper mode: the ray part only, see dns_loss_bwd_points).  ldd_fine: row stride of d_fine in floats (0 = L, contiguous) -- lets the caller place the
 * fine decoder's loss gradient straight into a wider row that later kernels add to (fused_step.MapStep). */
#define DNS_LOSS_SUMS_FLOATS (32 + 5 * 1024)
/* dns_loss_rays (ABI v10) = dns_loss_sums + dns_loss_finalize + the RAY part of dns_loss_bwd where nothing has to happen between the
 * sums and the coefficients (one rank, no all-reduce): the point pass's partial sums (mapper) and ONE single-workgroup kernel that
 * walks the rays, reduces in a fixed order (no atomics: sums[0..15] are reproducible), finalises out[16] and writes d_color,
 * d_depth, d_var (tracker; may be NULL), d_logits.  1 <= N <= 2^20.  The mapper's point gradients follow with dns_loss_bwd_points.
 * For SMALL ray counts (the tracker's 500-1000 rays: one launch instead of four); at 4096 rays the single workgroup takes 63 us
 * where the three launches take 22. */
int dns_loss_rays(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, int tracker,
                  const float* pred_color, const float* pred_depth, const float* pred_var, const float* pred_logits,
                  const float* gt_color, const float* gt_depth, const int64_t* gt_label, const uint8_t* valid,
                  const float* fine, const float* coarse, const float* z, float* sums, float* out, const float* g_total,
                  float* d_color, float* d_depth, float* d_var, float* d_logits, void* stream);
/* dns_loss_finalize_bwd (ABI v10) = dns_loss_finalize + the RAY part of dns_loss_bwd in one launch: every workgroup of the rays'
 * backward derives the terms / coefficients from sums[0..15] itself, workgroup 0 writes out[16] for the kernels that follow
 * (dns_loss_bwd_points, dns_keep_best).  Works behind an all-reduce of the sums too.  N >= 1. */
int dns_loss_finalize_bwd(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, int tracker,
                          const float* sums, float* out, const float* g_total, const float* pred_color,
                          const float* pred_depth, const float* pred_var, const float* pred_logits, const float* gt_color,
                          const float* gt_depth, const int64_t* gt_label, const uint8_t* valid, float* d_color,
                          float* d_depth, float* d_var, float* d_logits, void* stream);
int dns_loss_sums(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, int tracker,
                  const float* pred_color, const float* pred_depth, const float* pred_var, const float* pred_logits,
                  const float* gt_color, const float* gt_depth, const int64_t* gt_label, const uint8_t* valid,
                  const float* fine, const float* coarse, const float* z, float* sums, void* stream);
int dns_loss_finalize(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, int tracker,
                      const float* sums, float* out, void* stream);
int dns_loss_bwd(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, int tracker,
                 const float* out, const float* g_total, const float* pred_color, const float* pred_depth,
                 const float* pred_var, const float* pred_logits, const float* gt_color, const float* gt_depth,
                 const int64_t* gt_label, const uint8_t* valid, const float* fine, const float* coarse, const float* z,
                 float* d_color, float* d_depth, float* d_var, float* d_logits, float* d_fine, float* d_coarse,
                 uint32_t ldd_fine, void* stream);

/* The point part of dns_loss_bwd alone (dns_loss_bwd with d_fine = d_coarse = NULL runs the ray part alone), with the
 * compositing's gradient of the occupancy logit added in: d_fine[p, 0] += d_occ[p * ld_occ] (d_occ NULL = nothing) -- the occupancy
 * is column 0 of the fine latents (slams/mapping.py:626-627), so the sum the reference's autograd forms needs no
 * read-modify-write pass over a strided column.  Call order: dns_loss_bwd (rays) -> dns_composite_bwd -> this. */
int dns_loss_bwd_points(const float* lambdas, uint32_t N, uint32_t S, uint32_t C, uint32_t L, const float* out,
                        const float* g_total, const float* gt_depth, const uint8_t* valid, const float* fine, const float* coarse,
                        const float* z, float* d_fine, float* d_coarse, uint32_t ldd_fine, const float* d_occ, uint32_t ld_occ,
                        void* stream);

/* ---- fused Adam --------------------------------------------------------------------------------
 * torch.optim.Adam.step with default betas / eps, no weight decay, no amsgrad (reference slams/mapping.py:464,910,
 * slams/tracking.py:120-124,339) over up to 32 parameter tensors in one launch.  tensors [host]: per tensor the
 * parameter, its gradient (NULL = skip), first / second moment buffers, element count and learning rate.
 * state: 3 device floats {step count, 1-beta1^t, 1-beta2^t}; zero it when the optimiser is created ("fresh moments
 * every optimize() call", slams/mapping.py:464); each call advances the count on the device. */
typedef struct DnsAdamTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint64_t n;
  float lr;
} DnsAdamTensor;
int dns_adam_step(const DnsAdamTensor* tensors, uint32_t n_tensors, float beta1, float beta2, float eps,
                  float* state, void* stream);

/* ---- the tracker's optimise iteration as ONE kernel + a pose kernel (ABI v11) ---------------------------------------
 * Replaces the per-iteration body of Tracker.run (reference slams/tracking.py:313-340: get_target_samples :128-186,
 * renderer :188-214, the three masked losses :85-96, backward to the pose, Adam on (quat, T), keep-best :326-335) for the
 * frozen scene.  A 256-thread workgroup owns 2 (S > 32) or 4 rays from the pixel draw to their share of the pose gradient:
 * sampling, OneBlob + hash-grid encoding, coarse / colour / logit networks forward, compositing, losses, compositing and
 * network backward, encoding backward; a one-workgroup pose kernel sums the workgroups' partial results, forms the loss,
 * keeps the best pose, runs the quaternion chain rule and the Adam update.  Two launches per iteration.
 *   The draws of ALL n_iters iterations of a frame are made up front: pix [n_iters, n_rays] int64 (index into the window
 *   [H0,H1) x [W0,W1)), t_surf / t_zero [n_iters, n_surface], dmax [n_iters] (bits of max(gt_depth > 0) over each draw;
 *   dns_track_fused_begin computes it and forces the mid sample of every t_surf row in one launch: neither depends on the
 *   pose); t_uniform [n_uniform] is shared.  iter [1] uint32: device counter of the frame's iterations (zero it per frame):
 *   launch k reads draws min(iter, n_iters - 1) and the pose kernel advances it -- every launch of a frame has the SAME
 *   arguments, so one captured iteration replays n_iters times.
 *   quat [4], trans [3]: the pose, updated in place.  adam_m / adam_v [8] (quat at 0, trans at 4), adam_state [3] (step count,
 *   1 - beta1^t, 1 - beta2^t): zero them per frame.  best_loss [1] (+inf per frame), best_cam [7].
 *   w_coarse / w_color / w_logit: dns_mlp_prepare images of the three networks (inputs 3 n_bins + 2 n_levels -> hidden + 1;
 *   3 n_bins + n_feat -> 3 and -> n_class).  code [n_rays * S, code_dim] or NULL: the 2-D feature code of every sample.
 *   n_feat = hidden + code_dim; WITHOUT a code either n_feat = the networks' full second-segment width (zero code columns, images
 *   of the full networks) or n_feat = hidden with images prepared with DNS_MLP_LIVE_IN(3 n_bins + hidden): no feature block is
 *   built then, the colour / logit networks read the latent out of the coarse network's output rows.
 *   ws: dns_track_fused_ws_floats(a) floats, 256-byte aligned (rows the workgroups hand from phase to phase).
 *   out [8]: loss terms p, d, l, total, n_valid of THIS iteration (before the update); g_quat [4], g_trans [3]: its gradient.
 * Supported: S <= 64, networks 64 x 2 or 32 x 1, 64 < 3 n_bins + 2 n_levels <= 96, 96 < 3 n_bins + n_feat <= 128; otherwise
 * DNS_E_ARG (callers fall back to the launch sequence of the single entry points). */
typedef struct DnsTrackFused {
  const float* color;
  const float* depth;
  const float* label;
  int32_t H, W, H0, H1, W0, W1;
  const double* cam;                 /* fx fy cx cy */
  const double* bound;               /* [3][2] */
  const int64_t* pix;
  const float* t_uniform;
  const float* t_surf;
  const float* t_zero;
  const uint32_t* dmax;
  uint32_t* iter;
  uint32_t n_iters;
  uint32_t n_uniform, n_surface, n_rays;
  float* quat;
  float* trans;
  const float* table;
  const DnsGridMeta* meta;
  uint32_t n_bins;
  const float* w_coarse;
  const float* w_color;
  const float* w_logit;
  uint32_t n_neurons, n_hidden_layers, hidden, n_feat, n_class;
  const float* code;
  uint32_t code_dim;
  float lambda_p, lambda_d, lambda_l;
  float* ws;
  float* adam_m;
  float* adam_v;
  float* adam_state;
  float lr_quat, lr_trans, beta1, beta2, eps;
  float* best_loss;
  float* best_cam;
  float* out;
  float* g_quat;
  float* g_trans;
  /* ---- the stem form (ABI v25): maps != NULL runs the 2-D branch of a stem-trained map INSIDE the iteration (feature_matching +
   * Decoder.merge on the iteration's points, slams/tracking.py:162-165; Merge frozen like the scene).  maps NULL: as before.
   *   maps [n_views, map_h, map_w, map_c] channels-last half-resolution stem maps (16-byte aligned, map_c % 4 == 0);
   *   w2c [n_views, 16], origin [n_views, 3]: the reference views; bit r of follow_mask: view r takes w2c = inverse(c2w(quat,
   *   trans)) and origin = trans of the pose as it stands when the iteration starts (slams/tracking.py:316-319) instead.
   *   w_merge: dns_mlp_prepare image of Merge (merge_in = 3 merge_bins + map_c inputs in (64, 128], % 8 == 0; merge_out outputs
   *   == hidden == 32), merge_bound [3][2].  n_views in [1, 8].  n_feat >= 2 hidden; code must be NULL. */
  const float* maps;
  const float* w2c;
  const float* origin;
  uint32_t follow_mask;
  const float* w_merge;
  uint32_t merge_in, merge_out, merge_bins;
  const double* merge_bound;
  uint32_t n_views, map_c;
  int32_t map_h, map_w;
} DnsTrackFused;
uint64_t dns_track_fused_args_bytes(void);   /* sizeof(DnsTrackFused) as the library was built: callers check their own layout */
uint64_t dns_track_fused_ws_floats(const DnsTrackFused* a);
int dns_track_fused_begin(const int64_t* pix_all, uint32_t n_rays, uint32_t n_iters, const float* depth, int W, int H0, int W0,
                          int W1, float* t_surf_all, uint32_t n_surface, uint32_t* dmax_all, void* stream);
int dns_track_fused_iter(const DnsTrackFused* a, void* stream);

/* ---- small fused helpers of the mapping iteration ----------------------------------------------
 * Total-variation smoothness of coarse[:, 0] on a lattice of nx x n x n points (x-major; nx = n: the n^3 cube of
 * slams/mapping.py:151-157), divided by sample_points^3.  lat [nx*n*n, ld] (the coarse latents, occupancy in column 0).
 * halo != 0: the last x-plane belongs to the next slab of a lattice cut along x (one slab per GPU) -- it closes the
 * x-differences of plane nx-2 and contributes no y / z differences, so the slabs' values sum to the cube's value.
 * out: 1 float.  Backward: d_lat [nx*n*n, ld] = g[0] * d loss / d lat (column 0; the other columns are zeroed). */
int dns_tv_fwd(const float* lat, uint32_t ld, uint32_t nx, uint32_t n, int halo, uint32_t sample_points, float* out,
               void* stream);
int dns_tv_bwd(const float* lat, uint32_t ld, uint32_t nx, uint32_t n, int halo, uint32_t sample_points, const float* g,
               float* d_lat, void* stream);

/* Counting sort of P points by weight-set id into 128-slot tiles for dns_mlp_fwd/bwd (the per-class dispatch of
 * Mapper.fine_fn, slams/mapping.py:590-601).  slot_of_point [P] int64 (negative = no network).  Outputs row_index
 * [n_slots] (-1 = padding), tile_group [n_slots/128] (-1 = skip; groups with fewer than min_count points are
 * skipped, mapping.py:597).  n_slots: multiple of 128, >= P + 127 * n_groups.  ws: 512 uint32 of scratch. */
int dns_group_slots(const int64_t* slot_of_point, uint32_t P, uint32_t n_groups, uint32_t min_count, uint32_t n_slots,
                    uint32_t* ws, int32_t* row_index, int32_t* tile_group, void* stream);

/* Device-side error word.  Kernels that consume DEVICE counters (the cursors of dns_group_slots: a stale or corrupted cursor
 * would otherwise be an out-of-bounds store, not an error code) clamp to their buffers' capacity and, when they had to, set a
 * bit of a sticky per-device word in pinned host memory (allocated by dns_init(); never device memory).  Every entry point
 * polls the word after its launches -- no synchronisation: the bit shows up once the faulting kernel has run -- and from
 * then on returns DNS_E_LAUNCH with the cause in dns_last_error() until the word is cleared.
 *   dns_device_error(0) -> the word (0 = none), dns_device_error(1) -> the word, then cleared.
 *   bit 0: dns_group_slots / dns_group_scatter: a group's cursor ran past n_slots
 * dns_group_scatter is the scatter step of dns_group_slots alone, on caller-supplied cursors [n_groups] (uint32, the first
 * free slot of every group; advanced): the hardening test drives it with a deliberately stale cursor. */
int dns_device_error(int clear);
int dns_group_scatter(const int64_t* slot_of_point, uint32_t P, uint32_t n_groups, uint32_t* cursor, uint32_t n_slots,
                      int32_t* row_index, void* stream);

/* ---- glue of one mapping iteration as single launches (csrc/step.hip) ---------------------------
 * Each replaces a handful of elementwise torch ops of the reference's iteration; used by dns_slam_amd/fused_step.py.
 * dns_class_slots: slot_of_point[p] = lut[label of p] (-1 when the label is outside [0, n_lut)); the label of point p is
 *   labels[p mod N] when tiled (the reference's gt_label.repeat(1, S) layout, slams/mapping.py:613), else labels[p / S].
 * dns_feature_block: feat[p, 0:hidden] = fine[p, 1:1+hidden], feat[p, hidden:hidden+C] = code[p, :] * trunc(p) with
 *   trunc = (1 - [z < 0.95 d]) (1 - [z > 1.05 d]) [d > 0], d = gt_depth[p / S] (slams/mapping.py:553-556; code NULL = zeros),
 *   and raw[p, 3] = fine[p, 0] (raw [P,4], NULL = skip) -- the colour / logit networks' feature input (models/decoder.py:123)
 *   and the occupancy column of the compositing input (slams/mapping.py:627).  hidden, C multiples of 4; feat, code 16-byte aligned.
 * dns_rgb_sigmoid: raw[p, 0:3] = sigmoid(raw[p, 0:3]) in place (models/decoder.py:124), column 3 untouched.
 * dns_raw_bwd: the backward of both: d_col[p, 0:3] = d_raw[p, 0:3] s (1 - s) with s = raw[p, 0:3], d_col[p, 3] = 0, and
 *   d_occ[p * ld_occ] = (accumulate ? += : =) d_raw[p, 3].
 * dns_lattice_points: normalised coordinates of the n^3 smoothness lattice (slams/mapping.py:133-143 as one float64 affine
 *   map): pts[i,j,k] = float(mar + r6[0:3] * off + r6[3:6] * vox + (i,j,k) * vox); consts9 [host, 9 doubles] = vox, off, mar;
 *   r6 [device, 6 floats] = the offset and jitter draws.  order (NULL = x-major): output row m holds lattice element order[m];
 *   count (0 = n^3): the number of rows / entries of order -- a rank's slab of x-planes of the ONE lattice in union-batch mode
 *   (x-major index i n^2 + j n + k) -- a Morton order of the elements makes the hash-grid gather of the lattice 2.3x faster
 *   (neighbouring rows share table lines: 112 -> 49 us at 63^3), the caller maps the network's output back for the TV kernel. */
int dns_class_slots(const int64_t* labels, uint32_t N, uint32_t S, int tiled, const int64_t* lut, uint32_t n_lut,
                    int64_t* slot_of_point, void* stream);
int dns_feature_block(const float* fine, uint32_t ld_fine, uint32_t hidden, const float* code, uint32_t C, const float* z,
                      const float* gt_depth, uint32_t N, uint32_t S, float* feat, uint32_t ld_feat, float* raw, void* stream);
/* dns_feature_block with the block written in the split-row format (above; ABI v9): xs_out [P, ldxs] halfs (hidden + C values
 * per row), xexp [P] (xs_out NULL: the fp32 block only); feat (NULL = skip) receives the fp32 block.  n_ref > 1: code is [n_frames][n_ref]
 * [pts_per_frame][C] and the n_ref slabs of a point are AVERAGED before the truncation mask -- the mean over the reference frames
 * of Decoder.merge's latents (models/decoder.py:76, utils/common.py:677).  max(hidden, C) / 4 must be a power of two <= 16. */
int dns_feature_block_split(const float* fine, uint32_t ld_fine, uint32_t hidden, const float* code, uint32_t C, uint32_t n_ref,
                            uint32_t pts_per_frame, const float* z, const float* gt_depth, uint32_t N, uint32_t S, float* feat,
                            uint32_t ld_feat, void* xs_out, uint32_t ldxs, int32_t* xexp, uint32_t flags, float* raw, void* stream);
int dns_rgb_sigmoid(float* raw, uint32_t P, void* stream);
int dns_raw_bwd(const float* d_raw, const float* raw, uint32_t P, float* d_col, float* d_occ, uint32_t ld_occ, int accumulate,
                void* stream);
int dns_lattice_points(const float* r6, const double* consts9, uint32_t n, const int32_t* order, uint32_t count, float* pts,
                       void* stream);
/* dns_draw_finish: the index arithmetic behind one iteration's pixel draws for all K frames (select_uv + select_by_class,
 * utils/common.py:274,313-328) plus what follows from the drawn pixels alone.  The RANDOM NUMBERS come from the caller's
 * generator: i1 [K, n1] int64 uniform picks in [0, HW), u [K, n2] float64 in [0, 1).  Per frame f: pix[f, 0:n1] = i1[f],
 * pix[f, n1 + s] = sorted_flat[start_flat[f, s] + min(int64(u[f, s] * count_f64[f, s]), count_m1[f, s])] (sorted_flat [K * HW]:
 * every frame's pixel indices ordered by class; start_flat already holds the frame's offset f * HW), labels[f, r] =
 * int64(label[f, pix[f, r]]), dmax[f] = bit pattern of max(0, max_r depth[f, pix[f, r]]) -- the form dns_raygen_sample takes
 * with depth_max_given = 1.  pix, labels [K * (n1 + n2)] int64; depth, label [K, HW] fp32. */
int dns_draw_finish(const int64_t* i1, const double* u, const double* count_f64, const int64_t* count_m1,
                    const int64_t* start_flat, const int64_t* sorted_flat, const float* depth, const float* label,
                    uint32_t n_frames, uint32_t n1, uint32_t n2, uint32_t HW, int64_t* pix, int64_t* labels, uint32_t* dmax,
                    void* stream);
/* Tracker glue (slams/tracking.py:171-172, 326-335; utils/common.py:572-574), used by fused_step.TrackStep:
 * dns_track_mask: valid[n] = gt_depth[n] > min_depth && inside[n] (uint8).
 * dns_keep_best: if (loss[0] < best_loss[0]) { best_loss[0] = loss[0]; best_cam[0:7] = (quat[0:4] | trans[0:3]) } -- device-side
 *   keep-best-pose of the tracking loop, no host read of the loss (a NaN loss keeps the old best).
 * dns_force_half: t[idx] = 0.5 unless some t[i] == 0.5 already (the forced mid-sample of sample_along_rays' surface draws). */
int dns_track_mask(const float* gt_depth, const uint8_t* inside, uint32_t N, float min_depth, uint8_t* valid, void* stream);
int dns_keep_best(const float* loss, const float* quat, const float* trans, float* best_loss, float* best_cam, void* stream);
int dns_force_half(float* t, uint32_t n, uint32_t idx, void* stream);

/* ---- 2-D feature lookup (feature_matching / feature_searching, utils/common.py:632-673) --------
 * pts [P,3] world points, w2c [R,16] row-major world->camera of the R reference frames, K [host, 9 floats] intrinsics,
 * feat [R,h,w,C] stem feature maps, CHANNELS LAST.  code [R,P,C] = the bilinear (align_corners) value of the map at
 * the rounded projected full-resolution pixel, zero where the projection is invalid; mask [R,P] uint8 (NULL = skip). */
int dns_feature_gather(const float* pts, const float* w2c, const float* K, const float* feat, uint32_t R, uint32_t P,
                       uint32_t C, int h, int w, int H, int W, float* code, uint8_t* mask, void* stream);

/* The same lookup for the K target frames of one optimise iteration in ONE launch (slams/mapping.py:532-551 per target frame,
 * slams/tracking.py:162-165; ABI v9): reference rr = f R + r (R views per frame) looks at the points of frame f: pts
 * [n_frames, pts_per_frame, 3], w2c [n_frames R, 16], feat [n_frames R, h, w, C] channels last.  code row (rr, p) starts at
 * code + (rr pts_per_frame + p) ld_code -- e.g. column 3 n_bins of the Merge network's input rows -- and rel_out (NULL = skip)
 * [n_frames R, pts_per_frame, 3] receives pts - origin[rr] (refer_p, utils/common.py:675), origin [n_frames R, 3].
 * dns_refer_poses: the w2c / origin of those views: src[rr] >= 0 takes target frame src[rr]'s pose as it stands in the optimiser
 * (quat [K,4] (w,x,y,z), trans [K,3]; get_rotation_from_quad, detached: slams/mapping.py:537-543), src[rr] < 0 the stored pose
 * fixed_c2w[rr] [16] (:545); w2c = its inverse (torch.inverse, :547).
 * dns_merge_dy: backward of (mean over the R views, truncation mask) -- d_lat [n_frames, R, pts_per_frame, C] = d_code[p] *
 * trunc(p) / R for every view (models/decoder.py:76, slams/mapping.py:553-557); d_code [P, ld_dcode] (the first C columns of each
 * row) is CLEARED afterwards: the colour / logit networks add their input gradients into it every iteration.
 * dns_add_ref_sum: d_pts [P,3] += sum over the R views of d_rel [n_frames, R, pts_per_frame, 3] (the points' share of Merge's
 * gradient, through refer_p = pts - refer_o). */
int dns_feature_gather_frames(const float* pts, const float* w2c, const float* origin, const float* K, const float* feat,
                              uint32_t n_frames, uint32_t R, uint32_t pts_per_frame, uint32_t C, int h, int w, int H, int W,
                              float* code, uint32_t ld_code, float* rel_out, void* stream);
int dns_refer_poses(const float* quat, const float* trans, const int32_t* src, const float* fixed_c2w, uint32_t n, float* w2c,
                    float* origin, void* stream);
int dns_merge_dy(float* d_code, uint32_t ld_dcode, uint32_t C, uint32_t R, uint32_t pts_per_frame, const float* z,
                 const float* gt_depth, uint32_t N, uint32_t S, float* d_lat, void* stream);
int dns_add_ref_sum(const float* d_rel, uint32_t R, uint32_t pts_per_frame, uint32_t P, float* d_pts, void* stream);

/* ---- mesh extraction (Mesher.get_mesh, slams/meshing.py:562-784; csrc/mesh.hip; ABI v13) ------------------------------
 * Marching cubes (replaces skimage.measure.marching_cubes, meshing.py:668-688) on a dense volume vol [nx, ny, nz] fp32, C order,
 * vol[i,j,k] the value at origin + (i,j,k) * spacing.  A corner is inside iff v > level.  One vertex per grid edge whose ends
 * straddle the level, at p0 + t (p1 - p0), t = (level - v0) / (v1 - v0) (fp32 t, fp64 positions, stored fp32); vertices are
 * ordered by the edge index 3 * (C-order index of the edge's lower end) + axis.  Faces int32 [F,3], ordered by cube (C order of
 * its lowest corner), then table order (csrc/mc_table.hpp, generated by tools/gen_mc_table.py), wound so that the right-hand
 * normal points from inside (high values) to outside (skimage's gradient_direction='descent').  Grids of >= 2^31 edges and
 * non-finite origin / spacing are refused.
 *   dns_mc_ws_bytes: bytes of workspace for an nx x ny x nz grid (0: refused size).
 *   dns_mc_count: the counts and their scan into ws; totals [2] uint64 (device) = (V, F).  The caller reads totals back to size
 *     the outputs.
 *   dns_mc_emit: with the ws of dns_mc_count on the same volume and level: verts [v_cap, 3], faces [f_cap, 3]; nothing is
 *     written past either capacity.  origin, spacing: [host] 3 doubles each. */
uint64_t dns_mc_ws_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int dns_mc_count(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void* ws, uint64_t* totals, void* stream);
int dns_mc_emit(const float* vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const double* origin, const double* spacing,
                const void* ws, float* verts, uint64_t v_cap, int32_t* faces, uint64_t f_cap, void* stream);

/* Keyframe projection of P world points pts [P,3] into K keyframes: w2c [K,16] row-major (torch.inverse(est_c2w), fp32),
 * labels [K,H,W] fp32 (gt_label), max_depth [K] (max of each keyframe's gt_depth), intr [host] (fx, fy, cx, cy).  The projection
 * of both reference loops: cam = w2c @ [p,1], x *= -1, uv = K cam, z = cam_z + 1e-8, uv /= z; keyframe k sees p iff 0 < u < W,
 * 0 < v < H, z < 0.
 *   label [P] fp32: get_2d_feature's label_pts (meshing.py:313-373): the label at the rounded (half to even), clamped pixel of the
 *     LAST keyframe that sees p; 0 if none does.
 *   seen [P] uint8: point_masks' seen mask without the depth test (meshing.py:203-274, depth_test False): some keyframe sees p
 *     and -cam_z < 1.2 max_depth[k]. */
int dns_keyframe_project(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* labels, const float* max_depth,
                         int H, int W, const float* intr, float* label, uint8_t* seen, void* stream);

/* ---- mesh components (mesh.split(only_watertight=False) of slams/meshing.py:721-733; csrc/mesh_cc.hip; ABI v14) ----------
 * Connected components of the faces of a triangle list faces [F,3] int32 over verts [V,3] fp32, under trimesh's face_adjacency:
 * of the 3F undirected edges (min(a,b), max(a,b)), a key that occurs exactly twice joins the two faces that hold it (nothing if
 * both occurrences are in one face); a key that occurs once (boundary) or three or more times (non-manifold) joins nothing, and
 * neither does a shared vertex.  Any triangle list is accepted, not only dns_mc_emit's.
 *   dns_mesh_cc_ws_bytes: bytes of workspace for F faces (84 per face: a 4F-slot edge table of 20 bytes per slot and the
 *     union-find parents); 0: refused size (F = 0 needs none, F >= 2^29 is refused).
 *   dns_mesh_components: comp [F] int32 = the smallest face index of the face's component (independent of scheduling);
 *     comp_area [F] float64 = the total area of the face's component, a face's area being 0.5 |(v1 - v0) x (v2 - v0)| in float64
 *     from the fp32 positions (the order of the float64 sum is not fixed: run-to-run differences of a relative F 2^-53);
 *     status [2] uint32 (device): status[0] = the number of components, status[1] = 0, or non-zero if some face holds a vertex
 *     index outside [0, V) -- such an index is never dereferenced, the face joins nothing and has area 0, and the caller must
 *     treat the outputs as invalid.  The caller reads status back.  F = 0: nothing is launched and nothing is written. */
uint64_t dns_mesh_cc_ws_bytes(uint32_t F);
int dns_mesh_components(const float* verts, uint32_t V, const int32_t* faces, uint32_t F, void* ws, int32_t* comp, double* comp_area,
                        uint32_t* status, void* stream);

/* ---- mesh holes (mesh.fill_holes() of slams/meshing.py:770, i.e. trimesh.repair.fill_holes; csrc/mesh_holes.hip; ABI v26) ------
 * Closes the small boundary loops of a triangle list faces [F,3] int32 over V vertices with new faces; no vertex is added and the
 * input faces are not touched.  The definition:
 *   - An undirected edge (min(a,b), max(a,b)) that exactly one of the 3F face edges holds is a boundary edge, directed a -> b as
 *     its face winds it.  A face edge with a == b is not an edge (it is counted in `degenerate`); an edge with three or more
 *     holders is non-manifold (counted) and not boundary.
 *   - A vertex is SIMPLE iff exactly one boundary edge leaves it and exactly one enters it.  A loop is filled iff all its vertices
 *     are simple and it has 3 .. max_edges edges.  Loops through a non-simple vertex -- two holes touching in a vertex,
 *     inconsistent winding, non-manifold neighbourhoods -- are not filled; the boundary vertices that are not simple are counted
 *     in `vertices_skipped`.  (trimesh's outcome there depends on networkx's traversal order.)
 *   - The loop v0 -> v1 -> ... -> v_{L-1} -> v0, v0 its SMALLEST vertex index, gets the fan (v0, v_{i+1}, v_i), i = 1 .. L-2:
 *     L = 3 gives (v0, v2, v1), L = 4 gives (v0, v2, v1), (v0, v3, v2).  Every new face reverses the boundary half-edges it
 *     closes (trimesh's winding rule); the quad's diagonal starts at the loop's smallest vertex (trimesh's depends on networkx's
 *     traversal order).  A lone triangle gets its mirror face, as in trimesh.
 *   - Loops come in ascending order of v0, a loop's faces in fan order.
 * The added block is therefore a function of the mesh alone: the same bits from call to call, and under any permutation of the
 * input faces and any rotation of a face's three indices.
 *   dns_mesh_holes_ws_bytes: bytes of workspace for F faces over V vertices (four words per vertex, the scan's carries and a
 *     4F-slot edge table of 16 bytes per slot); 0: refused size (F = 0 needs none; F >= 2^29 and V >= 2^31 are refused).
 *   dns_mesh_holes_count: everything but the new faces.  max_edges in 3 .. 32.  info [DNS_HOLES_INFO_WORDS] uint32 (device), for
 *     the caller to read back: the counters below, all integer sums and so the same for every call.  A vertex index outside
 *     [0, V) is never dereferenced: it sets info[BAD_INDEX], its face contributes nothing, and the caller must treat the result
 *     as invalid.  info[TABLE_FULL] is 0 (4F slots hold 3F keys; checked rather than assumed).  F = 0: info is zeroed.
 *   dns_mesh_holes_emit: new_faces [info[FACES_ADDED], 3] int32 from the workspace dns_mesh_holes_count left, with the same V and
 *     max_edges.  Every store is below the 3 info[FACES_ADDED] words the caller sized new_faces by.  The caller skips the call
 *     where info[FACES_ADDED] is 0. */
#define DNS_HOLES_INFO_FACES_ADDED 0
#define DNS_HOLES_INFO_LOOPS_FILLED 1
#define DNS_HOLES_INFO_BOUNDARY_EDGES 2        /* before filling */
#define DNS_HOLES_INFO_NONMANIFOLD_EDGES 3
#define DNS_HOLES_INFO_VERTICES_SKIPPED 4
#define DNS_HOLES_INFO_DEGENERATE 5
#define DNS_HOLES_INFO_BAD_INDEX 6
#define DNS_HOLES_INFO_TABLE_FULL 7
#define DNS_HOLES_INFO_WORDS 8
uint64_t dns_mesh_holes_ws_bytes(uint32_t F, uint32_t V);
int dns_mesh_holes_count(const int32_t* faces, uint32_t F, uint32_t V, uint32_t max_edges, void* ws, uint32_t* info, void* stream);
int dns_mesh_holes_emit(const void* ws, uint32_t V, uint32_t max_edges, int32_t* new_faces, void* stream);

/* ---- mesh evaluation (eval_3d.py, cull_mesh.py of the reference; csrc/mesh_eval.hip; ABI v15, v16) ---------------------------
 * dns_nearest_points: for each of N queries query [N,3] fp32 the Euclidean distance dist [N] fp32 to the nearest of M reference
 * points ref [M,3] fp32 and that point's index idx [N] int32 (cKDTree(ref).query(query), eval_3d.py:24-42).  Every pair
 * distance is sqrt of the fp32 sum dx dx + dy dy + dz dz (no contraction); among equal distances the smaller index wins, so
 * both outputs are the same for every call and both methods.  The search runs over a uniform cell grid of the reference cloud
 * (about two cells per point, at most 2^21) in growing Chebyshev rings of cells round the query's cell, at most max_ring
 * (<= 64) of them; the queries that could not stop by then -- in large empty regions or far outside the cloud -- are finished by
 * a tiled all-pairs pass, so every query gets the exact answer wherever it lies.  flags = DNS_NEAREST_BRUTE sends every query
 * through that pass and builds no grid.
 *   dns_nearest_ws_bytes: bytes of workspace for M reference points and N queries (0: refused size, M or N >= 2^31).
 *   status [4] uint32 (device), for the caller to read back: status[0] = 0, or bit 0 / bit 1 set if a reference / query
 *     coordinate is not finite -- the outputs are then invalid (nothing is stored out of range); status[1] = the number of
 *     queries the all-pairs pass finished; status[2] = the number of grid cells.
 * N = 0: nothing is launched.  M = 0 with N > 0 is refused. */
#define DNS_NEAREST_BRUTE 1u
uint64_t dns_nearest_ws_bytes(uint32_t M, uint32_t N);
int dns_nearest_points(const float* ref, uint32_t M, const float* query, uint32_t N, uint32_t max_ring, uint32_t flags, void* ws,
                       float* dist, int32_t* idx, uint32_t* status, void* stream);

/* dns_icp_point_to_point (ABI v16): get_align_transformation of eval_3d.py:45-59 -- open3d's registration_icp with
 * TransformationEstimationPointToPoint -- of the source cloud src [N,3] fp32 onto the target cloud tgt [M,3] fp32, as ONE fixed
 * sequence of launches on the stream with no host read inside.  The cell grid of dns_nearest_points is built once over tgt; then
 * max_iter + 1 passes, pass 0 evaluating init [host, 16 doubles, row-major 4x4; NULL = identity] and pass k the transformation
 * after k updates.  A pass:
 *   - p' = fl32(T p): ((T[i][0] x + T[i][1] y) + T[i][2] z) + T[i][3] in float64 from the float64 T held in the workspace, rounded
 *     once to fp32; always from the ORIGINAL src (open3d transforms its float64 copy of the cloud update by update);
 *   - the nearest target point of p' under the pair distance and tie rule of dns_nearest_points (the smaller index), by the same
 *     ring search, which here also gives up once every unseen target point is provably farther than max_dist; the queries still
 *     undecided after max_ring (<= 64) rings go through the all-pairs pass, so the answer is exact for every max_dist;
 *   - a correspondence exists iff that fp32 distance is <= max_dist (inclusive; open3d's radius search is exclusive);
 *   - the 17 sums n, sum p' [3], sum q [3], sum q p'^T [9, row = q], sum |p' - q|^2 in float64 from the fp32 coordinates: per
 *     wave, per workgroup, one row per workgroup, the rows added by one workgroup in a fixed order.  No floating-point atomics:
 *     `result` is the same bits for every call;
 *   - fitness = n / N, inlier_rmse = sqrt(sum |p' - q|^2 / n) (0 without correspondences).  After pass k > 0 the registration stops
 *     (converged) when |fitness - previous| < rel_fitness and |inlier_rmse - previous| < rel_rmse; it stops after pass max_iter;
 *     otherwise T <- U T with U the rigid motion minimising sum |U p' - q|^2: the proper rotation maximising tr(R^T Sigma)
 *     (Horn's quaternion form, the eigenvector of a symmetric 4x4 by cyclic Jacobi in float64) and t = mean q - R mean p'.
 * After the stop the kernels of the remaining passes return at once.
 *   dns_icp_ws_bytes: bytes of workspace (0: refused size -- an empty cloud, or M or N >= 2^31).
 *   result [DNS_ICP_RESULT_DOUBLES] float64 (device): [0..16) T row-major, [16] fitness, [17] inlier_rmse, [18] n, [19] the number
 *     of updates applied, [20] 1 if the stopping rule ended the registration, [21..38) the 17 sums of the last evaluated pass, which
 *     is the pass that evaluated T.
 *   status [4] uint32 (device): status[0] = the non-finite bits of dns_nearest_points (bit 0 tgt, bit 1 src); status[1] = the
 *     queries the all-pairs pass finished, over all passes; status[2] = the number of grid cells; status[3] = why it stopped:
 *     DNS_ICP_STOP_MAX_ITER, _CONVERGED, _FEW (fewer than 3 correspondences: no update is defined; T stays as it is) or
 *     _NONFINITE (a non-finite coordinate in either cloud: nothing is evaluated, T = init, the other figures 0).
 * An empty cloud, max_dist <= 0 or not finite, a non-finite init, negative criteria and max_iter > DNS_ICP_MAX_ITER are refused.
 * Every store lies inside the sizes passed in, whatever the coordinates and init. */
#define DNS_ICP_RESULT_DOUBLES 38
#define DNS_ICP_MAX_ITER 1000u
#define DNS_ICP_STOP_MAX_ITER 0u
#define DNS_ICP_STOP_CONVERGED 1u
#define DNS_ICP_STOP_FEW 2u
#define DNS_ICP_STOP_NONFINITE 3u
uint64_t dns_icp_ws_bytes(uint32_t M, uint32_t N);
int dns_icp_point_to_point(const float* src, uint32_t N, const float* tgt, uint32_t M, const double* init, float max_dist,
                           uint32_t max_iter, double rel_fitness, double rel_rmse, uint32_t max_ring, void* ws, double* result,
                           uint32_t* status, void* stream);

/* dns_frustum_seen: seen [P] uint8 = some of the K poses w2c [K,16] (row-major world->camera, fp32) sees the point pts [P,3]:
 * check_proj of eval_3d.py:62-88 and the loop of cull_mesh.py:53-74 in fp32: cam = w2c @ [p,1], x = -cam.x, z' = cam.z + 1e-5,
 * u = (fx x + cx cam.z) / z', v = (fy cam.y + cy cam.z) / z'; seen iff 0 <= -z', 0 < u < W and 0 < v < H.  intr [host] (fx, fy,
 * cx, cy).  K = 0 sees nothing. */
int dns_frustum_seen(const float* pts, uint32_t P, const float* w2c, uint32_t K, int H, int W, const float* intr, uint8_t* seen,
                     void* stream);

/* ---- 2-D evaluation (eval_2d.py of the reference; csrc/image_metrics.hip; ABI v17) --------------------------------------------
 * dns_ms_ssim: MS-SSIM and masked MSE of F image pairs pred, gt [F,H,W,3] fp32 (the project's image layout), as ONE fixed
 * sequence of 10 launches on the stream for any F, with no host read and no floating-point atomics: every output is the same
 * bits for every call.  The definition is pytorch_msssim.ms_ssim(data_range=1.0, size_average=True) with its defaults:
 *   - window g[k] = exp(-(k-5)^2 / (2 1.5^2)), k = 0..10, normalised to sum 1 in fp32 (dns_ms_ssim_window returns the eleven
 *     fp32 values the library uses [host]); a separable VALID convolution G* along H, then W, per channel: a level of h x w pixels
 *     has (h-10) x (w-10) outputs;
 *   - per level mu_x = G*X, mu_y = G*Y, s_xx = G*(X X) - mu_x^2, s_yy = G*(Y Y) - mu_y^2, s_xy = G*(X Y) - mu_x mu_y,
 *     cs = (2 s_xy + C2) / (s_xx + s_yy + C2), ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) cs, C1 = 0.01^2, C2 = 0.03^2,
 *     each averaged over the level's outputs per channel;
 *   - between levels a 2x2 average pool, stride 2, zero padding of size % 2 on each axis (padded zeros count in the divisor 4):
 *     output i covers the sources 2i - p and 2i - p + 1, the pooled size is (s + 2 (s % 2) - 2) / 2 + 1;
 *   - ms_ssim = mean over the 3 channels of prod_l relu(term_l)^w_l, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), term = cs at
 *     levels 0..3 and ssim at level 4.
 * The pixels and the pooled pixels are fp32, everything computed from them float64.
 *   depth [F,H,W] fp32 or NULL: mse[f] = the mean of (pred - gt)^2 (the fp32 difference, squared and summed in float64) over the
 *     three channels of the pixels with depth > 0 -- every pixel without depth; n_valid[f] = the number of those pixels; a frame
 *     without one has mse = NaN (as torch's mse_loss of an empty selection).
 *   ms_ssim [F], mse [F] float64; n_valid [F] int64; levels [F,5,3] float64: the per-level, per-channel means before relu.
 *   dns_ms_ssim_ws_bytes: bytes of workspace (the pooled levels and one row of partial sums per workgroup); 0: refused size.
 * min(H, W) <= DNS_MS_SSIM_MIN_SIDE is refused (DNS_E_ARG, nothing launched), as the library asserts; so are F = 0, F > 65535 and
 * sides > 32768. */
#define DNS_MS_SSIM_MIN_SIDE 160u
void dns_ms_ssim_window(float* window);
uint64_t dns_ms_ssim_ws_bytes(uint32_t F, uint32_t H, uint32_t W);
int dns_ms_ssim(const float* pred, const float* gt, const float* depth, uint32_t F, uint32_t H, uint32_t W, void* ws, double* ms_ssim,
                double* mse, int64_t* n_valid, double* levels, void* stream);

/* dns_label_confusion: confusion matrices of F label-image pairs gt, pred [F,N] int32: conf [F,n_class,n_class] int64, rows = gt,
 * conf[f,g,p] = the number of pixels of frame f with gt g and pred p; n_invalid [F] int64 = the pixels whose gt or pred lies outside
 * [0, n_class), which are counted there and nowhere else.  Both outputs are cleared by the call.  n_class <=
 * DNS_CONFUSION_LDS_CLASSES: a histogram in LDS per workgroup of 4096 pixels, flushed with 64-bit integer atomics; above it 64-bit
 * integer atomics on conf directly.  Integer sums: exact and the same for every call on both paths. */
#define DNS_CONFUSION_LDS_CLASSES 64u
#define DNS_CONFUSION_MAX_CLASSES 4096u
int dns_label_confusion(const int32_t* gt, const int32_t* pred, uint32_t F, uint64_t N, uint32_t n_class, int64_t* conf,
                        int64_t* n_invalid, void* stream);

/* ---- Depth L1 (calc_2d_metric, eval_3d.py:120-210 of the reference; csrc/mesh_raster.hip; ABI v18) ---------------------------
 * dns_rasterize_depth: depth [V,H,W] fp32 of the mesh verts [P,3] fp32, faces [F,3] int32 seen from the V poses w2c [V,16] fp32
 * (row-major world->camera, OpenCV axes: x right, y down, z forward); intr [host] (fx, fy, cx, cy), pixel centres at integer
 * coordinates.  Depth is camera-space z, the background 0, both faces of a triangle are drawn, nothing nearer than z_near or
 * beyond z_far.  Homogeneous rasterisation, no clipping, every operation one fp32 rounding in this order:
 *   v = ((r0 x + r1 y) + r2 z) + t per row of w2c;  d = ((j - cx) / fx, (i - cy) / fy, 1) for pixel (row i, column j);
 *   per edge, its vertices ordered by vertex index a < b: c = v_a x v_b (c.x = a.y b.z - a.z b.y, ...), negated when the winding
 *   runs b -> a; E = (d.x c.x + d.y c.y) + c.z; covered iff all three E >= 0 or all three E <= 0;
 *   n = (v1 - v0) x (v2 - v0), t = ((n.x v0.x + n.y v0.y) + n.z v0.z) / ((n.x d.x + n.y d.y) + n.z), accepted iff
 *   z_near <= t <= z_far; the pixel is the minimum of the accepted t (atomicMin on the bits), so the image is the same bits for
 *   every call, both methods and every list_cap.
 * A triangle with a non-finite vertex (in world or camera space) is skipped and flagged; one with n = 0 is skipped; one with an
 * index outside [0, P) is skipped and flagged (never dereferenced).
 *   flags: DNS_RASTER_SIMPLE = every triangle is drawn by its set-up thread (the baseline); otherwise boxes of at most 8 x 8
 *     pixels are, and the others go through a list to one workgroup each.  DNS_RASTER_STATS = count the set-up-thread
 *     triangles into status[2] (one atomic each: for tests and tools).
 *   list_cap: 0, or a smaller number of (triangle, view) pairs per launch than the default 2^24 (the list always holds every pair
 *     of a launch; a small cap means more launches -- at most 65536).
 *   dns_rasterize_ws_bytes: bytes of workspace (0: refused size -- F >= 2^31, a side 0 or > 32768).
 *   status [4] uint32 (device): status[0] = DNS_RASTER_NONFINITE | DNS_RASTER_BAD_INDEX bits; status[1] = (triangle, view) pairs
 *     drawn through the list; status[2] = pairs drawn by their set-up thread (with DNS_RASTER_STATS).
 * V = 0: nothing is launched.  F = 0: all zeros.  Needs 0 < z_near <= z_far < inf.
 *
 * dns_depth_l1: err [V] float64 = sum |a - b| / (H W) over ALL pixels of the stacks a, b [V,H,W] fp32 (differences and sums in
 * float64).  partial [V * DNS_DEPTH_L1_PARTS] float64 is the caller's scratch: one strided partial sum per workgroup, added in
 * a fixed order -- the same bits for every call.
 *
 * dns_views_see_any: sees [K] uint8 = pose k of w2c [K,16] sees at least one of the points pts [N,3], under the projection,
 * epsilon and inequalities of dns_frustum_seen (w2c in its convention).  N = 0: all zeros. */
#define DNS_RASTER_SIMPLE 1u
#define DNS_RASTER_STATS 2u
#define DNS_RASTER_NONFINITE 1u
#define DNS_RASTER_BAD_INDEX 2u
#define DNS_DEPTH_L1_PARTS 64u
uint64_t dns_rasterize_ws_bytes(uint32_t F, uint32_t V, uint32_t H, uint32_t W);
int dns_rasterize_depth(const float* verts, uint32_t P, const int32_t* faces, uint32_t F, const float* w2c, uint32_t V, uint32_t H,
                        uint32_t W, const float* intr, float z_near, float z_far, uint32_t flags, uint32_t list_cap, void* ws,
                        float* depth, uint32_t* status, void* stream);
int dns_depth_l1(const float* a, const float* b, uint32_t V, uint32_t H, uint32_t W, double* partial, double* err, void* stream);
int dns_views_see_any(const float* pts, uint32_t N, const float* w2c, uint32_t K, int H, int W, const float* intr, uint8_t* sees,
                      void* stream);

/* ---- Headless visualiser (utils/viz.py:45-177 of the reference; csrc/mesh_render.hip; ABI v27) ----------------------------------
 * dns_render_mesh: colour [V,H,W,3] fp32, depth [V,H,W] fp32 and index [V,H,W] int32 of the mesh verts [P,3], faces [F,3] int32,
 * colors [P,3] fp32 (per vertex) and of the points [N,3] fp32 with point_colors [N,3] fp32, drawn as squares of point_size
 * (1..16) pixels, seen from the V poses w2c [V,16]; intr, z_near, z_far, list_cap, the status words, DNS_RASTER_SIMPLE and
 * DNS_RASTER_STATS as for dns_rasterize_depth.  Triangle set-up, coverage, depth, the skipped triangles and their flags are that
 * function's expressions (csrc/dev_raster.hpp), so with N = 0 and no culling `depth` is dns_rasterize_depth's image bit for bit.
 *   visibility: per pixel the minimum of the 64-bit keys (bits of the depth << 32) | id over everything that covers it, id = the
 *     face index for a triangle and 0x80000000 | point index for a point: the nearest surface; at equal depth the lower face
 *     index, and a triangle before a point.  The images are the same bits for every call, both methods and every list_cap.
 *   culling, per (face, view), by num = (n.x v0.x + n.y v0.y) + n.z v0.z of the set-up: num < 0 is front-facing (the normal of
 *     the winding points at the camera).  DNS_RENDER_CULL_BACK drops the faces with num > 0, DNS_RENDER_CULL_FRONT those with
 *     num < 0; either drops num == 0.  Setting both is refused.
 *   points, every operation one fp32 rounding: p = ((r0 x + r1 y) + r2 z) + t per row; skipped and flagged
 *     (DNS_RENDER_NONFINITE_POINT) when the point or p is not finite; accepted iff z_near <= p.z <= z_far;
 *     u = fx (p.x / p.z) + cx, w = fy (p.y / p.z) + cy, h = point_size * 0.5; the square is the columns ceil(u - h) ..
 *     ceil(u - h) + point_size - 1 and the rows ceil(w - h) .. ceil(w - h) + point_size - 1 (the pixel centres in
 *     [u - h, u + h)), clipped to the image; its key depth is p.z.
 *   shading, one thread per pixel, every operation one fp32 rounding in this order:
 *     background (no key): color = background [3 host floats], depth 0, index -1;
 *     point: color = point_colors[point], depth = p.z, index = -2 - point;
 *     face f: index = f, depth = t; with d, E0, E1, E2 (edges (0,1), (1,2), (2,0)) and den = (n.x d.x + n.y d.y) + n.z as
 *       above: the three edge vectors sum to n, so den is the sum of the edge functions, and the weights divide by that sum
 *       of the rounded E, S = (E0 + E1) + E2, which keeps them a partition of one: the perspective-correct weights are
 *       w0 = E1 / S, w1 = E2 / S, w2 = E0 / S ((1, 0, 0) when S == 0: all three E are 0, the triangle is seen edge-on) and
 *       per channel color = (w0 c0 + w1 c1) + w2 c2, c_k = colors[faces[f][k]];
 *       with DNS_RENDER_HEADLIGHT: nn = (n.x n.x + n.y n.y) + n.z n.z, dd = (d.x d.x + d.y d.y) + 1,
 *       light = ambient + (1 - ambient) * (|den| / (sqrt(nn) * sqrt(dd))), color = color * light (flat, two-sided; points are
 *       not shaded).  0 <= ambient <= 1.
 *   dns_render_mesh_ws_bytes: the keys (8 bytes per pixel and view), the list counters and the list (0: refused size).
 * V = 0: nothing is launched.  F = 0 and N = 0: the background everywhere. */
#define DNS_RENDER_CULL_BACK 4u
#define DNS_RENDER_CULL_FRONT 8u
#define DNS_RENDER_HEADLIGHT 16u
#define DNS_RENDER_NONFINITE_POINT 4u
uint64_t dns_render_mesh_ws_bytes(uint32_t F, uint32_t V, uint32_t H, uint32_t W);
int dns_render_mesh(const float* verts, uint32_t P, const int32_t* faces, uint32_t F, const float* colors, const float* points,
                    const float* point_colors, uint32_t N, uint32_t point_size, const float* w2c, uint32_t V, uint32_t H, uint32_t W,
                    const float* intr, float z_near, float z_far, uint32_t flags, float ambient, const float* background,
                    uint32_t list_cap, void* ws, float* color, float* depth, int32_t* index, uint32_t* status, void* stream);

/* ---- keyframe codes of the mesh vertex query (get_2d_feature, slams/meshing.py:311-377; csrc/mesh_feature.hip; ABI v19) -------
 * For points pts [P,3] fp32 and K keyframes (w2c [K,16] fp32 row-major = torch.inverse(est_c2w), depth [K,H,W] fp32 = gt_depth,
 * intr [host] (fx, fy, cx, cy)), keyframe k CONTRIBUTES to point p when it sees it -- dns_keyframe_project's projection and
 * inequalities (0 < u < W, 0 < v < H, z < 0), no maximum-depth test -- and the truncation test passes at the rounded (half to
 * even), clamped pixel (iu, iv): neither -z < depth[k, iv, iu] * 0.95 nor -z > depth[k, iv, iu] * 1.05 (fp32 products; both
 * limits inclusive; a depth of 0 never passes).  The pairs form a list, point-major, keyframes ascending within a point:
 *   dns_kf_pair_count: count [P] int32 = contributing keyframes per point.  P * K must stay below 2^31.
 *   dns_kf_pair_emit: offset [P] int64 = the exclusive prefix of count (made by the caller); records [capacity, 4] int32,
 *     16-byte aligned: pair offset[p] + i is {point, keyframe, iu, iv}.  Nothing is stored at or beyond `capacity`.
 *   dns_kf_pair_rows: for the n records, rel [n,3] = pts[point] - origin[keyframe] (origin [K,3] = est_c2w[:3,3]; refer_p,
 *     meshing.py:364) and, at code + pair * ld_code, the C values of the stem map feat [K,h,w,C] (channels last, half
 *     resolution) up-sampled bilinearly to H x W with align_corners=True and read at (iv, iu) -- dns_feature_gather's tap
 *     expressions.  C % 4 == 0, ld_code % 4 == 0, feat / code / records 16-byte aligned; anything else is DNS_E_ARG.
 *   dns_kf_code_mean: code [P,D] = the sum of the point's segment of latents [n, ld_lat] (Merge's output per pair) added in list
 *     order in fp32 -- the order of the reference's `+=` over the keyframes -- divided by (float)count; zeros where count == 0.
 *     D % 4 == 0, ld_lat % 4 == 0, 16-byte aligned.
 * No atomics: every output is the same bits for every call and for every split of the points into chunks. */
int dns_kf_pair_count(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* depth, int H, int W,
                      const float* intr, int32_t* count, void* stream);
int dns_kf_pair_emit(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* depth, int H, int W,
                     const float* intr, const int64_t* offset, int32_t* records, uint64_t capacity, void* stream);
int dns_kf_pair_rows(const int32_t* records, uint64_t n, const float* pts, uint32_t P, const float* origin, uint32_t K,
                     const float* feat, uint32_t C, int h, int w, int H, int W, float* rel, float* code, uint32_t ld_code,
                     void* stream);
int dns_kf_code_mean(const float* latents, uint32_t ld_lat, uint64_t n, const int64_t* offset, const int32_t* count, uint32_t P,
                     uint32_t D, float* code, void* stream);

/* ---- point masks (Mesher.point_masks, slams/meshing.py:124-291; csrc/mesh_masks.hip; ABI v20) --------------------------------
 * cls [P] uint8 = 0 unseen, 1 seen, 2 forecast for the points pts [P,3] fp32 against the K poses w2c [K,16] fp32 (row-major
 * world->camera), under dns_keyframe_project's projection (intr [host] = fx, fy, cx, cy).  Pose k has the point INSIDE when
 * 0 < u < W, 0 < v < H and z < 0, and in its FORECAST FRUSTUM when -1000 < u < W + 1000, -1000 < v < H + 1000 and z < 0.  A point
 * is seen when some pose has it inside and that pose's depth rule for seeing holds; forecast when it is not seen and some pose has
 * it in the forecast frustum under that pose's rule for forecasting.  With dz = -cam_z the rules are, by mode:
 *   frustum only (max_depth NULL, depths NULL; get_mask_use_all_frames, :164-201): none.
 *   depth limit  (max_depth [K] = the maximum of each keyframe's gt_depth; :257-271): dz < 1.2 max_depth[k] for both; the seen
 *     points are dns_keyframe_project's, the same bits.
 *   depth test   (depths [K,H,W] fp32, chunk > 0 = the reference's points_batch_size; :229-255): ds = the bilinear sample of
 *     depths[k] at (u, v) with pixel i at coordinate i and taps outside the image contributing 0 (F.grid_sample, zeros padding,
 *     align_corners=True); seeing needs dz < ds + 0.1 and ds - 2.5 < dz; forecasting needs dz < m[c,k], the maximum of ds over ALL
 *     points of the point's chunk c = p / chunk, whatever frustum they lie in (torch.max(depth_sample), :243: the result depends
 *     on the chunk length, as the reference's does; chunk >= P is one chunk).  Two passes: the table m [n_chunks, K] is built in
 *     ws by integer atomic maxima (order-independent: the same bits for every call), then the classes.  The library presets the
 *     table; dns_point_masks_ws_bytes gives its size (0 when none is needed or the size is refused).
 * A non-finite (u, v) (cam_z + 1e-8 == 0) samples as 0 and is inside nothing; the reference carries a NaN into the chunk maximum
 * there.  P = 0: nothing is launched.  K = 0: every point is unseen.  Refused: P >= 2^31, both max_depth and depths, depths with
 * chunk == 0, chunk != 0 without depths, H or W < 1, a depth test without ws. */
uint64_t dns_point_masks_ws_bytes(uint32_t P, uint32_t K, uint32_t chunk);
int dns_point_masks(const float* pts, uint32_t P, const float* w2c, uint32_t K, const float* max_depth, const float* depths,
                    uint32_t chunk, int H, int W, const float* intr, void* ws, uint8_t* cls, void* stream);

/* ---- TSDF fusion of posed depth images (the volume of get_bound_from_frames, slams/meshing.py:380-445; csrc/tsdf.hip; ABI v21) --
 * Open3D's ScalableTSDFVolume as tests/tsdf_ref.py restates it: units of 16^3 voxels of edge voxel_length, unit (ux, uy, uz)
 * covering [16 u voxel_length, 16 (u + 1) voxel_length) per axis.  intr [host, 4 doubles] = fx, fy, cx, cy.
 *   dns_tsdf_touch: depth [K,H,W] fp32, pose [K,16] float64 row-major camera->world (Open3D's convention: the camera looks along
 *     +z).  Every pixel (i, j) with i % stride == 0, j % stride == 0 and 0 < depth < 1000 is back-projected in float64 and touches
 *     the units floor((p - sdf_trunc) / L) .. floor((p + sdf_trunc) / L) per axis, L = 16 voxel_length (2 sdf_trunc < L required).
 *     table [cap] uint64 receives the distinct (unit, frame) keys -- (int16 ux) << 48 | (uy + 32768) << 32 | (uz + 32768) << 16 |
 *     frame, so that their order as SIGNED 64-bit integers is the lexicographic order of (ux, uy, uz, frame) -- in unspecified
 *     slots, all-ones elsewhere (the library presets it).  status [1]: bit 0 = the table was too small (retry with a larger one;
 *     the table's content is then incomplete), bit 1 = a unit index outside 16 bits.  K <= 65535.
 *   dns_tsdf_integrate: units [B,3] int32 and, for unit b, its frames frames[offset[b] .. offset[b+1]) (offset [B+1] int64) in the
 *     order to integrate them.  extrinsic [K,16] float64 world->camera is rounded to fp32; mult [H,W] fp32 is the camera-distance
 *     multiplier sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1).  The voxel centre (i + 0.5) voxel_length + 16 u voxel_length is
 *     rounded to fp32 and transformed in fp32; with z > 0, u = x fx / z + cx + 0.5 (v likewise) must satisfy 1e-4 <= u < W - 1e-4;
 *     with d = depth[(int)v, (int)u] the update applies when d > 0 and sdf = (d - z) mult > -sdf_trunc: t = min(1, sdf / sdf_trunc),
 *     tsdf = (tsdf w + t) / (w + 1), w += 1.  tsdf, weight [B,16,16,16] fp32 (x, y, z), 16-byte aligned, are written once each.
 *   dns_tsdf_vertex_count / dns_tsdf_vertex_emit: units sorted in the key order above.  Voxel a and axis e emit one vertex when a
 *     and a + e are observed (weight > 0) with different (tsdf < 0) and at least one of the four cubes around that edge has eight
 *     observed corners, looking into neighbouring units (a missing unit is unobserved): float64 0.5 voxel_length + voxel_length
 *     index, plus |f_a| voxel_length / (|f_a| + |f_b|) along e.  count [B] int64 per unit; offset [B] = its exclusive prefix (the
 *     caller's); verts [capacity,3] float64 ordered by unit, voxel ((x 16 + y) 16 + z), axis.  Nothing is stored at or beyond capacity.
 * No float atomics: the same bits for every call. */
int dns_tsdf_touch(const float* depth, const double* pose, uint32_t K, int H, int W, int stride, const double* intr,
                   double voxel_length, double sdf_trunc, uint64_t* table, uint32_t cap, uint32_t* status, void* stream);
int dns_tsdf_integrate(const int32_t* units, uint32_t B, const int64_t* offset, const int32_t* frames, const float* depth,
                       const double* extrinsic, const float* mult, uint32_t K, int H, int W, const double* intr,
                       double voxel_length, double sdf_trunc, float* tsdf, float* weight, void* stream);
int dns_tsdf_vertex_count(const int32_t* units, uint32_t B, const float* tsdf, const float* weight, int64_t* count, void* stream);
int dns_tsdf_vertex_emit(const int32_t* units, uint32_t B, const float* tsdf, const float* weight, double voxel_length,
                         const int64_t* offset, double* verts, uint64_t capacity, void* stream);

/* ---- 3-D convex hull (quickhull; csrc/hull.hip, csrc/hull_topology.hpp; ABI v21) ---------------------------------------------
 * points [N,3] float64 on the device.  Face f sees a point when n_f . x + d_f > eps + 1e-12 L (L = the largest absolute
 * coordinate; hull_topology.hpp states the algorithm and its degeneracy policy).  HOST outputs: faces_out [face_cap,3] int32
 * (indices into points, outward orientation), planes_out [face_cap,4] float64 (unit outward n, d: inside is n . x + d <= 0),
 * *n_faces_out, info [4] = the measured maximum of n . x + d over all points and faces, rounds, sweeps, L.  ws: device memory of
 * dns_convex_hull_ws_bytes(N, face_cap) bytes (0 = refused), face_cap bounding the faces ever made, replaced ones included.
 * Returns DNS_OK; 1 when face_cap was too small (retry with a larger one); DNS_E_ARG for fewer than 4 points or points within
 * eps of one plane; DNS_E_STATE on a capturing stream or when the topology could not be kept (never a face with a zero normal).
 * The call synchronises the stream once per round and is NOT graph-capturable. */
uint64_t dns_convex_hull_ws_bytes(uint32_t N, uint32_t face_cap);
int dns_convex_hull(const double* points, uint32_t N, double eps, void* ws, uint32_t face_cap, int32_t* faces_out,
                    double* planes_out, uint32_t* n_faces_out, double* info, void* stream);

/* ---- image stem (reference models/layers.py:56-58,95-98 through models/encoder.py:9-17; csrc/stem.hip, csrc/stem_tile.hpp; ABI v22)
 * conv 7x7 stride 2 zero-pad 3, 3 -> 64 channels, no bias, exact fp32 products and fp32 accumulation in (ky, kx, c) order; then
 * y = relu(fma(conv, s_c, t_c)), the ReLU keeping a NaN.  images [n,H,W,3] fp32 channels-last; out [n,h,w,64] fp32 channels-last,
 * h = (H-1)/2 + 1, w = (W-1)/2 + 1, 128-byte aligned.  wpack [148][64]: weight[o][c][ky][kx] at row (ky 7 + kx) 3 + c, column o,
 * row 147 zero; 16-byte aligned.  st [2][64]: s then t.  The bits of an image's map depend on nothing but the image, wpack and st.
 * flags of dns_stem_forward:
 *   DNS_STEM_STORE | DNS_STEM_EPILOGUE  the normalised maps (frozen statistics: st from the running statistics);
 *   DNS_STEM_STATS [| DNS_STEM_STORE]   one row [2][64] float64 per workgroup in `partials` -- sums of conv and conv^2 over the
 *                                       workgroup's pixels, taken from the fp32 conv values -- dns_stem_partial_rows(n, H, W)
 *                                       rows (0 = shape refused); with DNS_STEM_STORE the raw convolution is stored as well.
 * Any other combination is refused.
 * dns_stem_batch_stats adds the rows in a fixed order (level1: scratch of 256 rows) and writes st for nn.BatchNorm2d's TRAIN
 * mode: mean and biased variance over the n h w values of a channel, s = gamma / sqrt(var + eps), t = beta - mean s in float64,
 * rounded to fp32; n h w = 1 is refused.  Running statistics are neither read nor written.  dns_stem_normalise applies
 * y = relu(fma(y, s_c, t_c)) in place to [n_pixels][64] raw values: the bits DNS_STEM_EPILOGUE stores.  No atomics anywhere. */
#define DNS_STEM_STATS 1u
#define DNS_STEM_EPILOGUE 2u
#define DNS_STEM_STORE 4u
uint64_t dns_stem_partial_rows(uint32_t n, uint32_t H, uint32_t W);
int dns_stem_forward(const float* images, uint32_t n, uint32_t H, uint32_t W, const float* wpack, const float* st, float* out,
                     uint32_t flags, double* partials, void* stream);
int dns_stem_batch_stats(const double* partials, uint32_t n, uint32_t H, uint32_t W, const float* gamma, const float* beta,
                         double eps, double* level1, float* st, void* stream);
int dns_stem_normalise(float* out, uint64_t n_pixels, const float* st, void* stream);

/* ---- the 2-D code of a frame's samples (csrc/frame_codes.hip, csrc/frame_codes_plan.hpp; ABI v23) -----------------------------
 * Replaces, per chunk of a full-frame render, feature_matching (reference utils/common.py:645-679) + Decoder.merge
 * (models/decoder.py:67-77) as frame_vis (slams/mapping.py:666-689) and novel_view_render (eval_2d.py:260-283) call them: one
 * kernel, the Merge rows never reach HBM.  pts [P,3]; w2c [R,16] row-major world->camera; origin [R,3] = the translations of the
 * inverse poses; K [host, 9 floats] row-major intrinsics; feat [R,h,w,C] fp32 channels-last stem maps; keep [P] bytes or NULL;
 * bound [host, 6 doubles] b0x,b1x,b0y,b1y,b0z,b1z = Merge's bound; params = the Merge network's fp32 weights (3 n_bins + C inputs,
 * hid outputs, n_neurons x n_hidden_layers = 32 x 1 or 64 x 2).  out [P][ld_out], columns [0, hid).
 * Per view r: the projection and validity test of dns_feature_gather (y and z flipped, u = rint(q0 / (q2 + 1e-5)), valid iff
 * 0 < u < W-1, 0 < v < H-1, cz > 0); the code is the bilinear value (align_corners=True) of the half-resolution map at that integer
 * pixel -- dns_feature_gather's bits -- or zeros where the view is not valid (no tap is read then); the row is OneBlob of
 * (p - origin_r), normalised with bound in fp64 (dns_encode_fwd's bits), followed by the code; the latent is the network on the row
 * (dns_mlp_fwd's bits).  out = (latent_0 + latent_1 + ... in view order) / R.  keep[p] == 0: a zero row, none of p's taps read.
 * No atomics: the same bits for every call, every split of the points and every tile_pts.  tile_pts = the points a workgroup
 * takes at a time: 0 = chosen by the library (128, or 64 / 32 where the points would not fill the device), else 32, 64 or 128.
 * ws: dns_frame_codes_ws_floats(...) floats for the same tile_pts, 16-byte aligned; 0 = shape refused (C or 3 n_bins no multiple of
 * 4, 3 n_bins + C no multiple of 8 or above 128, hid no multiple of 4 or above 64, R above 64, another network shape or tile).
 * feat, params and out 16-byte aligned, ld_out a multiple of 4.  P = 0: nothing is launched. */
uint64_t dns_frame_codes_ws_floats(uint32_t P, uint32_t R, uint32_t n_bins, uint32_t C, uint32_t hid, uint32_t n_neurons,
                                   uint32_t n_hidden_layers, uint32_t tile_pts);
int dns_frame_codes(const float* pts, uint32_t P, const float* w2c, const float* origin, uint32_t R, const float* K,
                    const float* feat, uint32_t C, int h, int w, int H, int W, const uint8_t* keep, const double* bound,
                    uint32_t n_bins, const float* params, uint32_t n_neurons, uint32_t n_hidden_layers, uint32_t hid,
                    float* ws, uint64_t ws_floats, float* out, uint32_t ld_out, uint32_t tile_pts, void* stream);

/* ---- LPIPS (eval_2d.py:81-82,304 of the reference: torchmetrics 0.11.1's LearnedPerceptualImagePatchSimilarity(net_type='alex',
 * normalize=True) over lpips 0.1.4; csrc/lpips.hip, csrc/conv_plan.hpp; ABI v24) ---------------------------------------------
 * The definition, per image pair pred, gt [H,W,3] fp32 (the project's channels-last layout):
 *   1. input scaling: x = clamp(x, 0, 1); x = 2x - 1; x = (x - shift_c) / scale_c, shift = (-0.030, -0.088, -0.188),
 *      scale = (0.458, 0.448, 0.450).  A NaN stays a NaN.  The first convolution's zero padding is zero IN THIS SCALED SPACE.
 *   2. tower = torchvision AlexNet `features`; every convolution has a bias and is followed by ReLU; the features are
 *        f0 = conv1(x)         3 ->  64, 11x11, stride 4, pad 2
 *        f1 = conv2(pool(f0)) 64 -> 192,  5x5,  pad 2
 *        f2 = conv3(pool(f1)) 192 -> 384, 3x3,  pad 1
 *        f3 = conv4(f2)      384 -> 256,  3x3,  pad 1
 *        f4 = conv5(f3)      256 -> 256,  3x3,  pad 1
 *      pool = max 3x3, stride 2, no padding, floor mode.  ReLU and max keep a NaN.
 *   3. head, per layer l and pixel: n(f) = f / (sqrt(sum_c f_c^2) + 1e-10);
 *      d_l = mean over pixels of sum_c lin_l[c] (n(f_pred)_c - n(f_gt)_c)^2.  lin_l has no bias; there is no dropout.
 *   4. lpips = sum_l d_l.
 * Sides below 31 leave the second pool empty and are refused.  The arithmetic is pinned to a float64 restatement of this definition
 * (tests/lpips_ref.py), not to a file written by the lpips package: neither it nor any pretrained weight is part of the repository.
 *
 * dns_conv_cl: channels-last convolution + bias (NULL = none) + ReLU (DNS_CONV_RELU, keeping a NaN): x [n,H,W,Cin] ->
 * out [n,h,w,Cout], h = (H + 2 pad - ks) / stride + 1, square kernel ks <= 11, stride <= 4, pad < ks, Cout a multiple of 64; exact
 * fp32 products, fp32 accumulation from 0 in (ky, channel slice, kx, c) order, then + bias: the bits of an image's map depend on
 * nothing but the image, wpack and bias.  wpack: the packed weight image [shape[0]][shape[1]][shape[2]][64] of dns_conv_pack_shape
 * (shape = {Cout / 64, chunks, k per chunk padded to even, CK channels per chunk}): chunk = ky (Cin / CK) + cs; element
 * (cb, chunk, kx CK + c, o) = weight[cb 64 + o][cs CK + c][ky][kx]; rows past ks CK zero; 16-byte aligned.  x 16-byte aligned where
 * Cin % 4 == 0; out 128-byte aligned.  DNS_CONV_SCALE_INPUT (Cin = 3 only): step 1 is applied to x as it is staged, the padding
 * staying 0.  No atomics.
 * dns_max_pool_cl: x [n,h,w,C] -> out [n,(h-3)/2+1,(w-3)/2+1,C], C a multiple of 4, both 16-byte aligned; a NaN in a window wins.
 * dns_lpips_head: one layer: fa, fb [F,h,w,C] (C a multiple of 64, <= 512), lin [C] -> partials [F][dns_lpips_head_blocks(h, w)]
 * float64, one per workgroup (64 consecutive pixels), everything after the fp32 features in float64; a pixel whose features are all
 * zero contributes 0.  dns_lpips_finish: partials / h / w [host arrays of n_layers <= 5 entries]: adds each layer's partials in
 * index order, divides by h w -> layers [F][n_layers]; lpips [F] = their sum in layer order.  No floating-point atomics: the same
 * bits for every call and every batch. */
#define DNS_CONV_RELU 1u
#define DNS_CONV_SCALE_INPUT 2u
int dns_conv_pack_shape(uint32_t Cin, uint32_t Cout, uint32_t ks, uint32_t stride, uint32_t pad, uint32_t* shape);
int dns_conv_cl(const float* x, uint32_t n, uint32_t H, uint32_t W, uint32_t Cin, const float* wpack, const float* bias, uint32_t Cout,
                uint32_t ks, uint32_t stride, uint32_t pad, uint32_t flags, float* out, void* stream);
int dns_max_pool_cl(const float* x, uint32_t n, uint32_t h, uint32_t w, uint32_t C, float* out, void* stream);
uint32_t dns_lpips_head_blocks(uint32_t h, uint32_t w);
int dns_lpips_head(const float* fa, const float* fb, const float* lin, uint32_t F, uint32_t h, uint32_t w, uint32_t C, double* partials,
                   void* stream);
int dns_lpips_finish(const double* const* partials, const uint32_t* h, const uint32_t* w, uint32_t n_layers, uint32_t F, double* lpips,
                     double* layers, void* stream);

/* ---- frame preparation (BaseDataset.__getitem__, datas/slam_datasets.py:85-149; csrc/frame_prep.hip, csrc/frame_prep_plan.hpp;
 * ABI v28) -------------------------------------------------------------------------------------------------------------------------
 * The raw 8/16-bit images of n frames -> the float colour, float depth and int64 class image the reference hands the tracker and
 * the mapper, in ONE launch, every output pixel on its own through the reference's stages in the reference's order:
 *   colour  1. fl32(u8) / 255.0f, a correctly rounded fp32 division, per tap;
 *           2. cv2.resize(color, (Wd, Hd)), bilinear on float32: the horizontal pass a w0 + b w1 first, the vertical pass on its
 *              results, each product and each sum rounded to fp32;
 *           3. F.interpolate(mode='bilinear', align_corners=True) to (Hs, Ws): horizontal, then vertical, rounded alike;
 *           4. the crop [edge, Hs - edge) x [edge, Ws - edge).
 *   depth   fl32(fl32(u16) / fl32(png_depth_scale)) * fl32(scale); F.interpolate(mode='nearest') to (Hs, Ws); the crop.
 *   label   cv2.resize(..., INTER_NEAREST) to (Wd, Hd); lut[value]; F.interpolate(mode='nearest'); the crop.
 * A stage whose source and destination sizes are equal is the identity (so without crop_size: Hs, Ws = Hd, Wd), and the colour of
 * all-identity dims is fl32(u8) / 255 bit for bit.  The resampling rules are the tables' (frame_prep_plan.hpp states each); the two
 * cv2 stages follow OpenCV's published rule, not arrays OpenCV wrote.  cv2.undistort is not built.
 *
 * dns_frame_prep_table_words: words of the table blob of dims d [host]; 0 = refused (a side of 0 or above 32768, labels with one
 *   side 0, 2 edge >= Hs or Ws).  Hl = Wl = 0: no label image.
 * dns_frame_prep_tables: fills words [host, n_words = dns_frame_prep_table_words(d)] on the host; the caller copies it to the device.
 * dns_prepare_frames: color uint8 [n,Hc,Wc,3] (bgr != 0: channel order B, G, R), depth uint16 [n,Hd,Wd], label uint8
 *   (label_bytes 1) or uint16 (2) [n,Hl,Wl] or NULL with label_bytes 0 and Hl = Wl = 0, lut int32 [65536] (NULL without labels),
 *   tables: the DEVICE copy of the blob of d, table_words its size (checked against d) -> out_color fp32 [n,H,W,3] in RGB,
 *   out_depth fp32 [n,H,W], out_label int64 [n,H,W] (NULL without labels), H = Hs - 2 edge, W = Ws - 2 edge.  n <= 65535.  No
 *   atomics; every table index is clamped into its image before it is used, so no read leaves the images whatever the blob
 *   holds; a frame's bits do not depend on n.
 * dns_label_first_seen: label uint8 / uint16 [n_pixels] (frames concatenated; n_pixels < 2^31) -> first int32 [65536]: for every
 *   value the smallest flat index at which it occurs, -1 for a value that does not.  Integer atomic minimum: the same for every call.
 *   (This is what cal_class_n's set(label_data.flatten()) needs: a set's iteration order depends on the order in which DISTINCT
 *   keys arrive, i.e. on first occurrences.) */
typedef struct DnsFramePrepDims {
  uint32_t Hc, Wc;   /* colour image */
  uint32_t Hd, Wd;   /* depth image: the size cv2.resize takes colour and labels to */
  uint32_t Hl, Wl;   /* label image; 0, 0 = none */
  uint32_t Hs, Ws;   /* cfg['cam']['crop_size']; Hd, Wd where the config sets none */
  uint32_t edge;     /* cfg['cam']['crop_edge'] */
} DnsFramePrepDims;
uint64_t dns_frame_prep_table_words(const DnsFramePrepDims* d);
int dns_frame_prep_tables(const DnsFramePrepDims* d, int32_t* words, uint64_t n_words);
int dns_prepare_frames(const uint8_t* color, int bgr, const uint16_t* depth, const void* label, int label_bytes, const int32_t* lut,
                       const DnsFramePrepDims* d, const int32_t* tables, uint64_t table_words, uint32_t n, float png_depth_scale,
                       float scale, float* out_color, float* out_depth, int64_t* out_label, void* stream);
int dns_label_first_seen(const void* label, int label_bytes, uint64_t n_pixels, int32_t* first, void* stream);

/* ---- keyframe overlap (the projection block of keyframe_selection_overlap, slams/mapping.py:208-226; csrc/keyframes.hip;
 * ABI v29) -----------------------------------------------------------------------------------------------------------------------
 * dns_keyframe_overlap: pts fp32 [P,3], c2w fp32 [n,4,4] (row-major, all on the device) -> out int32 [n]: per keyframe the number
 * of points that project more than `edge` pixels inside the H x W image with z < 0.  No host read.  The arithmetic, every
 * operation rounded once (no contraction), tests/keyframe_overlap_ref.py being the numpy restatement that the counts must EQUAL:
 *   1. the pose and the point are widened to float64;
 *   2. w = inverse(c2w) by the adjugate: the six 2 x 2 minors s0..s5 of rows 0-1 and c0..c5 of rows 2-3 (column pairs 01, 02, 03, 12,
 *      13, 23), det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0, and every entry of rows 0-2 as its three-term
 *      cofactor sum, in the order csrc/keyframes.hip writes out, divided by det;
 *   3. camera coordinates ((w_r0 x + w_r1 y) + w_r2 z) + w_r3 for r = 0, 1, 2; xc is negated;
 *   4. ze = zc + eps; u = (fx xc + cx zc) / ze, v = (fy yc + cy zc) / ze;
 *   5. u, v rounded to fp32; inside = u < fl32(W - edge), u > fl32(edge), v < fl32(H - edge), v > fl32(edge), ze < 0, all strict.
 * A point with a non-finite coordinate is outside; a pose with a non-finite entry, or whose determinant is 0 or non-finite, counts 0.
 * Counting is a wave ballot per pass and one integer atomic add per workgroup into out (zeroed first by a kernel): order-free.
 * n == 0: nothing is done; P == 0: out is zeroed.  n <= 65535, P < 2^31, H, W, edge <= 2^24. */
int dns_keyframe_overlap(const float* pts, uint32_t P, const float* c2w, uint32_t n, int H, int W, double fx, double fy, double cx,
                         double cy, int edge, double eps, int32_t* out, void* stream);

/* ---- visualisation panels (fig_plot, utils/common.py:682-745, as frame_vis calls it, slams/mapping.py:638-724; csrc/vis_panels.hip,
 * csrc/plasma_lut.hpp; ABI v29) ---------------------------------------------------------------------------------------------------
 * dns_vis_panels: gt_color, est_color fp32 [H,W,3], gt_depth, est_depth fp32 [H,W], gt_label, est_label int32 [H,W], label_lut
 * int32 [n_lut] or NULL -> out uint8 [3H + 2 gap, 3W + 2 gap, 3] and vmax_bits (one word: the bits of the depth row's vmax).
 * Panel (r, c) starts at pixel (r (H + gap), c (W + gap)); rows: depth, colour, label; columns: input, generated, |input -
 * generated| (fp32 for depth and colour; on the mapped integer labels for the label row).  Everything outside a panel = background.
 *   scalar panels: index = trunc(fl32(fl32(x / vmax) * 256)), below 0 -> 0, 256 and above -> 255, then plasma_lut.hpp's triple: what
 *     matplotlib's plasma(Normalize(0, vmax)(x), bytes=True) gives.  vmax == 0 -> index 0.  Depth: vmax = the largest finite
 *     positive gt depth (0 if there is none), an integer atomic maximum on the floats' bits: the same on every call.  Labels:
 *     vmax = max_label, after label = label_lut[label] where 0 <= label < n_lut (else unchanged, as dict.get(value, value)).
 *     A non-finite scalar pixel takes the background colour (matplotlib draws its "bad" colour, transparent, there).
 *   colour panels: trunc(fl32(clip(x, 0, 1) * 255)) per channel; a NaN is taken as 0.
 * Titles, axes and the JPEG encoding of the reference's figure are not rebuilt.  H, W <= 16384, gap <= 4096, background <= 255. */
int dns_vis_panels(const float* gt_color, const float* est_color, const float* gt_depth, const float* est_depth,
                   const int32_t* gt_label, const int32_t* est_label, const int32_t* label_lut, uint32_t n_lut, uint32_t H, uint32_t W,
                   float max_label, uint32_t gap, uint32_t background, uint8_t* out, uint32_t* vmax_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DNS_HIP_H */
