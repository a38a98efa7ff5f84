"""What MapStep and TrackStep (fused_step.py) share: the row format of a point set's MLP input, the in-step 2-D branch and
the ray-branch buffers.

A ROW FORMAT is how a point set's network input lives in memory (include/dns_hip.h): ``Fp32Rows``, ``SplitRows`` or ``HalfRows``
(one base class, ``_Rows``, for what they share).  One object is built per point set (ray branch, lattice); it owns the rows and offers the four operations a step needs of them --
``encode`` the points, build the ``feature_block``, ``fwd`` and ``bwd`` of a network -- so the steps themselves never ask which
format they run on.  A network travels as one ``Net`` value.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import ops
from ._lib import DnsSplitRows, check, ptr

_V = C.c_void_p


def aligned_floats(n, align, dev):
    """[n] fp32 whose first element sits on a multiple of ``align`` floats."""
    blob = torch.empty(n + 64, device=dev)
    off = (-blob.data_ptr() // 4) % align
    return blob[off:off + n]


class Net(NamedTuple):
    w: torch.Tensor                            # fp32 parameters, or their prepared operand images (flags then carry DNS_MLP_PREPARED)
    shape: tuple                               # (n_in, n_out, n_neurons, n_hidden_layers)
    flags: int = 0                             # DNS_MLP_FP16 | DNS_MLP_PREPARED
    stride: int = 0                            # floats between the weight sets of a pool
    table: Optional[tuple] = None              # (row_index, tile_group, n_slots) of a grouped launch; None = one slot per point
    hidden: Optional[torch.Tensor] = None      # kept hidden activations (dns_mlp_fwd h_save -> dns_mlp_bwd h_saved)


def dwin_on_side(fork, x, x2, n_in1, net, d_p, ws, n_slots, ri, tg, flags):
    """dW_in = dH_1^T x (memory-bound, needs only what the backward launch left in ws) on the side stream, beside the next
    network's vector-bound backward kernel.  ``fork`` = (main stream, side stream, side stream handle)."""
    main, side, side_st = fork
    ev = torch.cuda.Event()
    ev.record(main)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        ops.launch_mlp_dwin(x, x2, n_in1, net.shape, d_p, ws, n_slots, ri, tg, net.stride, flags, side_st)


class _Rows:
    """What the formats share: the sizes (``n`` points, rows of ``ld`` columns of which ``pe`` are OneBlob, a feature block of
    ``n_feat`` columns or none) and the two entry points that write any of them -- dns_encode_fwd_split and
    dns_feature_block_split, whose outputs are (fp32 rows, ld, f16 rows / planes, ld, exponents, flags): ``enc_out``, ``block_out``."""
    live = 0                                   # the DNS_MLP_LIVE_IN word of the two-segment launches
    forks_dwin = True                          # the backward can leave dW_in to a dns_mlp_dwin launch

    def __init__(self, n, ld, pe, n_feat):
        self.n, self.ld, self.pe, self.n_feat = n, ld, pe, n_feat

    def encode(self, pts, b6, n_bins, table, meta, x3, dydx, st):
        check(ops.lib.dns_encode_fwd_split(ptr(pts), b6, self.n, n_bins, ptr(table), meta, ptr(x3), *self.enc_out, ptr(dydx), st),
              "dns_encode_fwd_split")

    def feature_block(self, fine, hid, code, views, z, gt_depth, N, S, raw, st):
        """(latents | truncated 2-D code) for the colour / logit networks, occupancy into the compositing input.  ``views`` =
        (n_refer, points per frame) when ``code`` holds one row per reference view (their mean is taken here), else None."""
        check(ops.lib.dns_feature_block_split(ptr(fine), hid + 1, hid, ptr(code), self.n_feat - hid, *(views or (1, 0)), ptr(z),
                                              ptr(gt_depth), N, S, *self.block_out, ptr(raw), st), "dns_feature_block_split")


class Fp32Rows(_Rows):
    """fp32 rows [n, ld] = (OneBlob | hash grid) and, with ``n_feat``, the feature block [n, n_feat] the colour / logit networks
    read as their second input segment (dns_mlp_fwd / dns_mlp_bwd).  ``null_split``: the (plane stride, flags)
    dns_feature_block_split is given beside its NULL split planes (nothing reads them; MapStep has always passed the layout the
    planes would have, TrackStep zeros)."""

    def __init__(self, n, ld, pe, n_feat, dev, live=0, null_split=(0, 0)):
        super().__init__(n, ld, pe, n_feat)
        self.live, self.buf = live, torch.empty(n, ld, device=dev)
        self.grid = _V(self.buf.data_ptr() + 4 * pe)
        self.feat = torch.empty(n, n_feat, device=dev) if n_feat else None
        self.block_out = (ptr(self.feat), n_feat, None, null_split[0], None, null_split[1])

    def encode(self, pts, b6, n_bins, table, meta, x3, dydx, st):
        check(ops.lib.dns_encode_fwd(ptr(pts), b6, self.n, n_bins, ptr(table), meta, ptr(x3), ptr(self.buf), self.ld, self.grid,
                                     self.ld, ptr(dydx), st), "dns_encode_fwd")

    def feature_block(self, fine, hid, code, views, z, gt_depth, N, S, raw, st):
        if views is not None:
            return super().feature_block(fine, hid, code, views, z, gt_depth, N, S, raw, st)
        check(ops.lib.dns_feature_block(ptr(fine), hid + 1, hid, ptr(code), self.n_feat - hid, ptr(z), ptr(gt_depth), N, S,
                                        ptr(self.feat), self.n_feat, ptr(raw), st), "dns_feature_block")

    def fwd(self, net, y, st, two=False):
        """y = net(rows) or, with ``two``, net(pe columns of the rows | feature block)."""
        w, shape, flags, stride, table, hidden = net       # (one unpack, not a field lookup per argument: the tracker is host-bound)
        x2, n_in1, live = (self.feat, self.pe, self.live) if two else (None, 0, 0)
        ri, tg, n_slots = table or (None, None, self.n)
        ops.launch_mlp_fwd(self.buf, x2, n_in1, w, shape, y, n_slots, ri, tg, stride, hidden, flags | live, st)

    def bwd(self, net, dy, d_x, d_feat, d_p, ws, acc, st, fork=None):
        """Input gradients into d_x (and d_feat: the launch is then the two-segment one) and, with d_p, weight gradients;
        ``acc`` = the entry point's accumulate bits (+ DNS_MLP_DX_FROM).  ``fork``: dW_in goes to the side stream."""
        w, shape, flags, stride, table, hidden = net
        x2, n_in1, live = (None, 0, 0) if d_feat is None else (self.feat, self.pe, self.live)
        ri, tg, n_slots = table or (None, None, self.n)
        ops.launch_mlp_bwd(self.buf, x2, n_in1, dy, w, shape, d_x, d_feat, d_p, ws, n_slots, ri, tg, stride, hidden,
                           acc | flags | live | (ops.MLP_NO_DWIN_FLAG if fork else 0), st)
        if fork:
            dwin_on_side(fork, self.buf, x2, n_in1, net, d_p, ws, n_slots, ri, tg, (flags & ops.MLP_FP16_FLAG) | live)


class SplitRows(_Rows):
    """Split rows (ABI v9): the encoder and the feature block write their rows ONCE in the form the MLP kernels' matrix
    instructions take (f16 hi | lo halfs + one exponent per row) and every forward / backward launch loads its operand
    fragments straight from memory; the fp32 rows are still written for the streaming dW_in kernels.  Half-width networks
    (``fp16``) read the hi plane only.  The entry points take fp32 weights and full-width rows (no prepared images, no
    DNS_MLP_LIVE_IN, no DNS_MLP_DX_FROM)."""
    feat = rows_f = None                       # (a point set without a feature block: the lattice)

    def __init__(self, n, ld, pe, n_feat, dev, fp16):
        super().__init__(n, ld, pe, n_feat)
        np_, flags = (1, 1) if fp16 else (2, 0)                        # planes; DNS_SPLIT_HI_ONLY

        def rows(cols):
            x = torch.empty(n, cols, device=dev)
            xs, xexp = torch.empty(n, np_ * cols, device=dev, dtype=torch.float16), torch.empty(n, device=dev, dtype=torch.int32)
            desc = DnsSplitRows(xs.data_ptr(), xexp.data_ptr(), np_ * cols, cols if np_ == 2 else 0)
            return x, (xs, xexp), desc, (ptr(x), cols, ptr(xs), np_ * cols, ptr(xexp), flags)
        self.buf, self.planes_x, self.rows_x, self.enc_out = rows(ld)
        if n_feat:
            self.feat, self.planes_f, self.rows_f, self.block_out = rows(n_feat)

    def fwd(self, net, y, st, two=False):
        ri, tg, n_slots = net.table or (None, None, self.n)
        check(ops.lib.dns_mlp_fwd_split(C.byref(self.rows_x), C.byref(self.rows_f) if two else None, self.pe if two else 0,
                                        ptr(net.w), *net.shape, ptr(y), y.stride(0), n_slots, ptr(ri), ptr(tg), net.stride,
                                        net.flags, st), "dns_mlp_fwd_split")

    def bwd(self, net, dy, d_x, d_feat, d_p, ws, acc, st, fork=None):
        rows_f, x2, n_in1 = (None, None, 0) if d_feat is None else (C.byref(self.rows_f), self.feat, self.pe)
        ri, tg, n_slots = net.table or (None, None, self.n)
        check(ops.lib.dns_mlp_bwd_split(C.byref(self.rows_x), rows_f, n_in1, ptr(dy), dy.stride(0), ptr(net.w), *net.shape, ptr(d_x),
                                        0 if d_x is None else d_x.stride(0), ptr(d_feat), 0 if d_feat is None else d_feat.stride(0),
                                        ptr(d_p), ptr(ws), n_slots, ptr(ri), ptr(tg), net.stride, (acc & 3) | net.flags, st),
              "dns_mlp_bwd_split")
        if fork:
            dwin_on_side(fork, self.buf, x2, n_in1, net, d_p, ws, n_slots, ri, tg, net.flags)
        else:
            ops.launch_mlp_dwin(self.buf, x2, n_in1, net.shape, d_p, ws, n_slots, ri, tg, net.stride, net.flags, st)


class HalfRows(_Rows):
    """Half rows (ABI v12): networks that ask for tcnn's own precision run on the native f16 kernels -- the encoder and the
    feature block write plain f16 rows, every network launch reads them, ONE backward kernel per network forms all gradients
    (no dH_1 workspace, no dns_mlp_dwin: ``ws`` and ``fork`` are ignored), gradients carry tcnn's static loss scale.  fp32
    weights (no prepared images)."""
    forks_dwin = False
    buf = feat = None                          # (no fp32 rows)

    def __init__(self, n, ld, pe, n_feat, dev, live, loss_scale):
        super().__init__(n, ld, pe, n_feat)
        self.live, self.loss_scale = live, loss_scale
        self.xh = torch.empty(n, ld, device=dev, dtype=torch.float16)
        self.feath = torch.empty(n, n_feat, device=dev, dtype=torch.float16) if n_feat else None
        self.enc_out = (None, 0, ptr(self.xh), ld, None, ops.SPLIT_PLAIN)
        self.block_out = (None, 0, ptr(self.feath), n_feat, None, ops.SPLIT_PLAIN)

    def fwd(self, net, y, st, two=False):
        x2, n_in1, live = (self.feath, self.pe, self.live) if two else (None, 0, 0)
        ri, tg, n_slots = net.table or (None, None, self.n)
        ops.launch_mlp_fwd_half(self.xh, x2, n_in1, net.w, net.shape, y, n_slots, ri, tg, net.stride, live, st, self.n_feat)

    def bwd(self, net, dy, d_x, d_feat, d_p, ws, acc, st, fork=None):
        x2, n_in1, live = (None, 0, 0) if d_feat is None else (self.feath, self.pe, self.live)
        ri, tg, n_slots = net.table or (None, None, self.n)
        ops.launch_mlp_bwd_half(self.xh, x2, n_in1, dy, net.w, net.shape, d_x, d_feat, d_p, n_slots, ri, tg, net.stride, acc | live,
                                self.loss_scale, st, self.n_feat)


class Stem2D:
    """The 2-D branch inside an iteration (slams/mapping.py:532-551, slams/tracking.py:162-165): projected image code + relative
    point of every sample in every reference view -> OneBlob -> Merge network; the feature block takes the mean over the views.
    ``n_frames`` frames of ``ppf`` points, ``R`` views each.  ``want_dw``: Merge trains (workspace for its weight gradients);
    ``want_pose``: its OneBlob input carries gradient back to the points (d_mpe, d_rel)."""

    def __init__(self, who, merge, n_frames, R, ppf, Cs, fh, fw, hid, intrinsics, dev, want_dw, want_pose):
        mg = merge.decoder
        self.shape = n_in, n_out, nn, nl = (mg.n_input_dims, mg.n_output_dims, mg.n_neurons, mg.n_hidden_layers)
        self.n_bins = merge.pe_fn.n_bins
        pe = self.pe = 3 * self.n_bins
        if not (n_in == pe + Cs and n_out == hid and pe % 4 == 0):
            raise ValueError(f"{who}: Decoder.merge's network does not match the stem features / hidden width")
        self.b6 = ops._bound6(merge.bound)
        self.n_frames, self.R, self.ppf, self.Cs, self.fh, self.fw = n_frames, int(R), ppf, int(Cs), int(fh), int(fw)
        Mr = self.Mr = n_frames * self.R * ppf
        f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        self.mbuf, self.rel, self.xm = f(Mr, n_in), f(Mr, 3), f(Mr, 3)
        self.code_cols = self.mbuf[:, pe:]                             # Merge's second input segment, in place
        self.mlat, self.mdy = f(Mr, n_out), f(Mr, n_out)
        self.d_mpe, self.d_rel = (f(Mr, pe), f(Mr, 3)) if want_pose else (None, None)
        self.ws = f(max(int(ops.lib._raw.dns_mlp_bwd_ws_floats(Mr, nn, nl)), 4)) if want_dw else None
        fx, fy, cx, cy = intrinsics
        self.K9 = (C.c_float * 9)(float(fx), 0.0, float(cx), 0.0, float(fy), float(cy), 0.0, 0.0, 1.0)

    def forward(self, pts, w2c, origin, maps, H, W, net, st):
        lib, n_in = ops.lib, self.shape[0]
        check(lib.dns_feature_gather_frames(ptr(pts), ptr(w2c), ptr(origin), self.K9, ptr(maps), self.n_frames, self.R, self.ppf,
                                            self.Cs, self.fh, self.fw, H, W, ptr(self.code_cols), n_in, ptr(self.rel), st),
              "dns_feature_gather_frames")
        check(lib.dns_encode_fwd(ptr(self.rel), self.b6, self.Mr, self.n_bins, None, None, ptr(self.xm), ptr(self.mbuf), n_in,
                                 None, 0, None, st), "dns_encode_fwd")
        ops.launch_mlp_fwd(self.mbuf, None, 0, net.w, self.shape, self.mlat, self.Mr, None, None, 0, None, net.flags, st)

    def backward(self, d_code, ldf, z, gt_depth, N, S, net, d_w, st, fork=None):
        """Merge's backward (models/decoder.py:67-77): d code (``d_code``: pointer to its columns in rows of ``ldf`` floats) -> the
        R views' latent gradients -> weight gradients into ``d_w`` and, with ``want_pose``, d OneBlob -> d(relative point)."""
        lib = ops.lib
        check(lib.dns_merge_dy(d_code, ldf, self.shape[1], self.R, self.ppf, ptr(z), ptr(gt_depth), N, S, ptr(self.mdy), st),
              "dns_merge_dy")
        ops.launch_mlp_bwd(self.mbuf, self.code_cols, self.pe, self.mdy, net.w, self.shape, self.d_mpe, None, d_w, self.ws, self.Mr,
                           None, None, 0, None, ops.MLP_DX_FIRST_FLAG | net.flags | (ops.MLP_NO_DWIN_FLAG if fork else 0), st)
        if fork:
            dwin_on_side(fork, self.mbuf, None, 0, net, d_w, self.ws, self.Mr, None, None, net.flags & ops.MLP_FP16_FLAG)
        if self.d_rel is not None:
            check(lib.dns_encode_bwd(ptr(self.xm), self.b6, self.Mr, self.n_bins, None, None, ptr(self.d_mpe), self.pe, None, 0,
                                     None, ptr(self.d_rel), None, None, 0, 0, st), "dns_encode_bwd")

    def add_ref_sum(self, P, d_x3, st):
        """d(relative point), summed over the views, into the points' gradient (before the pose reduction)."""
        check(ops.lib.dns_add_ref_sum(ptr(self.d_rel), self.R, self.ppf, P, ptr(d_x3), st), "dns_add_ref_sum")


def alloc_ray_buffers(o, N, S, n_class, n_feat, dev):
    """The ray branch's buffers as attributes of the step ``o``: rays and samples, the networks' and the compositing's outputs,
    the loss workspaces and the gradients on the way back to the points."""
    P = N * S
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    o.rays_o, o.rays_d, o.gt_color, o.gt_depth = f(N, 3), f(N, 3), f(N, 3), f(N)
    o.gt_label = torch.empty(N, device=dev, dtype=torch.int64)
    o.inside = torch.empty(N, device=dev, dtype=torch.uint8)
    o.z, o.pts, o.x3 = f(N, S), f(N, S, 3), f(P, 3)
    o.raw, o.logit = f(P, 4), f(P, n_class)
    o.depth, o.var, o.rgb, o.weights, o.sem = f(N), f(N), f(N, 3), f(N, S), f(N, n_class)
    o.sums_ws, o.out, o.one = f(ops.LOSS_SUMS_FLOATS), f(16), torch.ones(1, device=dev)
    o.d_color, o.d_depth, o.d_sem = f(N, 3), f(N), f(N, n_class)
    o.d_raw, o.d_logit = f(P, 4), f(P, n_class)
    # d_featx [P, 4 + n_feat]: column 3 = d occupancy, columns 4.. = the feature-block gradient of the colour / logit networks, so
    # columns 3 .. 3 + hidden are the fine (tracker: coarse) network's output gradient in one strided view.  Zeroed once: the
    # 2-D code's columns only ever accumulate and nothing reads them -- the code has no gradient
    o.d_featx = torch.zeros(P, 4 + n_feat, device=dev)
    o.d_feat = o.d_featx[:, 4:]
    o.d_x3 = f(P, 3)
