"""torch.autograd bindings of the HIP entry points (include/dns_hip.h).

PyTorch is plumbing here: device buffers, the current stream and the autograd graph.  All arithmetic
happens in libdns_hip.so; nothing in this module has a CPU or eager-torch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import os

import numpy as np
import torch

from ._lib import DnsGridMeta, check, lib as _rawlib, ptr, require_cuda, stream_ptr


class _TimedLib:
    """Pass-through to libdns_hip.so that, when ``ops.timer`` is armed, brackets every launch-carrying entry point
    with events on the current stream (the stream the kernels are launched on) -- bench.py's per-kernel durations."""

    def __init__(self, raw):
        self._raw = raw
        self.records = None          # list of (name, start_event, end_event, units, key arguments, kernel-span range) while armed
        self.kernels = False         # also collect the library's per-kernel spans (dns_kernel_timing)

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if self.records is None or name in ("dns_grid_meta_init", "dns_mlp_bwd_ws_floats", "dns_mlp_prepared_floats", "dns_encode_bwd_ws_floats", "dns_raygen_bwd_ws_floats", "dns_last_error",
                                            "dns_abi_version", "dns_init") or name.startswith("dns_kernel_timing"):
            return fn

        ui = self._UNITS_ARG.get(name)
        info_of = self._INFO.get(name)

        def timed(*a):
            k0 = self._raw.dns_kernel_timing_count() if self.kernels else 0
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            k1 = self._raw.dns_kernel_timing_count() if self.kernels else 0
            units = 0 if ui is None else (a[ui] if not isinstance(ui, tuple) else a[ui[0]] * a[ui[1]])
            self.records.append((name, e0, e1, int(units), info_of(a) if info_of else None, (k0, k1)))
            return rc
        return timed

    # per-call facts the roofline needs: the network shape of an MLP launch and which gradients it produces
    # (n_in = the LIVE input width: with DNS_MLP_LIVE_IN the kernels skip the identically-zero columns, and the roofline counts
    #  the work that is done, not the multiplications by zero the reference's full-width GEMM performs)
    _live = staticmethod(lambda n_in, flags: ((int(flags) >> 16) & 0xff) or n_in)
    @staticmethod
    def _grid_info(meta_ref):
        """levels of a grid and how many of them the scatter sends through pair lists (hashed levels of more than one 8192-row
        chunk, dense levels of at least six: csrc/scatter_plan.hpp list_plan)"""
        m = getattr(meta_ref, "_obj", None)
        if m is None:
            return None
        L = int(m.n_levels)
        in_lists = lambda l: 8192 < m.size[l] <= (1 << 20) and (m.hashed[l] or (m.size[l] + 8191) // 8192 >= 6)
        return {"n_levels": L, "list_levels": sum(1 for l in range(L) if in_lists(l))}

    _INFO = {"dns_encode_bwd": lambda a: _TimedLib._grid_info(a[5]),
             "dns_mlp_fwd": lambda a: {"n_in": _TimedLib._live(a[6], a[17]), "n_out": a[7], "nn": a[8], "nl": a[9]},
             "dns_mlp_dwin": lambda a: {"n_in": _TimedLib._live(a[5], a[14]), "n_out": 0, "nn": a[6], "nl": a[7]},
             "dns_mlp_bwd": lambda a: {"n_in": _TimedLib._live(a[8], a[23]), "n_out": a[9], "nn": a[10], "nl": a[11], "dx": bool(a[12]),
                                       "dw": bool(a[16])},
             "dns_mlp_fwd_half": lambda a: {"n_in": _TimedLib._live(a[6], a[16]), "n_out": a[7], "nn": a[8], "nl": a[9]},
             "dns_mlp_bwd_half": lambda a: {"n_in": _TimedLib._live(a[8], a[21]), "n_out": a[9], "nn": a[10], "nl": a[11], "dx": bool(a[12]),
                                            "dw": bool(a[16]), "dx_from": (int(a[21]) >> 24) & 0x7f, "acc": int(a[21]) & 3},
             "dns_mlp_fwd_split": lambda a: {"n_in": a[4], "n_out": a[5], "nn": a[6], "nl": a[7]},
             "dns_mlp_bwd_split": lambda a: {"n_in": a[6], "n_out": a[7], "nn": a[8], "nl": a[9], "dx": bool(a[10]), "dw": bool(a[14])}}

    # argument index holding the number of units (points / slots / rays) a launch processes
    _UNITS_ARG = {"dns_encode_fwd": 2, "dns_encode_bwd": 2, "dns_mlp_fwd": 12, "dns_mlp_bwd": 18,
                  "dns_composite_fwd": 3, "dns_composite_bwd": 3, "dns_raygen_sample": (14, 15), "dns_raygen_bwd": (7, 8),
                  "dns_rays_from_pixels": 12, "dns_mlp_dwin": 10, "dns_feature_block": (7, 8), "dns_loss_sums": (1, 2),
                  "dns_loss_bwd": (1, 2), "dns_loss_rays": (1, 2), "dns_loss_finalize_bwd": (1, 2), "dns_raw_bwd": 2, "dns_rgb_sigmoid": 1, "dns_class_slots": (1, 2),
                  "dns_hashgrid_indices": 1, "dns_sample_along_rays": 2, "dns_feature_gather": (4, 5),
                  "dns_encode_fwd_split": 2, "dns_mlp_fwd_half": 12, "dns_mlp_bwd_half": 17, "dns_mlp_fwd_split": 10, "dns_mlp_bwd_split": 16, "dns_feature_block_split": (9, 10),
                  "dns_composite_fwd_ex": 3, "dns_composite_bwd_ex": 3, "dns_loss_bwd_points": (1, 2)}

    def arm(self, kernels=False):
        self.kernels = bool(kernels)
        if self.kernels:
            check(self._raw.dns_kernel_timing(1), "dns_kernel_timing")
        self.records = []

    def disarm(self):
        """-> {entry point: (calls, total_ms, total_units)}; call after a device synchronise.  With ``arm(kernels=True)``
        ``self.kernel_spans`` then holds one ``(entry point, kernel, ms, units, info)`` per kernel launch."""
        recs, self.records = self.records or [], None
        out = {}
        spans = []
        if self.kernels:
            check(self._raw.dns_kernel_timing(0), "dns_kernel_timing")
            buf, ms = C.create_string_buffer(160), C.c_float()
        for name, e0, e1, units, info, (k0, k1) in recs:
            c, t, u = out.get(name, (0, 0.0, 0))
            out[name] = (c + 1, t + e0.elapsed_time(e1), u + units)
            for k in range(k0, k1):
                check(self._raw.dns_kernel_timing_get(k, buf, 160, C.byref(ms)), "dns_kernel_timing_get")
                spans.append((name, buf.value.decode().strip("()"), float(ms.value), units, info))
        self.kernel_spans, self.kernels = spans, False
        return out


lib = _TimedLib(_rawlib)
timer = lib


# ----------------------------------------------------------------------------- grid meta
class GridMeta:
    """Host-side hash-grid level table (tcnn GridEncoding constructor; reference call site
    models/pos_encoding.py:31-46).  ``per_level_scale`` follows pos_encoding.py:33 in float64."""

    def __init__(self, log2_hashmap_size: int, desired_resolution: int, n_levels: int = 16,
                 n_features: int = 2, base_resolution: int = 16, per_level_scale: Optional[float] = None):
        if per_level_scale is None:
            per_level_scale = float(np.exp2(np.log2(desired_resolution / base_resolution) / (n_levels - 1)))
        self.c = DnsGridMeta()
        check(lib.dns_grid_meta_init(C.byref(self.c), n_levels, n_features, log2_hashmap_size, base_resolution,
                                     per_level_scale), "dns_grid_meta_init")
        self.n_levels = n_levels
        self.n_features = n_features
        self.total_rows = int(self.c.total_rows)
        self.out_dim = n_levels * n_features
        self._args = (log2_hashmap_size, desired_resolution, n_levels, n_features, base_resolution, per_level_scale)

    def levels(self):
        c = self.c
        return [dict(scale=np.float32(c.scale[l]), resolution=int(c.resolution[l]), size=int(c.size[l]),
                     offset=int(c.offset[l]), hashed=bool(c.hashed[l])) for l in range(self.n_levels)]

    # picklable (spawn / torch.save / deepcopy of modules that own one)
    def __getstate__(self):
        return {"args": self._args}

    def __setstate__(self, st):
        a = st["args"]
        self.__init__(a[0], a[1], a[2], a[3], a[4], a[5])


def _bound6(bound) -> Optional[C.Array]:
    """[3,2] float64 bound -> 6 host doubles b0x,b1x,b0y,b1y,b0z,b1z."""
    if bound is None:
        return None
    if isinstance(bound, C.Array):
        return bound
    cached = getattr(bound, "_dns_b6", None) if isinstance(bound, torch.Tensor) else None
    if cached is not None:
        return cached
    b = torch.as_tensor(bound, dtype=torch.float64).detach().cpu().reshape(3, 2)   # one sync, then cached on the tensor
    b6 = (C.c_double * 6)(*[float(v) for v in b.reshape(-1)])
    if isinstance(bound, torch.Tensor):
        try:
            bound._dns_b6 = b6
        except Exception:
            pass
    return b6


# ----------------------------------------------------------------------------- encoding
# (form, queue_cap) of the table-gradient scatter, include/dns_hip.h DNS_SCATTER_*: 0 auto (pair lists for the hashed levels, LDS
# sweep / queues for the dense ones), 1 per-corner atomics (tcnn's form), 2 LDS sweep for every level, 3 per-chunk queues for
# every multi-chunk level; queue_cap 0 = sized by the library
SCATTER_AUTO, SCATTER_ATOMIC, SCATTER_BINNED, SCATTER_QUEUES = 0, 1, 2, 3
SCATTER_REPLAY = 0x10       # include/dns_hip.h DNS_SCATTER_REPLAY: hashed levels' corner rows stored once, replayed by the chunk visits
SCATTER_LISTS = 0x20        # include/dns_hip.h DNS_SCATTER_LISTS (implied by auto): hashed levels through per-chunk lists of {point, corner pair} words
SCATTER_FORM = (SCATTER_AUTO | (SCATTER_REPLAY if os.environ.get("DNS_SCATTER_REPLAY", "0") == "1" else 0)
                | (SCATTER_LISTS if os.environ.get("DNS_SCATTER_LISTS", "0") == "1" else 0), 0)
SAVE_DY_DX = True           # encode forward keeps d(grid)/dx when the points need a gradient (False: the backward re-gathers)


class _EncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, table, meta: Optional[GridMeta], bound, n_bins: int, want_pe: bool, want_grid: bool):
        require_cuda(pts, table)
        P = pts.shape[0]
        pts = pts.contiguous().float()
        pe_dim = 3 * n_bins if want_pe else 0
        g_dim = meta.out_dim if want_grid else 0
        ld = pe_dim + g_dim
        out = torch.empty(P, ld, device=pts.device, dtype=torch.float32)
        b6 = _bound6(bound)
        x = torch.empty(P, 3, device=pts.device, dtype=torch.float32) if b6 is not None else pts
        pe_ptr = ptr(out) if want_pe else None
        grid_ptr = C.c_void_p(out.data_ptr() + 4 * pe_dim) if want_grid else None
        # the points need a gradient (poses, through pts): keep d(grid features)/dx like tcnn does -- 384 B per
        # point written here instead of a second 8-corner gather per level in the backward
        dydx = torch.empty(meta.n_levels * 3 * P * 2, device=pts.device, dtype=torch.float32) \
            if (want_grid and pts.requires_grad and SAVE_DY_DX) else None
        check(lib.dns_encode_fwd(ptr(pts), b6, P, n_bins, ptr(table) if want_grid else None,
                                 C.byref(meta.c) if want_grid else None,
                                 ptr(x) if b6 is not None else None, pe_ptr, ld, grid_ptr, ld, ptr(dydx), stream_ptr()),
              "dns_encode_fwd")
        ctx.save_for_backward(x, table if want_grid else None, dydx)
        ctx.meta, ctx.b6, ctx.n_bins, ctx.pe_dim, ctx.g_dim = meta, b6, n_bins, pe_dim, g_dim
        ctx.need_x = pts.requires_grad
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, table, dydx = ctx.saved_tensors
        P = x.shape[0]
        d_out = d_out.contiguous()
        ld = ctx.pe_dim + ctx.g_dim
        need_x = ctx.needs_input_grad[0]
        need_t = ctx.g_dim > 0 and ctx.needs_input_grad[1]
        d_x = torch.empty(P, 3, device=x.device, dtype=torch.float32) if need_x else None
        d_table = torch.zeros_like(table) if need_t else None
        d_pe = ptr(d_out) if ctx.pe_dim else None
        d_grid = C.c_void_p(d_out.data_ptr() + 4 * ctx.pe_dim) if ctx.g_dim else None
        form, cap = SCATTER_FORM
        ws = torch.empty(int(lib.dns_encode_bwd_ws_floats(P, C.byref(ctx.meta.c), form, cap)), device=x.device,
                         dtype=torch.float32) if need_t else None
        check(lib.dns_encode_bwd(ptr(x), ctx.b6, P, ctx.n_bins, ptr(table) if ctx.g_dim else None,
                                 C.byref(ctx.meta.c) if ctx.g_dim else None, d_pe, ld, d_grid, ld,
                                 ptr(d_table), ptr(d_x), ptr(dydx) if need_x else None, ptr(ws), form, cap, stream_ptr()),
              "dns_encode_bwd")
        return d_x, d_table, None, None, None, None, None


def encode(pts: torch.Tensor, table: Optional[torch.Tensor], meta: Optional[GridMeta], bound=None, n_bins: int = 16,
           want_pe: bool = True, want_grid: bool = True) -> torch.Tensor:
    """[P,3] -> [P, 3*n_bins (+) L*F] (OneBlob channels first).  With ``bound`` the input is world points and
    the fp64 normalisation of slams/mapping.py:608 happens in-kernel."""
    if table is None:
        table = pts.new_zeros(1)
    return _EncodeFn.apply(pts, table, meta, bound, n_bins, want_pe, want_grid)


def hashgrid_rows(x: torch.Tensor, meta: GridMeta) -> torch.Tensor:
    """Debug/parity: absolute table rows [P, L, 8] (int64) of the corners the kernel gathers."""
    require_cuda(x)
    x = x.contiguous().float()
    rows = torch.empty(x.shape[0], meta.n_levels, 8, device=x.device, dtype=torch.int32)
    check(lib.dns_hashgrid_indices(ptr(x), x.shape[0], C.byref(meta.c), ptr(rows), stream_ptr()), "dns_hashgrid_indices")
    return rows.to(torch.int64) & 0xFFFFFFFF


# ----------------------------------------------------------------------------- MLP
def mlp_out_padded(n_out: int) -> int:
    return (n_out + 15) // 16 * 16


def mlp_param_count(n_in: int, n_out: int, n_neurons: int, n_hidden_layers: int) -> int:
    return n_neurons * n_in + (n_hidden_layers - 1) * n_neurons * n_neurons + mlp_out_padded(n_out) * n_neurons


def _row_major_2d(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
        if x.data_ptr() % 16 != 0:
            x = x.clone()
    return x


# The backward recomputes the hidden activations (two layers of f16 matrix instructions cost less than reading 512 B per
# point back from HBM): the forward keeps nothing.  True = dns_mlp_fwd also writes them (h_save; inspection only).
LOSS_SUMS_FLOATS = 32 + 5 * 1024          # include/dns_hip.h DNS_LOSS_SUMS_FLOATS
MLP_SAVE_HIDDEN = False
MLP_FP16_FLAG = 0x100                      # include/dns_hip.h DNS_MLP_FP16
MLP_PREPARED_FLAG = 0x200                  # include/dns_hip.h DNS_MLP_PREPARED
MLP_NO_DWIN_FLAG = 0x400                   # include/dns_hip.h DNS_MLP_NO_DWIN
MLP_DX_FIRST_FLAG = 0x800                  # include/dns_hip.h DNS_MLP_DX_FIRST
MLP_DX_FROM = lambda c: int(c) << 24       # include/dns_hip.h DNS_MLP_DX_FROM(c): no input gradient for columns [0, c)
MLP_LIVE_IN = lambda n: int(n) << 16       # include/dns_hip.h DNS_MLP_LIVE_IN(n): input columns [n, n_in) are identically zero


# ---- the MLP entry points on fp32 and half rows, each spelled positionally ONCE inside the package (the split-row pair: launch.
# SplitRows; tests and tools keep direct calls: they exercise the ABI).  Tensors or None in; the pointers, the row strides and the
# zero stride of an absent tensor are formed here.  ``lib`` is read at call time, so a timer armed after a step was built still
# brackets every launch (bench.py's per-kernel table).  ``shape`` = (n_in, n_out, n_neurons, n_hidden_layers).
def launch_mlp_fwd(x, x2, n_in1, w, shape, y, n_slots, row_index, tile_group, stride, h_save, flags, st):
    check(lib.dns_mlp_fwd(ptr(x), x.stride(0), ptr(x2), 0 if x2 is None else x2.stride(0), n_in1, ptr(w), *shape, ptr(y), y.stride(0),
                          n_slots, ptr(row_index), ptr(tile_group), stride, ptr(h_save), flags, st), "dns_mlp_fwd")


def launch_mlp_bwd(x, x2, n_in1, dy, w, shape, d_x, d_x2, d_params, ws, n_slots, row_index, tile_group, stride, h_saved, flags, st):
    check(lib.dns_mlp_bwd(ptr(x), x.stride(0), ptr(x2), 0 if x2 is None else x2.stride(0), n_in1, ptr(dy), dy.stride(0), ptr(w),
                          *shape, ptr(d_x), 0 if d_x is None else d_x.stride(0), ptr(d_x2), 0 if d_x2 is None else d_x2.stride(0),
                          ptr(d_params), ptr(ws), n_slots, ptr(row_index), ptr(tile_group), stride, ptr(h_saved), flags, st),
          "dns_mlp_bwd")


def launch_mlp_dwin(x, x2, n_in1, shape, d_params, ws, n_slots, row_index, tile_group, stride, flags, st):
    check(lib.dns_mlp_dwin(ptr(x), x.stride(0), ptr(x2), 0 if x2 is None else x2.stride(0), n_in1, shape[0], shape[2], shape[3],
                           ptr(d_params), ptr(ws), n_slots, ptr(row_index), ptr(tile_group), stride, flags, st), "dns_mlp_dwin")


def launch_mlp_fwd_half(x, x2, n_in1, w, shape, y, n_slots, row_index, tile_group, stride, flags, st, ldx2=0):
    """``ldx2``: what an ABSENT x2 passes as its row stride (MapStep's single-segment launches have always passed their feature
    block's width there; the kernels read it with x2 alone)."""
    check(lib.dns_mlp_fwd_half(ptr(x), x.stride(0), ptr(x2), ldx2 if x2 is None else x2.stride(0), n_in1, ptr(w), *shape, ptr(y),
                               y.stride(0), n_slots, ptr(row_index), ptr(tile_group), stride, flags, st), "dns_mlp_fwd_half")


def launch_mlp_bwd_half(x, x2, n_in1, dy, w, shape, d_x, d_x2, d_params, n_slots, row_index, tile_group, stride, flags, loss_scale,
                        st, ldx2=0):
    check(lib.dns_mlp_bwd_half(ptr(x), x.stride(0), ptr(x2), ldx2 if x2 is None else x2.stride(0), n_in1, ptr(dy), dy.stride(0),
                               ptr(w), *shape, ptr(d_x), 0 if d_x is None else d_x.stride(0), ptr(d_x2),
                               0 if d_x2 is None else d_x2.stride(0), ptr(d_params), n_slots, ptr(row_index), ptr(tile_group),
                               stride, flags, loss_scale, st), "dns_mlp_bwd_half")


class _MlpFn(torch.autograd.Function):
    """y = MLP(x; params).  ``params`` is [G, count] (G weight sets, G=1 for a plain network)."""

    @staticmethod
    def forward(ctx, x, params, shape, row_index, tile_group, n_slots):
        n_in, n_out, nn, nl = shape[:4]
        fp16 = MLP_FP16_FLAG if (len(shape) > 4 and shape[4]) else 0
        require_cuda(params, row_index, tile_group)
        if not x.is_cuda:
            raise ValueError("dns_slam_amd ops run on the GPU only (got a non-CUDA tensor); there is no CPU fallback")
        x = _row_major_2d(x.float())
        P = x.shape[0]
        if row_index is None:
            y = torch.empty(P, n_out, device=x.device, dtype=torch.float32)
            n_slots = P
        else:
            y = torch.zeros(P, n_out, device=x.device, dtype=torch.float32)
        stride = params.shape[-1] if params.dim() == 2 else 0
        # keep the hidden activations when a backward will follow: it then skips the forward recompute
        keep = MLP_SAVE_HIDDEN and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        h_save = torch.empty(nl * n_slots * nn, device=x.device, dtype=torch.float32) if keep else None
        launch_mlp_fwd(x, None, 0, params, shape[:4], y, n_slots, row_index, tile_group, stride, h_save, fp16, stream_ptr())
        ctx.save_for_backward(x, params, row_index, tile_group, h_save)
        ctx.shape, ctx.n_slots, ctx.stride, ctx.fp16 = shape[:4], n_slots, stride, fp16
        return y

    @staticmethod
    def backward(ctx, dy):
        x, params, row_index, tile_group, h_save = ctx.saved_tensors
        n_in, n_out, nn, nl = ctx.shape
        dy = dy.contiguous()
        P = x.shape[0]
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if row_index is None:
            d_x = torch.empty(P, n_in, device=x.device, dtype=torch.float32) if need_x else None
        else:
            d_x = torch.zeros(P, n_in, device=x.device, dtype=torch.float32) if need_x else None
        d_p = torch.zeros_like(params) if need_p else None
        ws = torch.empty(int(lib.dns_mlp_bwd_ws_floats(ctx.n_slots, nn, nl)), device=x.device, dtype=torch.float32)
        launch_mlp_bwd(x, None, 0, dy, params, ctx.shape, d_x, None, d_p, ws, ctx.n_slots, row_index, tile_group, ctx.stride, h_save,
                       ctx.fp16, stream_ptr())
        return d_x, d_p, None, None, None, None


class _MlpCatFn(torch.autograd.Function):
    """y = MLP(cat(x1, x2, -1); params) without building the concatenation: the kernels read the two column segments in
    place (dns_mlp_fwd/bwd two-segment input) and write the two input gradients separately."""

    @staticmethod
    def forward(ctx, x1, x2, params, shape):
        n_in, n_out, nn, nl = shape[:4]
        fp16 = MLP_FP16_FLAG if (len(shape) > 4 and shape[4]) else 0
        require_cuda(params)
        if not (x1.is_cuda and x2.is_cuda):
            raise ValueError("dns_slam_amd ops run on the GPU only (got a non-CUDA tensor); there is no CPU fallback")
        x1, x2 = _row_major_2d(x1.float()), _row_major_2d(x2.float())
        P, n1 = x1.shape
        y = torch.empty(P, n_out, device=x1.device, dtype=torch.float32)
        h_save = torch.empty(nl * P * nn, device=x1.device, dtype=torch.float32) if MLP_SAVE_HIDDEN else None
        launch_mlp_fwd(x1, x2, n1, params, shape[:4], y, P, None, None, 0, h_save, fp16, stream_ptr())
        ctx.save_for_backward(x1, x2, params, h_save)
        ctx.shape, ctx.fp16 = shape[:4], fp16
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, params, h_save = ctx.saved_tensors
        n_in, n_out, nn, nl = ctx.shape
        dy = dy.contiguous()
        P, n1 = x1.shape
        need_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        d1 = torch.empty(P, n1, device=x1.device, dtype=torch.float32) if need_x else None
        d2 = torch.empty(P, n_in - n1, device=x1.device, dtype=torch.float32) if need_x else None
        d_p = torch.zeros_like(params) if ctx.needs_input_grad[2] else None
        ws = torch.empty(int(lib.dns_mlp_bwd_ws_floats(P, nn, nl)), device=x1.device, dtype=torch.float32)
        launch_mlp_bwd(x1, x2, n1, dy, params, ctx.shape, d1, d2, d_p, ws, P, None, None, 0, h_save, ctx.fp16, stream_ptr())
        return (d1 if ctx.needs_input_grad[0] else None), (d2 if ctx.needs_input_grad[1] else None), d_p, None


def mlp_cat(x1: torch.Tensor, x2: torch.Tensor, params: torch.Tensor, n_out: int, n_neurons: int = 32,
            n_hidden_layers: int = 1, fp16: bool = False) -> torch.Tensor:
    """``mlp(torch.cat((x1, x2), -1), ...)`` with the concatenation left implicit (models/decoder.py:73,123-124).  Falls
    back to the explicit cat when a segment is not a multiple of 4 columns / 16-byte addressable or wider than 64."""
    n1, n2 = x1.shape[-1], x2.shape[-1]
    ok = (n1 % 4 == 0 and n2 % 4 == 0 and 0 < n1 <= 64 and 0 < n2 <= 64 and x1.dim() == 2 and x2.dim() == 2
          and x1.stride(-1) == 1 and x2.stride(-1) == 1 and x1.stride(0) % 4 == 0 and x2.stride(0) % 4 == 0
          and x1.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0 and x1.dtype == torch.float32 and x2.dtype == torch.float32)
    if not ok:
        return mlp(torch.cat((x1, x2), -1), params, n1 + n2, n_out, n_neurons, n_hidden_layers, fp16)
    return _MlpCatFn.apply(x1, x2, params, (n1 + n2, n_out, n_neurons, n_hidden_layers, bool(fp16)))


def mlp(x: torch.Tensor, params: torch.Tensor, n_in: int, n_out: int, n_neurons: int = 32,
        n_hidden_layers: int = 1, fp16: bool = False) -> torch.Tensor:
    """Bias-free ReLU MLP on the matrix cores (tcnn CutlassMLP replacement): exact fp32, or with ``fp16`` tcnn's own
    precision (fp16 operands, fp32 accumulate; parameters, kept activations and weight gradients stay fp32)."""
    return _MlpFn.apply(x, params, (n_in, n_out, n_neurons, n_hidden_layers, bool(fp16)), None, None, 0)


# ---- half rows (include/dns_hip.h, ABI v12): tcnn's own arithmetic -- f16 activations and weight operands, fp32 accumulation, a
# static loss scale.  Thin, non-autograd wrappers (fused_step.MapStep drives the entry points directly; tests use these).
HALF_LOSS_SCALE = 128.0                       # tcnn's default loss_scale for half-precision networks
SPLIT_PLAIN = 2                               # DNS_SPLIT_PLAIN: dns_encode_fwd_split / dns_feature_block_split write plain f16 rows


def _cuda_rows(*tensors):
    """CUDA tensors with unit column stride (row-strided views are what these entry points take: ld arguments)."""
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("dns_slam_amd ops run on the GPU only (got a non-CUDA tensor); there is no CPU fallback")
        if t.dim() == 2 and t.stride(1) != 1:
            raise ValueError("dns_slam_amd ops need unit column stride")


def _half_rows_ok(t):
    return t is None or (t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1)


def mlp_fwd_half(x, params, n_in, n_out, n_neurons, n_hidden_layers, x2=None, row_index=None, tile_group=None, n_slots=None,
                 param_stride=0, live_in=0, out=None):
    """y = MLP(x | x2) on f16 rows (dns_mlp_fwd_half): x [rows, >= n_in1] / x2 [rows, >= n_in - n_in1] float16, params fp32 (a pool
    [G, stride] with tile_group), y fp32 [rows, n_out].  ``live_in``: DNS_MLP_LIVE_IN width (0 = n_in)."""
    _cuda_rows(x, x2, out)
    require_cuda(params)
    if not (_half_rows_ok(x) and _half_rows_ok(x2)):
        raise ValueError("mlp_fwd_half: x / x2 must be 2-D float16 CUDA tensors with unit column stride")
    rows = x.shape[0]
    n_slots = rows if n_slots is None else n_slots
    y = out if out is not None else torch.zeros(rows, n_out, device=x.device, dtype=torch.float32)
    n_in1 = x.shape[1] if x2 is not None else 0
    launch_mlp_fwd_half(x, x2, n_in1, params, (n_in, n_out, n_neurons, n_hidden_layers), y, n_slots, row_index, tile_group, param_stride,
                        MLP_LIVE_IN(live_in) if live_in else 0, stream_ptr())
    return y


def mlp_bwd_half(x, dy, params, n_in, n_out, n_neurons, n_hidden_layers, x2=None, d_x=None, d_x2=None, d_params=None, row_index=None,
                 tile_group=None, n_slots=None, param_stride=0, accumulate=0, loss_scale=HALF_LOSS_SCALE):
    """Input and weight gradients of the same network (dns_mlp_bwd_half; ONE kernel, dW_in included).  dy fp32 [rows, n_out];
    d_x / d_x2 fp32 (None = skip), d_params fp32 like params (+=; None = skip).  ``accumulate``: the entry point's accumulate_dx
    word (bits 0 / 1, MLP_DX_FIRST_FLAG, MLP_LIVE_IN(n), MLP_DX_FROM(c))."""
    _cuda_rows(x, x2, dy, d_x, d_x2)
    require_cuda(params, d_params)
    if not (_half_rows_ok(x) and _half_rows_ok(x2)):
        raise ValueError("mlp_bwd_half: x / x2 must be 2-D float16 CUDA tensors with unit column stride")
    n_slots = x.shape[0] if n_slots is None else n_slots
    n_in1 = x.shape[1] if x2 is not None else 0
    launch_mlp_bwd_half(x, x2, n_in1, dy, params, (n_in, n_out, n_neurons, n_hidden_layers), d_x, d_x2, d_params, n_slots, row_index,
                        tile_group, param_stride, int(accumulate), float(loss_scale), stream_ptr())


def group_slots(slot_of_point: torch.Tensor, n_groups: int, min_count: int = 2):
    """Device-side (sync-free) layout for the grouped MLP: points counting-sorted by weight-set id into 128-slot tiles
    (dns_group_slots).  ``slot_of_point`` [P] int64 in [0, n_groups) (negative = no network).  Returns (row_index
    int32 [n_slots], tile_group int32 [n_slots/128], n_slots).  Groups with fewer than ``min_count`` points are
    skipped, as ``Mapper.fine_fn`` does (slams/mapping.py:597: ``if index.sum() > 1``)."""
    require_cuda(slot_of_point)
    slot_of_point = slot_of_point.contiguous()
    if slot_of_point.dtype != torch.int64:
        slot_of_point = slot_of_point.to(torch.int64)
    P = slot_of_point.shape[0]
    dev = slot_of_point.device
    n_slots = (P + 127) // 128 * 128 + 128 * n_groups
    row_index = torch.empty(n_slots, device=dev, dtype=torch.int32)
    tile_group = torch.empty(n_slots // 128, device=dev, dtype=torch.int32)
    ws = torch.empty(512, device=dev, dtype=torch.int32)
    check(lib.dns_group_slots(ptr(slot_of_point), P, n_groups, min_count, n_slots, ptr(ws), ptr(row_index), ptr(tile_group),
                              stream_ptr()), "dns_group_slots")
    return row_index, tile_group, n_slots


def mlp_grouped(x: torch.Tensor, params_pool: torch.Tensor, slot_of_point: torch.Tensor, n_in: int, n_out: int,
                n_neurons: int = 32, n_hidden_layers: int = 1, min_count: int = 2, fp16: bool = False) -> torch.Tensor:
    """Per-point weight sets (the per-class fine decoders, slams/mapping.py:590-601): point p runs through
    ``params_pool[slot_of_point[p]]``; points with no network / tiny groups get zeros."""
    G = params_pool.shape[0]
    row_index, tile_group, n_slots = group_slots(slot_of_point, G, min_count)
    return _MlpFn.apply(x, params_pool, (n_in, n_out, n_neurons, n_hidden_layers, bool(fp16)), row_index, tile_group, n_slots)


# ----------------------------------------------------------------------------- the renderer's four networks, fused glue
class _RenderNetsFn(torch.autograd.Function):
    """Coarse + per-class fine + colour + logit networks of ``Mapper.renderer`` (slams/mapping.py:616-626) as ONE
    autograd node.  Same kernels as ``mlp`` / ``mlp_grouped``; what it removes is glue traffic:
      * the colour / logit input ``cat(pe, cat(fine[:, 1:], pixel))`` (models/decoder.py:123-124) is never built: the
        networks read the pe columns of ``buf`` and the [P, 64] feature block as a two-segment input;
      * in the backward every network adds its input gradient in place (accumulate_dx) into one d_buf / d_feat pair
        instead of autograd materialising one [P, 80] / [P, 112] gradient per consumer and summing them;
      * the compositing input ``cat(sigmoid(colour), fine[:, 0:1])`` (slams/mapping.py:622-627) is an output of the node
        (the colour network writes into its rows), so neither the cat nor the [P, h+1] zero-padded gradient of the
        ``fine[:, 0:1]`` slice and its sum with the losses' gradient exist.
    buf: [P, pe_dim + grid_dim] (OneBlob | hash grid), pixel: [P, C] 2-D feature code."""

    @staticmethod
    def forward(ctx, buf, pixel, coarse_p, fine_pool, color_p, logit_p, slot_of_point, cfg):
        pe_dim, shp_c, shp_f, shp_col, shp_log, min_count, fp16, n_groups = cfg[:8]
        need_coarse = cfg[8] if len(cfg) > 8 else True
        fp16 = MLP_FP16_FLAG if fp16 else 0
        require_cuda(buf, pixel, coarse_p, fine_pool, color_p, logit_p, slot_of_point)
        buf = _row_major_2d(buf.float())
        pixel = pixel.float()
        P, dev = buf.shape[0], buf.device
        keep = MLP_SAVE_HIDDEN
        st = stream_ptr()

        def run(x, x2, n_in1, params, shape, y, ri, tg, n_slots, stride, live=0):
            h = torch.empty(shape[3] * n_slots * shape[2], device=dev, dtype=torch.float32) if keep else None
            launch_mlp_fwd(x, x2, n_in1, params, shape, y, n_slots, ri, tg, stride, h, fp16 | live, st)
            return h

        # (need_coarse = False: the forward-only frame render, slams/mapping.py:638-694 -- the coarse latents feed the latent
        #  loss alone, mapping.py:893-896, and frame_vis drops them: one of the four networks is not run)
        coarse = torch.empty(P if need_coarse else 0, shp_c[1], device=dev, dtype=torch.float32)
        h_c = run(buf, None, 0, coarse_p, shp_c, coarse, None, None, P, 0) if need_coarse else None
        ri, tg, n_slots = group_slots(slot_of_point, n_groups or fine_pool.shape[0], min_count)
        fine = torch.zeros(P, shp_f[1], device=dev, dtype=torch.float32)
        h_f = run(buf, None, 0, fine_pool, shp_f, fine, ri, tg, n_slots, fine_pool.shape[-1])
        if pixel.shape[1] == 0 and not torch.is_grad_enabled():
            # forward-only, no 2-D code: the colour / logit networks read the latent straight out of the fine rows (second input
            # segment = fine[:, 1:], row stride hidden + 1: dns_mlp_fwd takes a 4-byte aligned slice) -- no [P, hidden] copy
            # (537 MB written and read again per 65 536-ray chunk of a frame render)
            feat = fine[:, 1:]
        else:
            feat = torch.cat((fine[:, 1:], pixel), -1)                    # [P, hidden + C]
        # A code of ZERO columns (forward-only callers without a 2-D code: the reference multiplies a zero code through,
        # slams/mapping.py:553-557): the colour / logit networks run as their live (pe + hidden)-input networks, DNS_MLP_LIVE_IN
        live = 0
        if pe_dim + feat.shape[1] < shp_col[0]:
            if torch.is_grad_enabled() or (pe_dim + feat.shape[1]) % 8 != 0:
                raise ValueError("render_nets: a code narrower than the networks' input is a forward-only form (no_grad, multiple of 8)")
            live = MLP_LIVE_IN(pe_dim + feat.shape[1])
        # raw = (sigmoid(colour) | occupancy) = the compositing kernel's input (slams/mapping.py:622-627): the colour
        # network writes its three columns straight into the [P, 4] rows
        raw = torch.empty(P, 4, device=dev, dtype=torch.float32)
        logit = torch.empty(P, shp_log[1], device=dev, dtype=torch.float32)
        h_col = run(buf, feat, pe_dim, color_p, shp_col, raw, None, None, P, 0, live)
        h_log = run(buf, feat, pe_dim, logit_p, shp_log, logit, None, None, P, 0, live)
        raw.sigmoid_()                                                    # column 3 is not written yet
        raw[:, 3] = fine[:, 0]
        ctx.save_for_backward(buf, feat, coarse_p, fine_pool, color_p, logit_p, ri, tg, h_c, h_f, h_col, h_log, raw)
        ctx.cfg, ctx.n_slots, ctx.pixel_dim = cfg, n_slots, pixel.shape[1]
        ctx.set_materialize_grads(False)
        return coarse, fine, raw, logit

    @staticmethod
    def backward(ctx, d_coarse, d_fine, d_raw, d_logit):
        buf, feat, coarse_p, fine_pool, color_p, logit_p, ri, tg, h_c, h_f, h_col, h_log, raw = ctx.saved_tensors
        pe_dim, shp_c, shp_f, shp_col, shp_log, _, fp16, _ = ctx.cfg[:8]
        if len(ctx.cfg) > 8 and not ctx.cfg[8]:
            raise RuntimeError("render_nets(need_coarse=False) is forward-only")
        fp16 = MLP_FP16_FLAG if fp16 else 0
        P, dev = buf.shape[0], buf.device
        st = stream_ptr()
        need_buf = ctx.needs_input_grad[0]
        need_pix = ctx.needs_input_grad[1]
        d_buf = torch.empty_like(buf)
        # [P, 4 + hidden + C]: column 3 = d occupancy (from raw), columns 4.. = the feature-block gradient of the colour
        # and logit networks, so that columns 3..3+hidden are the fine network's output gradient in ONE strided view
        n_f = shp_f[1]
        d_featx = torch.empty(P, 4 + feat.shape[1], device=dev, dtype=torch.float32)
        d_feat = d_featx[:, 4:]

        # one zero-fill for the four parameter gradients (they are views of one buffer)
        need = [ctx.needs_input_grad[i] for i in (2, 3, 4, 5)]
        sizes = [p.numel() if n else 0 for p, n in zip((coarse_p, fine_pool, color_p, logit_p), need)]
        flat = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
        offs = [sum(sizes[:i]) for i in range(4)]
        dps = {id(p): (flat[o:o + z].view_as(p) if n else None)
               for p, o, z, n in zip((coarse_p, fine_pool, color_p, logit_p), offs, sizes, need)}

        def run(x, x2, n_in1, dy, params, shape, d_x, d_x2, need_p, ri_, tg_, n_slots, stride, h, acc):
            d_p = dps[id(params)] if need_p else None
            ws = torch.empty(int(lib.dns_mlp_bwd_ws_floats(n_slots, shape[2], shape[3])), device=dev, dtype=torch.float32)
            launch_mlp_bwd(x, x2, n_in1, dy, params, shape, d_x, d_x2, d_p, ws, n_slots, ri_, tg_, stride, h, acc | fp16, st)
            return d_p

        def grad(d, like_cols):
            return torch.zeros(P, like_cols, device=dev) if d is None else _row_major_2d(d.float())

        # 1. coarse: writes all columns of d_buf
        d_cp = run(buf, None, 0, grad(d_coarse, shp_c[1]), coarse_p, shp_c, d_buf, None, ctx.needs_input_grad[2],
                   None, None, P, 0, h_c, 0)
        # 2./3. colour then logit: pe columns of d_buf (+=), feature block d_feat (=, then +=).  The colour network's
        # output gradient is the sigmoid's: d_raw * s * (1 - s) on the whole [P, 4] rows (column 3 is not read, lddy 4)
        if d_raw is None:
            d_col = torch.zeros(P, 4, device=dev)
            d_featx[:, 3] = 0
        else:
            d_raw = d_raw.contiguous().float()
            d_col = torch.ops.aten.sigmoid_backward(d_raw, raw)
            d_featx[:, 3] = d_raw[:, 3]
        d_colp = run(buf, feat, pe_dim, d_col, color_p, shp_col, d_buf, d_feat,
                     ctx.needs_input_grad[4], None, None, P, 0, h_col, 1)
        d_logp = run(buf, feat, pe_dim, grad(d_logit, shp_log[1]), logit_p, shp_log, d_buf, d_feat,
                     ctx.needs_input_grad[5], None, None, P, 0, h_log, 3)
        # 4. fine: its output gradient = the caller's + d occupancy + what colour / logit sent back through the features
        d_ft = d_featx[:, 3:3 + n_f]
        if d_fine is not None:
            d_ft = d_fine.float() + d_ft
        d_fp = run(buf, None, 0, d_ft, fine_pool, shp_f, d_buf, None, ctx.needs_input_grad[3], ri, tg, ctx.n_slots,
                   fine_pool.shape[-1], h_f, 1)
        d_pix = d_feat[:, n_f - 1:] if need_pix else None
        return (d_buf if need_buf else None), d_pix, d_cp, d_fp, d_colp, d_logp, None, None


def render_nets(buf, pixel, coarse_p, fine_pool, color_p, logit_p, slot_of_point, pe_dim, shp_coarse, shp_fine,
                shp_color, shp_logit, min_count=2, fp16=False, n_groups=None, need_coarse=True):
    """-> (coarse [P, h+1], fine [P, h+1], raw [P, 4] = (sigmoid(colour), fine[:, 0]) -- the compositing input --,
    logits [P, n_class]); shapes are (n_in, n_out, n_neurons, n_hidden_layers) tuples (colour n_out = 3).  n_groups: only
    the first n_groups weight sets of fine_pool are in use (slot_of_point < n_groups) -- pass the whole pool rather than
    a slice of it and autograd has no [capacity, n_params] slice gradient to zero-fill and copy into."""
    cfg = (int(pe_dim), tuple(shp_coarse), tuple(shp_fine), tuple(shp_color), tuple(shp_logit), int(min_count), bool(fp16),
           None if n_groups is None else int(n_groups), bool(need_coarse))
    return _RenderNetsFn.apply(buf, pixel, coarse_p, fine_pool, color_p, logit_p, slot_of_point, cfg)


# ----------------------------------------------------------------------------- compositing
class _CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, z, logits):
        require_cuda(raw, z, logits)
        raw = raw.contiguous().float()
        z = z.contiguous().float()
        N, S = z.shape
        Cn = 0 if logits is None else logits.shape[-1]
        if logits is not None:
            logits = logits.contiguous().float()
        dev = raw.device
        depth = torch.empty(N, device=dev)
        var = torch.empty(N, device=dev)
        rgb = torch.empty(N, 3, device=dev)
        weights = torch.empty(N, S, device=dev)
        sem = torch.empty(N, Cn, device=dev) if Cn else None
        check(lib.dns_composite_fwd(ptr(raw), ptr(z), ptr(logits), N, S, Cn, ptr(depth), ptr(var), ptr(rgb),
                                    ptr(weights), ptr(sem), stream_ptr()), "dns_composite_fwd")
        ctx.save_for_backward(raw, z, logits)
        ctx.dims = (N, S, Cn)
        ctx.set_materialize_grads(False)                  # unused outputs (var, weights, ...) arrive as None, not zeros
        if sem is None:
            sem = raw.new_zeros(N, 0)
        return depth, var, rgb, weights, sem

    @staticmethod
    def backward(ctx, d_depth, d_var, d_rgb, d_weights, d_sem):
        raw, z, logits = ctx.saved_tensors
        N, S, Cn = ctx.dims
        d_raw = torch.empty_like(raw)
        d_logits = torch.empty_like(logits) if Cn else None
        c = lambda t: None if t is None else t.contiguous()
        check(lib.dns_composite_bwd(ptr(raw), ptr(z), ptr(logits), N, S, Cn, ptr(c(d_depth)), ptr(c(d_var)),
                                    ptr(c(d_rgb)), ptr(c(d_weights)), ptr(c(d_sem)) if Cn else None, ptr(d_raw),
                                    ptr(d_logits), stream_ptr()), "dns_composite_bwd")
        return d_raw, None, d_logits


def composite(raw: torch.Tensor, z_vals: torch.Tensor, logits: Optional[torch.Tensor] = None):
    """raw [N,S,4], z [N,S], logits [N,S,C] -> depth [N], var [N], rgb [N,3], weights [N,S], sem [N,C]."""
    return _CompositeFn.apply(raw, z_vals, logits)


# ----------------------------------------------------------------------------- ray generation + sampling
class _RaygenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, quat, trans, pix_idx, color, depth, label, cam, bound, window, npf, t_uniform, t_surf, t_zero,
                depth_max=None):
        require_cuda(quat, trans, pix_idx, color, depth, label, t_uniform, t_surf, t_zero)
        K, H, W = depth.shape
        H0, H1, W0, W1 = window
        n = K * npf
        nu = 0 if t_uniform is None else t_uniform.numel()
        ns = t_surf.shape[-1]
        if t_surf.dim() == 2 and (t_surf.shape != (K, ns) or t_zero.shape != (K, ns)):
            raise ValueError("per-frame jitter must be [K, n_surface] for both draws")
        jstride = ns if t_surf.dim() == 2 else 0               # [K, ns]: frame f samples with its own jitter rows
        S = nu + ns
        dev = quat.device
        quat = quat.contiguous().float()
        trans = trans.contiguous().float()
        rays_o = torch.empty(n, 3, device=dev)
        rays_d = torch.empty(n, 3, device=dev)
        gt_color = torch.empty(n, 3, device=dev)
        gt_depth = torch.empty(n, device=dev)
        gt_label = torch.empty(n, device=dev, dtype=torch.int64)
        inside = torch.empty(n, device=dev, dtype=torch.uint8)
        z = torch.empty(n, S, device=dev)
        pts = torch.empty(n, S, 3, device=dev)
        if depth_max is not None:                         # per-frame max sampled depth supplied (multi-GPU: global max)
            ws = depth_max.detach().float().contiguous().view(torch.int32)
        else:
            ws = torch.empty(K, device=dev, dtype=torch.int32)
        camv = (C.c_double * 4)(*[float(v) for v in cam])
        b6 = _bound6(bound)
        check(lib.dns_raygen_sample(ptr(pix_idx), ptr(color), ptr(depth), ptr(label), ptr(quat), ptr(trans), camv, b6,
                                    H, W, H0, H1, W0, W1, K, npf, ptr(t_uniform), ptr(t_surf), ptr(t_zero), nu, ns, jstride,
                                    ptr(ws), 0 if depth_max is None else 1, ptr(rays_o), ptr(rays_d), ptr(gt_color),
                                    ptr(gt_depth), ptr(gt_label),
                                    ptr(inside), ptr(z), ptr(pts), stream_ptr()), "dns_raygen_sample")
        ctx.save_for_backward(pix_idx, quat, z)
        ctx.misc = (camv, window, K, npf, S)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(gt_color, gt_depth, gt_label, inside, z)
        return rays_o, rays_d, pts, gt_color, gt_depth, gt_label, inside, z

    @staticmethod
    def backward(ctx, d_ro, d_rd, d_pts, *_):
        pix_idx, quat, z = ctx.saved_tensors
        camv, (H0, H1, W0, W1), K, npf, S = ctx.misc
        dev = quat.device
        d_quat = torch.zeros(K, 4, device=dev)
        d_trans = torch.zeros(K, 3, device=dev)
        ws = torch.empty(max(int(lib.dns_raygen_bwd_ws_floats(K, npf)), 1), device=dev)
        c = lambda t: None if t is None else t.contiguous()
        check(lib.dns_raygen_bwd(ptr(pix_idx), ptr(quat), camv, H0, H1, W0, W1, K, npf, S, ptr(z), ptr(c(d_pts)),
                                 ptr(c(d_ro)), ptr(c(d_rd)), ptr(ws), ptr(d_quat), ptr(d_trans), stream_ptr()),
              "dns_raygen_bwd")
        return (d_quat, d_trans) + (None,) * 12


def raygen_sample(quat, trans, pix_idx, color, depth, label, cam, bound, window, n_per_frame, t_uniform, t_surf, t_zero,
                  depth_max=None):
    """K stacked frames -> (rays_o, rays_d, pts, gt_color, gt_depth, gt_label, inside, z).  quat [K,4], trans [K,3],
    pix_idx [K*n_per_frame] int64 window-flat indices, color [K,H,W,3], depth/label [K,H,W] fp32,
    cam=(fx,fy,cx,cy), bound [3,2] fp64, window=(H0,H1,W0,W1)."""
    return _RaygenFn.apply(quat, trans, pix_idx, color, depth, label, tuple(cam), bound, tuple(window), n_per_frame,
                           t_uniform, t_surf, t_zero, depth_max)


class _RaysFromPixelsFn(torch.autograd.Function):
    """rays_o, rays_d, sample rows for given pixel indices and a rotation MATRIX (get_rays_from_uv, utils/common.py:248-264).
    The backward (dL/dR = sum_n dL/dd_n (x) dir_n, dL/dT = sum_n dL/do_n: SURVEY A1) is two [n,3]-sized reductions; they are
    plain torch on purpose -- this node only serves callers of the reference's free functions (Mesher, eval_2d: no
    gradient); the optimise steps differentiate the pose through dns_raygen_bwd."""

    @staticmethod
    def forward(ctx, R, T, pix_idx, image, cam, hw, window):
        require_cuda(R, T, pix_idx, image)
        H, W = hw
        H0, H1, W0, W1 = window
        dev = R.device
        n = (H1 - H0) * (W1 - W0) if pix_idx is None else pix_idx.numel()
        Rc, Tc = R.detach().contiguous().float(), T.detach().contiguous().float()
        Cn = 0 if image is None else image.shape[-1]
        rays_o = torch.empty(n, 3, device=dev)
        rays_d = torch.empty(n, 3, device=dev)
        sample = torch.empty(n, Cn, device=dev) if Cn else None
        ij = torch.empty(n, 2, device=dev)
        camv = (C.c_double * 4)(*[float(v) for v in cam])
        check(lib.dns_rays_from_pixels(ptr(pix_idx), ptr(image), Cn, ptr(Rc), ptr(Tc), camv, H, W, H0, H1, W0, W1, n,
                                       ptr(rays_o), ptr(rays_d), ptr(sample), ptr(ij), stream_ptr()), "dns_rays_from_pixels")
        ctx.save_for_backward(ij)
        ctx.cam = tuple(float(v) for v in cam)
        ctx.mark_non_differentiable(ij)
        if sample is None:
            sample = rays_o.new_zeros(n, 0)
        ctx.mark_non_differentiable(sample)
        ctx.set_materialize_grads(False)
        return rays_o, rays_d, sample, ij

    @staticmethod
    def backward(ctx, d_ro, d_rd, _ds, _dij):
        ij, = ctx.saved_tensors
        fx, fy, cx, cy = ctx.cam
        d_R = d_T = None
        if d_rd is not None and ctx.needs_input_grad[0]:
            dirs = torch.stack(((ij[:, 0] - cx) / fx, -(ij[:, 1] - cy) / fy, -torch.ones_like(ij[:, 0])), -1)
            d_R = d_rd.t() @ dirs
        if d_ro is not None and ctx.needs_input_grad[1]:
            d_T = d_ro.sum(0)
        return d_R, d_T, None, None, None, None, None


def rays_from_pixels(R, T, pix_idx, image, cam, hw, window):
    """R [3,3], T [3] (device), pix_idx [n] int64 window-flat (None = every pixel of the window in row-major order),
    image [H,W,C] or None, cam=(fx,fy,cx,cy), hw=(H,W), window=(H0,H1,W0,W1) -> rays_o, rays_d [n,3], sample [n,C], ij [n,2]."""
    if image is not None:
        image = image.contiguous().float()
    if pix_idx is not None:
        pix_idx = pix_idx.contiguous()
    return _RaysFromPixelsFn.apply(R.contiguous(), T.contiguous(), pix_idx, image, tuple(cam), tuple(hw), tuple(window))


def sample_along_rays(gt_depth, far_bb, t_uniform, t_surf, t_zero):
    """Stand-alone depth-guided sampling (utils/common.py:561-599) with explicit jitter: gt_depth [n] fp32,
    far_bb [n] or [n,1] fp64 (+0.01 already applied) -> z [n, S] ascending fp32."""
    require_cuda(gt_depth, far_bb, t_uniform, t_surf, t_zero)
    gt_depth = gt_depth.reshape(-1).contiguous().float()
    far_bb = far_bb.reshape(-1).contiguous().double()
    n = gt_depth.numel()
    nu = 0 if t_uniform is None else t_uniform.numel()
    ns = t_surf.numel()
    z = torch.empty(n, nu + ns, device=gt_depth.device)
    ws = torch.empty(1, device=gt_depth.device, dtype=torch.int32)
    check(lib.dns_sample_along_rays(ptr(gt_depth), ptr(far_bb), n, ptr(t_uniform), ptr(t_surf), ptr(t_zero), nu, ns,
                                    ptr(ws), ptr(z), stream_ptr()), "dns_sample_along_rays")
    return z


# ----------------------------------------------------------------------------- fused losses
class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_color, pred_depth, pred_var, pred_logits, fine, coarse, gt_color, gt_depth, gt_label, valid, z,
                lambdas, tracker, reduce_sums):
        require_cuda(pred_color, pred_depth, pred_var, pred_logits, fine, coarse, gt_color, gt_depth, gt_label, valid, z)
        c = lambda t: None if t is None else t.contiguous()
        pred_color, pred_depth, pred_var, pred_logits = c(pred_color), c(pred_depth), c(pred_var), c(pred_logits)
        fine, coarse, gt_color, gt_depth, gt_label, z = c(fine), c(coarse), c(gt_color), c(gt_depth), c(gt_label), c(z)
        N = pred_depth.shape[0]
        Cn = 0 if pred_logits is None else pred_logits.shape[-1]
        S = 1 if z is None else z.shape[1]
        L = 1 if fine is None else fine.shape[-1]
        dev = pred_depth.device
        lam = (C.c_float * 8)(*[float(v) for v in lambdas])
        sums_ws = torch.empty(LOSS_SUMS_FLOATS, device=dev)     # [0:16] results, the rest reduction workspace
        sums = sums_ws[:16]
        out = torch.empty(16, device=dev)
        check(lib.dns_loss_sums(lam, N, S, Cn, L, int(tracker), ptr(pred_color), ptr(pred_depth), ptr(pred_var),
                                ptr(pred_logits), ptr(gt_color), ptr(gt_depth), ptr(gt_label), ptr(valid), ptr(fine),
                                ptr(coarse), ptr(z), ptr(sums_ws), stream_ptr()), "dns_loss_sums")
        if reduce_sums is not None:
            reduce_sums(sums)                      # multi-GPU: global numerators / counts (dns_slam_amd.dist)
        check(lib.dns_loss_finalize(lam, N, S, Cn, L, int(tracker), ptr(sums), ptr(out), stream_ptr()), "dns_loss_finalize")
        ctx.save_for_backward(pred_color, pred_depth, pred_var, pred_logits, fine, coarse, gt_color, gt_depth, gt_label,
                              valid, z, out)
        ctx.misc = (lam, N, S, Cn, L, int(tracker))
        total = out[6]
        terms = out[:6]
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        (pred_color, pred_depth, pred_var, pred_logits, fine, coarse, gt_color, gt_depth, gt_label, valid, z,
         out) = ctx.saved_tensors
        lam, N, S, Cn, L, tracker = ctx.misc
        dev = pred_depth.device
        g = g_total.reshape(1).contiguous().float()
        d_color = torch.empty_like(pred_color)
        d_depth = torch.empty_like(pred_depth)
        d_var = torch.empty_like(pred_var) if pred_var is not None else None
        d_logits = torch.empty_like(pred_logits) if Cn else None
        d_fine = torch.empty_like(fine) if fine is not None else None
        d_coarse = torch.empty_like(coarse) if coarse is not None else None
        check(lib.dns_loss_bwd(lam, N, S, Cn, L, tracker, ptr(out), ptr(g), ptr(pred_color), ptr(pred_depth), ptr(pred_var),
                               ptr(pred_logits), ptr(gt_color), ptr(gt_depth), ptr(gt_label), ptr(valid), ptr(fine),
                               ptr(coarse), ptr(z), ptr(d_color), ptr(d_depth), ptr(d_var), ptr(d_logits), ptr(d_fine),
                               ptr(d_coarse), 0, stream_ptr()), "dns_loss_bwd")
        return (d_color, d_depth, d_var, d_logits, d_fine, d_coarse) + (None,) * 8


def mapping_losses(pred_color, pred_depth, pred_logits, fine, coarse, gt_color, gt_depth, gt_label, z_vals, lambdas,
                   valid=None, reduce_sums=None):
    """The six ray-batch loss terms of one mapping iteration, fused (slams/mapping.py:887-907 minus smoothness).
    lambdas = (lambda_p, lambda_d, lambda_l, lambda_lt, lambda_fs, lambda_opacity, truncation, sigma).
    -> (weighted total [scalar, differentiable], terms [6] = p, d, l, lt, fs, opacity)."""
    return _LossFn.apply(pred_color, pred_depth, None, pred_logits, fine, coarse, gt_color, gt_depth, gt_label, valid,
                         z_vals, lambdas, False, reduce_sums)


def tracking_losses(pred_color, pred_depth, pred_var, pred_logits, gt_color, gt_depth, gt_label, mask, lambdas):
    """The three masked tracking losses, fused (slams/tracking.py:85-96, 326-329). mask: bool / uint8 [N]."""
    valid = mask.to(torch.uint8).contiguous()
    lam = tuple(lambdas) + (0.0,) * (8 - len(lambdas))
    lam = (lam[0], lam[1], lam[2], 0.0, 0.0, 0.0, 0.0, 1.0)
    return _LossFn.apply(pred_color, pred_depth, pred_var, pred_logits, None, None, gt_color, gt_depth, gt_label, valid,
                         None, lam, True, None)



# ----------------------------------------------------------------------------- smoothness (TV)
class _TvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lat, n, sample_points, nx, halo):
        require_cuda(lat)
        lat = lat.contiguous().float()
        if lat.shape[0] != nx * n * n:
            raise ValueError(f"tv_smoothness: {lat.shape[0]} lattice rows for a {nx} x {n} x {n} slab")
        out = torch.empty(1, device=lat.device)
        check(lib.dns_tv_fwd(ptr(lat), lat.shape[1], nx, n, int(halo), sample_points, ptr(out), stream_ptr()), "dns_tv_fwd")
        ctx.save_for_backward(lat)
        ctx.misc = (n, sample_points, nx, int(halo))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lat, = ctx.saved_tensors
        n, sp, nx, halo = ctx.misc
        d = torch.empty_like(lat)
        check(lib.dns_tv_bwd(ptr(lat), lat.shape[1], nx, n, halo, sp, ptr(g.reshape(1).contiguous().float()), ptr(d), stream_ptr()),
              "dns_tv_bwd")
        return d, None, None, None, None


def tv_smoothness(latents: torch.Tensor, n: int, sample_points: int, nx: Optional[int] = None, halo: bool = False) -> torch.Tensor:
    """Total variation of latents[:, 0] on an n^3 lattice / sample_points^3 (slams/mapping.py:151-157).
    latents [n^3, L] = the coarse decoder's output on the lattice points (x-major).  ``nx`` / ``halo``: the rows are a slab of
    nx x-planes of a lattice cut along x, the last plane being the next slab's first (include/dns_hip.h): the slabs' values
    sum to the cube's."""
    return _TvFn.apply(latents, n, sample_points, n if nx is None else nx, halo)


# ----------------------------------------------------------------------------- 2-D feature lookup
def feature_gather(pts: torch.Tensor, refer_w2c: torch.Tensor, K, feat_nhwc: torch.Tensor, H: int, W: int):
    """pts [P,3], refer_w2c [R,4,4], K 3x3 (host values), feat_nhwc [R,h,w,C] -> (code [R,P,C], mask [R,P] bool).
    No gradient (frozen stem features, rounded pixel)."""
    require_cuda(pts, refer_w2c, feat_nhwc)
    pts = pts.detach().contiguous().float()
    w2c = refer_w2c.detach().contiguous().float()
    R, h, w, Cc = feat_nhwc.shape
    P = pts.shape[0]
    Kh = (C.c_float * 9)(*[float(v) for v in torch.as_tensor(K).reshape(-1).tolist()])
    code = torch.empty(R, P, Cc, device=pts.device)
    mask = torch.empty(R, P, device=pts.device, dtype=torch.uint8)
    check(lib.dns_feature_gather(ptr(pts), ptr(w2c), Kh, ptr(feat_nhwc), R, P, Cc, h, w, H, W, ptr(code), ptr(mask),
                                 stream_ptr()), "dns_feature_gather")
    return code, mask.bool()


def _byte_workspace(n_bytes, dev, refusal: str) -> torch.Tensor:
    """The uint8 workspace of n_bytes (a dns_*_ws_bytes value) on dev; 0 bytes is that function's refusal: ValueError(refusal)."""
    if int(n_bytes) == 0:
        raise ValueError(refusal)
    return torch.empty(int(n_bytes), dtype=torch.uint8, device=dev)


# ----------------------------------------------------------------------------- mesh extraction (csrc/mesh.hip)
def marching_cubes(volume: torch.Tensor, level: float, origin, spacing):
    """volume [nx, ny, nz] fp32 (C order; volume[i,j,k] at origin + (i,j,k) * spacing), level, origin / spacing 3 floats each
    -> (verts [V,3] fp32, faces [F,3] int32): skimage.measure.marching_cubes' shared-vertex mesh with gradient_direction=
    'descent' (meshing.py:668-688), vertex and face order as include/dns_hip.h states.  One host read (the two totals)."""
    vol = volume.detach().contiguous().float()
    require_cuda(vol)
    if vol.dim() != 3:
        raise ValueError(f"marching_cubes: volume must be [nx, ny, nz], got {tuple(vol.shape)}")
    nx, ny, nz = (int(s) for s in vol.shape)
    o = (C.c_double * 3)(*[float(v) for v in origin])
    s = (C.c_double * 3)(*[float(v) for v in spacing])
    if not all(np.isfinite(list(s))) or not all(np.isfinite(list(o))):
        raise ValueError("marching_cubes: origin and spacing must be finite")
    dev = vol.device
    ws_b = int(_rawlib.dns_mc_ws_bytes(nx, ny, nz)) if vol.numel() else 0
    if vol.numel() and ws_b == 0:
        raise ValueError(f"marching_cubes: grid {nx} x {ny} x {nz} is too large (>= 2^31 edges)")
    ws = torch.empty(max(ws_b, 1), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib.dns_mc_count(ptr(vol), nx, ny, nz, float(level), ptr(ws), ptr(totals), stream_ptr()), "dns_mc_count")
    V, F = (int(v) for v in totals.cpu().tolist())
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V or F:
        check(lib.dns_mc_emit(ptr(vol), nx, ny, nz, float(level), o, s, ptr(ws), ptr(verts), V, ptr(faces), F, stream_ptr()),
              "dns_mc_emit")
    return verts, faces


def _pose_args(who, points, w2c):
    """points [P,3] and w2c [K,4,4] as the pose kernels take them -> (pts, w, K): detached contiguous fp32 CUDA tensors."""
    pts = points.detach().contiguous().float()
    w = w2c.detach().contiguous().float()            # torch.inverse of a batch returns column-major matrices
    require_cuda(pts, w)
    if pts.dim() != 2 or pts.shape[1] != 3 or w.dim() != 3 or w.shape[1:] != (4, 4):
        raise ValueError(f"{who}: points [P,3] and w2c [K,4,4], got {tuple(pts.shape)} and {tuple(w.shape)}")
    return pts, w, int(w.shape[0])


def _intrinsics(fx, fy, cx, cy):
    return (C.c_float * 4)(float(fx), float(fy), float(cx), float(cy))


def keyframe_project(points: torch.Tensor, w2c: torch.Tensor, labels: torch.Tensor, max_depth: torch.Tensor, cam: dict):
    """points [P,3] world, w2c [K,4,4] (torch.inverse(est_c2w) in fp32), labels [K,H,W] (gt_label), max_depth [K] (max of each
    keyframe's gt_depth), cam {'fx','fy','cx','cy'} -> (label [P] fp32: get_2d_feature's label_pts, meshing.py:313-373;
    seen [P] bool: point_masks' seen mask without the depth test, meshing.py:203-274)."""
    pts, w, K = _pose_args("keyframe_project", points, w2c)
    lab = labels.detach().contiguous().float()
    md = max_depth.detach().contiguous().float().reshape(-1)
    require_cuda(lab, md)
    if lab.dim() != 3 or lab.shape[0] != K or md.numel() != K:
        raise ValueError("keyframe_project: w2c [K,4,4], labels [K,H,W], max_depth [K]")
    H, W = int(lab.shape[1]), int(lab.shape[2])
    intr = _intrinsics(cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    P = pts.shape[0]
    label = torch.empty(P, device=pts.device)
    seen = torch.empty(P, dtype=torch.uint8, device=pts.device)
    check(lib.dns_keyframe_project(ptr(pts), P, ptr(w), K, ptr(lab), ptr(md), H, W, intr, ptr(label), ptr(seen), stream_ptr()),
          "dns_keyframe_project")
    return label, seen.bool()


# ----------------------------------------------------------------------------- point masks (csrc/mesh_masks.hip)
MASK_UNSEEN, MASK_SEEN, MASK_FORECAST = 0, 1, 2


@torch.no_grad()
def point_masks(points: torch.Tensor, w2c: torch.Tensor, cam: dict, H: int, W: int, *, max_depth: Optional[torch.Tensor] = None,
                depths: Optional[torch.Tensor] = None, chunk: Optional[int] = None):
    """point_masks of the reference (meshing.py:124-291): points [P,3] world, w2c [K,4,4] fp32 world->camera, cam
    {'fx','fy','cx','cy'}, image size H x W -> cls [P] uint8, 0 = unseen, 1 = seen, 2 = forecast (a point is forecast only when no
    pose sees it).  Three modes (include/dns_hip.h):
      neither ``max_depth`` nor ``depths``   the frustum tests alone (get_mask_use_all_frames, :164-201);
      ``max_depth`` [K]                      both masks need -cam_z < 1.2 max_depth[k] (:257-271); seen is keyframe_project's;
      ``depths`` [K,H,W] and ``chunk``       the depth test (:229-255) against the bilinear sample of the keyframe's depth; the
                                             forecast limit is the maximum sample over the point's ``chunk``-point chunk, as the
                                             reference's per-points_batch_size torch.max -- the result depends on ``chunk``.
    P = 0 or K = 0: all unseen, nothing is launched."""
    who = "point_masks"
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points [P,3]")
    if points.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: {points.shape[0]} points (must be < 2^31)")
    if max_depth is not None and depths is not None:
        raise ValueError(f"{who}: max_depth (depth limit) and depths (depth test) exclude each other")
    if depths is not None and chunk is None:
        raise ValueError(f"{who}: the depth test needs chunk (the reference's points_batch_size)")
    if depths is None and chunk is not None:
        raise ValueError(f"{who}: chunk is the depth test's; pass depths with it")
    if chunk is not None and not 0 < int(chunk) < 1 << 32:
        raise ValueError(f"{who}: chunk must be in 1 .. 2^32 - 1, got {chunk}")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: image of {H} x {W}")
    pts, w, K = _pose_args(who, points, w2c)
    md = dep = None
    if max_depth is not None:
        md = max_depth.detach().contiguous().float().reshape(-1)
        require_cuda(md)
        if md.numel() != K:
            raise ValueError(f"{who}: w2c [K,4,4] and max_depth [K] with one K, got {tuple(w.shape)} and {tuple(max_depth.shape)}")
    if depths is not None:
        dep = depths.detach().contiguous().float()
        require_cuda(dep)
        if tuple(dep.shape) != (K, H, W):
            raise ValueError(f"{who}: depths must be [K,H,W] = {(K, H, W)}, got {tuple(dep.shape)}")
    P, dev = int(pts.shape[0]), pts.device
    if P == 0 or K == 0:
        return torch.zeros(P, dtype=torch.uint8, device=dev)
    cls = torch.empty(P, dtype=torch.uint8, device=dev)
    ws, c = None, 0
    if dep is not None:
        c = min(int(chunk), P)                               # a chunk beyond P is the one chunk of P points
        ws = torch.empty(int(_rawlib.dns_point_masks_ws_bytes(P, K, c)), dtype=torch.uint8, device=dev)
    check(lib.dns_point_masks(ptr(pts), P, ptr(w), K, ptr(md), ptr(dep), c, H, W, _intrinsics(cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                              ptr(ws), ptr(cls), stream_ptr()), "dns_point_masks")
    return cls


# ----------------------------------------------------------------------------- keyframe codes (csrc/mesh_feature.hip)
KF_WORKSPACE_BYTES = 1 << 30                 # default budget of keyframe_codes' row, latent, record and relative-point buffers


def _kf_args(who, points, w2c, depths, cam, chunked=False):
    for t in (points, w2c, depths):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{who}: dns_slam_amd ops run on the GPU only (got a non-CUDA tensor); there is no CPU fallback")
    if len({t.device for t in (points, w2c, depths)}) != 1:
        raise ValueError(f"{who}: the arguments live on different devices")
    pts, w, K = _pose_args(who, points, w2c)
    if depths.dim() != 3 or depths.shape[0] != K:
        raise ValueError(f"{who}: w2c [K,4,4] and depths [K,H,W] with one K, got {tuple(w2c.shape)} and {tuple(depths.shape)}")
    if not all(t.is_floating_point() for t in (points, w2c, depths)):
        raise ValueError(f"{who}: points, w2c and depths must be floating point")
    dep = depths.detach().contiguous().float()
    H, W = int(dep.shape[1]), int(dep.shape[2])
    if H < 1 or W < 1:
        raise ValueError(f"{who}: depth images of {H} x {W}")
    if not chunked and pts.shape[0] * max(K, 1) >= 1 << 31:           # (keyframe_codes launches per chunk: chunk * K is bounded there)
        raise ValueError(f"{who}: {pts.shape[0]} points x {K} keyframes (must be < 2^31 pairs)")
    return pts, w, dep, K, H, W, _intrinsics(cam["fx"], cam["fy"], cam["cx"], cam["cy"])


def _kf_pair_list(pts, w, dep, K, H, W, intr, records=None):
    """count [P] int32, offset [P] int64, n (the ONE host read) and the records [n, 4] int32 (in ``records`` when given)."""
    P, dev = pts.shape[0], pts.device
    count = torch.empty(P, dtype=torch.int32, device=dev)
    check(lib.dns_kf_pair_count(ptr(pts), P, ptr(w), K, ptr(dep), H, W, intr, ptr(count), stream_ptr()), "dns_kf_pair_count")
    incl = torch.cumsum(count, 0, dtype=torch.int64)
    offset = incl - count
    n = int(incl[-1].item())
    if records is None:
        records = torch.empty(max(n, 1), 4, dtype=torch.int32, device=dev)
    if n > records.shape[0]:
        raise RuntimeError(f"keyframe pairs: {n} pairs for a list of {records.shape[0]}")
    if n:
        check(lib.dns_kf_pair_emit(ptr(pts), P, ptr(w), K, ptr(dep), H, W, intr, ptr(offset), ptr(records), n, stream_ptr()),
              "dns_kf_pair_emit")
    return count, offset, n, records


@torch.no_grad()
def keyframe_pairs(points: torch.Tensor, w2c: torch.Tensor, depths: torch.Tensor, cam: dict):
    """points [P,3] world, w2c [K,4,4] (torch.inverse(est_c2w) in fp32), depths [K,H,W] (gt_depth), cam {'fx','fy','cx','cy'} ->
    (point [n] int64, keyframe [n] int64, iu [n] int64, iv [n] int64, count [P] int32): the (point, keyframe) pairs that
    contribute to get_2d_feature's code (meshing.py:337-356: seen, and inside the truncation band of the keyframe's depth at
    the rounded pixel (iu, iv)), point-major with the keyframes ascending within a point; count = pairs per point.  One host
    read (n)."""
    pts, w, dep, K, H, W, intr = _kf_args("keyframe_pairs", points, w2c, depths, cam)
    P, dev = pts.shape[0], pts.device
    if P == 0 or K == 0:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return e, e.clone(), e.clone(), e.clone(), torch.zeros(P, dtype=torch.int32, device=dev)
    count, _, n, rec = _kf_pair_list(pts, w, dep, K, H, W, intr)
    rec = rec[:n].long()
    return rec[:, 0].contiguous(), rec[:, 1].contiguous(), rec[:, 2].contiguous(), rec[:, 3].contiguous(), count


@torch.no_grad()
def keyframe_codes(points: torch.Tensor, w2c: torch.Tensor, origins: torch.Tensor, depths: torch.Tensor, stem_nhwc: torch.Tensor,
                   cam: dict, merge, max_pairs: Optional[int] = None):
    """get_2d_feature's pixel_pts (meshing.py:311-377): points [P,3] world, w2c [K,4,4], origins [K,3] (est_c2w[:3,3]), depths
    [K,H,W], stem_nhwc [K,h,w,C] fp32 (the stem maps, channels last, half resolution), ``merge`` the ``Decoder.merge`` module
    -> (code [P, hidden] fp32: the mean over the contributing keyframes of Merge(p - o_k, stem value at the rounded pixel), zeros
    where none contributes; count [P] int32).  Forward only.

    The points are taken in chunks of ``max_pairs // K`` (``max_pairs`` defaults to KF_WORKSPACE_BYTES over the bytes of a
    pair: 604 for the 112 -> 32 network), so the workspace is bounded whatever the scene and only ``chunk * K`` has to stay
    below 2^31; a point's pairs are never split and are added in keyframe order, so the result is
    the same bits for every ``max_pairs``.  One host read (the pair total) per chunk."""
    pts, w, dep, K, H, W, intr = _kf_args("keyframe_codes", points, w2c, depths, cam, chunked=True)
    dev = pts.device
    net = merge.decoder
    n_pe, hidden = int(merge.pe_dim), int(net.n_output_dims)
    if not (isinstance(origins, torch.Tensor) and origins.is_cuda and origins.device == dev and origins.is_floating_point()
            and origins.shape == (K, 3)):
        raise ValueError(f"keyframe_codes: origins must be a floating-point [K,3] = [{K},3] tensor on {dev}")
    if not (isinstance(stem_nhwc, torch.Tensor) and stem_nhwc.is_cuda and stem_nhwc.device == dev
            and stem_nhwc.dtype == torch.float32 and stem_nhwc.dim() == 4 and stem_nhwc.shape[0] == K):
        raise ValueError(f"keyframe_codes: stem_nhwc must be a float32 [K,h,w,C] tensor on {dev} with K = {K}")
    h, w_, Cc = (int(s) for s in stem_nhwc.shape[1:])
    if Cc % 4 != 0 or Cc == 0:
        raise ValueError(f"keyframe_codes: {Cc} stem channels (must be a multiple of 4)")
    if n_pe + Cc != int(net.n_input_dims) or n_pe % 4 != 0 or hidden % 4 != 0:
        raise ValueError(f"keyframe_codes: {n_pe} encoding + {Cc} stem columns for a Merge network of {net.n_input_dims} inputs")
    if net.params.device != dev:
        raise ValueError(f"keyframe_codes: the Merge network lives on {net.params.device}, the points on {dev}")
    if K and (h < 1 or w_ < 1):
        raise ValueError(f"keyframe_codes: stem maps of {h} x {w_}")
    org = origins.detach().contiguous().float()
    feat = stem_nhwc.detach().contiguous()
    P = pts.shape[0]
    code = torch.zeros(P, hidden, device=dev)
    count = torch.zeros(P, dtype=torch.int32, device=dev)
    if P == 0 or K == 0:
        return code, count
    ld = n_pe + Cc
    if max_pairs is None:
        max_pairs = KF_WORKSPACE_BYTES // (4 * (ld + hidden + 4 + 3))
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs < 1 << 31:
        raise ValueError(f"keyframe_codes: max_pairs {max_pairs}")
    if K >= 1 << 31:
        raise ValueError(f"keyframe_codes: {K} keyframes")
    chunk = min(max(max_pairs // K, 1), P)
    cap = chunk * K
    rows = torch.empty(cap, ld, device=dev)
    rel = torch.empty(cap, 3, device=dev)
    records = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    b6 = _bound6(merge.bound)
    for s0 in range(0, P, chunk):
        s1 = min(s0 + chunk, P)
        p = pts[s0:s1]
        cnt, offset, n, _ = _kf_pair_list(p, w, dep, K, H, W, intr, records)
        count[s0:s1] = cnt
        if n == 0:
            continue
        check(lib.dns_kf_pair_rows(ptr(records), n, ptr(p), s1 - s0, ptr(org), K, ptr(feat), Cc, h, w_, H, W, ptr(rel),
                                   C.c_void_p(rows.data_ptr() + 4 * n_pe), ld, stream_ptr()), "dns_kf_pair_rows")
        # Merge (models/decoder.py:67-77) on one view per row: OneBlob of the bound-normalised relative point into columns
        # 0..n_pe of the rows the stem values already sit in, then the network; no concatenation
        check(lib.dns_encode_fwd(ptr(rel), b6, n, merge.pe_fn.n_bins, None, None, None, ptr(rows), ld, None, 0, None, stream_ptr()),
              "dns_encode_fwd")
        lat = net(rows[:n])
        check(lib.dns_kf_code_mean(ptr(lat), lat.stride(0), n, ptr(offset), ptr(cnt), s1 - s0, hidden,
                                   C.c_void_p(code.data_ptr() + 4 * hidden * s0), stream_ptr()), "dns_kf_code_mean")
    return code, count


# ----------------------------------------------------------------------------- frame codes (csrc/frame_codes.hip)
FRAME_CODES_METHODS = ("fused", "launches")


FRAME_CODES_DEFAULT = "fused"              # what ``method=None`` means where the fused kernel takes the shape


def frame_codes_fused_ok(merge, Cs: int) -> bool:
    """The shapes ``frame_codes(method="fused")`` takes (the ones ``launch.Stem2D`` accepts, on the fp32-grade kernels):
    n_in = 3 n_bins + Cs with both parts multiples of 4 (and n_in one of 8, at most 128), hid a multiple of 4 up to 64, a Merge
    network of 32 x 1 or 64 x 2 that is not ``fp16``."""
    net = merge.decoder
    n_pe, hid = 3 * int(merge.pe_fn.n_bins), int(net.n_output_dims)
    n_in = n_pe + int(Cs)
    return (n_in == int(net.n_input_dims) and n_pe % 4 == 0 and n_pe > 0 and Cs % 4 == 0 and Cs > 0 and n_in % 8 == 0
            and n_in <= 128 and hid % 4 == 0 and 0 < hid <= 64 and not getattr(net, "fp16", False)
            and (int(net.n_neurons), int(net.n_hidden_layers)) in ((32, 1), (64, 2)))


@torch.no_grad()
def frame_codes(pts: torch.Tensor, refer_w2c: torch.Tensor, stem_nhwc: torch.Tensor, cam, H: int, W: int, merge, *, keep=None,
                method: Optional[str] = None, out: Optional[torch.Tensor] = None, tile: int = 0,
                origins: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 2-D code of the points of a rendered frame: pts [P,3] world, refer_w2c [R,4,4], stem_nhwc [R,h,w,Cs] fp32 (the stem
    maps, channels last, half resolution), cam {'fx','fy','cx','cy'} (or the four values), ``merge`` the ``Decoder.merge`` module
    -> code [P, hid] fp32: exactly ``common.feature_matching(H, W, K, pts, refer_w2c, maps, merge)`` -- per view the code at the
    rounded projected pixel (zeros where the view does not see the point), Merge on OneBlob(p - o_r) + code, the mean over the views
    (reference utils/common.py:645-679, models/decoder.py:67-77, as frame_vis and novel_view_render call them per chunk:
    slams/mapping.py:666-689, eval_2d.py:260-283).  Forward only.

    ``keep`` [P] uint8 / bool: a point with 0 gets a zero row and none of its taps are read.
    ``method="fused"``: one kernel (csrc/frame_codes.hip); the Merge rows live in a workgroup-private workspace slice.  ``"launches"``: the composition of
    the existing launches, ``common.feature_matching`` times ``keep`` -- the yardstick and the fallback.  A shape the fused kernel
    does not take (``frame_codes_fused_ok``) raises.  ``method=None`` (the default) is ``FRAME_CODES_DEFAULT`` where the fused kernel
    takes the shape and ``"launches"`` where it does not, without comment.
    ``out``: a float32 [P, hid] tensor to write into (rows of a larger tensor are fine).  ``tile``: points a workgroup of the fused
    kernel takes at a time, 32, 64 or 128 (0: chosen by the library from the point count; the bits do not depend on it).
    ``origins`` [R,3]: ``torch.inverse(refer_w2c)[:, :3, 3]`` where the caller has it already (``render_frame`` computes it once
    per frame, not once per chunk: the inverse reads its status back to the host); both methods take it."""
    pts, w2c, R = _pose_args("frame_codes", pts, refer_w2c)
    dev = pts.device
    if method is not None and method not in FRAME_CODES_METHODS:
        raise ValueError(f"frame_codes: method {method!r} (one of {FRAME_CODES_METHODS})")
    if not (isinstance(stem_nhwc, torch.Tensor) and stem_nhwc.is_cuda and stem_nhwc.device == dev and stem_nhwc.dtype == torch.float32
            and stem_nhwc.dim() == 4 and stem_nhwc.shape[0] == R):
        raise ValueError(f"frame_codes: stem_nhwc must be a float32 [R,h,w,Cs] tensor on {dev} with R = {R}")
    if R < 1:
        raise ValueError("frame_codes: no reference view")
    h, w_, Cs = (int(s) for s in stem_nhwc.shape[1:])
    if h < 1 or w_ < 1 or Cs < 1 or H < 1 or W < 1:
        raise ValueError(f"frame_codes: stem maps of {h} x {w_} x {Cs} for images of {H} x {W}")
    net = merge.decoder
    hid, n_bins = int(net.n_output_dims), int(merge.pe_fn.n_bins)
    if net.params.device != dev:
        raise ValueError(f"frame_codes: the Merge network lives on {net.params.device}, the points on {dev}")
    if 3 * n_bins + Cs != int(net.n_input_dims):
        raise ValueError(f"frame_codes: {3 * n_bins} encoding + {Cs} stem columns for a Merge network of {net.n_input_dims} inputs")
    P = pts.shape[0]
    if keep is not None:
        if not (isinstance(keep, torch.Tensor) and keep.is_cuda and keep.device == dev and keep.dtype in (torch.uint8, torch.bool)
                and keep.shape == (P,)):
            raise ValueError(f"frame_codes: keep must be a uint8 or bool [P] = [{P}] tensor on {dev}")
        keep = keep.detach().contiguous().view(torch.uint8)
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.float32
                and out.shape == (P, hid)):
            raise ValueError(f"frame_codes: out must be a float32 [P, hid] = [{P}, {hid}] tensor on {dev}")
    fused_ok = frame_codes_fused_ok(merge, Cs)
    if method is None:
        method = FRAME_CODES_DEFAULT if fused_ok else "launches"
    if method == "fused" and not fused_ok:
        raise ValueError(f"frame_codes: method='fused' takes 3 n_bins and Cs multiples of 4 (their sum one of 8, at most 128), hid a "
                         f"multiple of 4 up to 64 and an fp32-grade Merge network of 32 x 1 or 64 x 2; got n_bins {n_bins}, Cs {Cs}, "
                         f"hid {hid}, {net.n_neurons} x {net.n_hidden_layers}{', fp16' if getattr(net, 'fp16', False) else ''}")
    fx, fy, cx, cy = (cam["fx"], cam["fy"], cam["cx"], cam["cy"]) if isinstance(cam, dict) else cam
    feat = stem_nhwc.detach().contiguous()
    if origins is not None:
        if not (isinstance(origins, torch.Tensor) and origins.is_cuda and origins.device == dev and origins.shape == (R, 3)
                and origins.is_floating_point()):
            raise ValueError(f"frame_codes: origins must be a floating-point [R,3] = [{R},3] tensor on {dev}")
        origins = origins.detach().float().contiguous()
    if method == "launches":
        K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        if P == 0:
            code = torch.zeros(0, hid, device=dev)
        elif origins is None:
            from .common import feature_matching
            code = feature_matching(H, W, K, pts, w2c, feat.permute(0, 3, 1, 2), merge)
        else:
            # feature_matching (common.py) with the origins handed over instead of inverted
            gathered, _ = feature_gather(pts, w2c, K, feat, H, W)
            code = merge(pts[None, :, :] - origins[:, None, :], origins, gathered)
        if keep is not None:
            code = code * keep[:, None].to(code.dtype)
        if out is None:
            return code
        out.copy_(code)
        return out
    direct = out is not None and out.stride(1) == 1 and out.stride(0) % 4 == 0 and out.stride(0) >= hid and out.data_ptr() % 16 == 0
    res = out if direct else torch.empty(P, hid, device=dev)
    if P:
        origin = torch.inverse(w2c)[:, :3, 3].contiguous() if origins is None else origins      # refer_o, as feature_matching takes it
        params = net.params.detach()
        if params.data_ptr() % 16 != 0 or not params.is_contiguous() or params.dtype != torch.float32:
            params = params.float().contiguous().clone()
        nn_, nl = int(net.n_neurons), int(net.n_hidden_layers)
        n_ws = int(lib.dns_frame_codes_ws_floats(P, R, n_bins, Cs, hid, nn_, nl, int(tile)))
        if n_ws == 0:
            raise ValueError(f"frame_codes: {P} points x {R} views in tiles of {tile} refused (at most 64 views, fewer than 2^31 points, "
                             f"tiles of 0 = automatic, 32, 64 or 128)")
        ws = torch.empty(n_ws, device=dev)
        K9 = (C.c_float * 9)(float(fx), 0.0, float(cx), 0.0, float(fy), float(cy), 0.0, 0.0, 1.0)
        check(lib.dns_frame_codes(ptr(pts), P, ptr(w2c), ptr(origin), R, K9, ptr(feat), Cs, h, w_, H, W, ptr(keep),
                                  _bound6(merge.bound), n_bins, ptr(params), nn_, nl, hid, ptr(ws), n_ws, ptr(res), res.stride(0),
                                  int(tile), stream_ptr()), "dns_frame_codes")
    if out is not None and not direct:
        out.copy_(res)
        return out
    return res


# ----------------------------------------------------------------------------- mesh components (csrc/mesh_cc.hip)
def mesh_components(verts: torch.Tensor, faces: torch.Tensor):
    """verts [V,3] fp32, faces [F,3] int32 (any triangle list with shared vertex indices) -> (comp [F] int32: the smallest
    face index of the face's component, comp_area [F] float64: the area of the face's component, n_comp int).  Components as
    mesh.split(only_watertight=False) forms them (meshing.py:722): faces joined through the edges exactly two faces hold
    (include/dns_hip.h).  A vertex index outside [0, V) raises ValueError.  One host read (the count and the index flag)."""
    v = verts.detach().contiguous().float()
    f = faces.detach().contiguous()
    require_cuda(v, f)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"mesh_components: verts [V,3] and faces [F,3], got {tuple(v.shape)} and {tuple(f.shape)}")
    if f.dtype != torch.int32:
        raise ValueError(f"mesh_components: faces must be int32, got {f.dtype}")
    V, F = int(v.shape[0]), int(f.shape[0])
    dev = f.device
    comp = torch.empty(F, dtype=torch.int32, device=dev)
    comp_area = torch.empty(F, dtype=torch.float64, device=dev)
    if F == 0:
        return comp, comp_area, 0
    ws = _byte_workspace(_rawlib.dns_mesh_cc_ws_bytes(F), dev, f"mesh_components: {F} faces are too many (>= 2^29)")
    status = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib.dns_mesh_components(ptr(v), V, ptr(f), F, ptr(ws), ptr(comp), ptr(comp_area), ptr(status), stream_ptr()),
          "dns_mesh_components")
    n_comp, bad = (int(x) for x in status.cpu().tolist())
    if bad:
        raise ValueError(f"mesh_components: a face holds a vertex index outside [0, {V})" if bad & 1 else
                         f"mesh_components: edge table overflow (status {bad:#x})")
    return comp, comp_area, n_comp


# ----------------------------------------------------------------------------- mesh holes (csrc/mesh_holes.hip)
HOLES_INFO_KEYS = ("faces_added", "loops_filled", "boundary_edges", "nonmanifold_edges", "vertices_skipped", "degenerate",
                   "bad_index")
HOLES_MAX_EDGES = 4                        # trimesh.repair.fill_holes closes loops of three and four edges


def mesh_fill_holes(faces: torch.Tensor, n_verts: int, max_edges: int = HOLES_MAX_EDGES):
    """faces [F,3] int32 over ``n_verts`` vertices -> (faces_out [F + A, 3] int32: the input faces, unchanged, then the A faces
    that close the boundary loops of 3 .. ``max_edges`` edges, info: a dict of ints with ``HOLES_INFO_KEYS`` plus ``watertight``,
    true iff the INPUT has no boundary and no non-manifold edge).  mesh.fill_holes() of meshing.py:770 under the definition of
    include/dns_hip.h: every added face starts with its loop's smallest vertex, loops in ascending order of it, a loop's faces in
    fan order; loops through a vertex with more than one boundary edge in or out are left open and their vertices counted in
    ``vertices_skipped``.  ``max_edges`` in 3 .. 32.  A vertex index outside [0, n_verts) raises ValueError.  One host read (the
    whole of info, the total included)."""
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"mesh_fill_holes: faces must be a tensor, got {type(faces).__name__}")
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 3 <= int(max_edges) <= 32:
        raise ValueError(f"mesh_fill_holes: max_edges must be an int in 3 .. 32, got {max_edges!r}")
    if isinstance(n_verts, bool) or not isinstance(n_verts, (int, np.integer)) or not 0 <= int(n_verts) < 2 ** 31:
        raise ValueError(f"mesh_fill_holes: n_verts must be an int in [0, 2^31), got {n_verts!r}")
    f = faces.detach().contiguous()
    require_cuda(f)
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"mesh_fill_holes: faces [F,3], got {tuple(f.shape)}")
    if f.dtype != torch.int32:
        raise ValueError(f"mesh_fill_holes: faces must be int32, got {f.dtype}")
    V, F, max_edges = int(n_verts), int(f.shape[0]), int(max_edges)
    if F == 0:
        info = {k: 0 for k in HOLES_INFO_KEYS}
        info["watertight"] = True
        return faces, info
    dev = f.device
    ws = _byte_workspace(_rawlib.dns_mesh_holes_ws_bytes(F, V), dev, f"mesh_fill_holes: {F} faces are too many (>= 2^29)")
    info_d = torch.empty(8, dtype=torch.int32, device=dev)
    check(lib.dns_mesh_holes_count(ptr(f), F, V, max_edges, ptr(ws), ptr(info_d), stream_ptr()), "dns_mesh_holes_count")
    words = [int(x) for x in info_d.cpu().tolist()]
    if words[6]:
        raise ValueError(f"mesh_fill_holes: a face holds a vertex index outside [0, {V})")
    if words[7]:
        raise ValueError("mesh_fill_holes: edge table overflow")
    info = dict(zip(HOLES_INFO_KEYS, words))
    info["watertight"] = info["boundary_edges"] == 0 and info["nonmanifold_edges"] == 0
    A = info["faces_added"]
    if A == 0:
        return f, info
    out = torch.empty(F + A, 3, dtype=torch.int32, device=dev)
    out[:F] = f
    check(lib.dns_mesh_holes_emit(ptr(ws), V, max_edges, ptr(out[F:]), stream_ptr()), "dns_mesh_holes_emit")
    return out, info


# ----------------------------------------------------------------------------- mesh evaluation (csrc/mesh_eval.hip)
NEAREST_MAX_RINGS = 8


def nearest_points_launch(ref: torch.Tensor, query: torch.Tensor, method: str = "grid", max_rings: int = NEAREST_MAX_RINGS):
    """``nearest_points`` without its host read: -> (dist, idx, status [4] int32 on the device); the caller reads status
    (include/dns_hip.h: status[0] != 0 = non-finite coordinate, the outputs invalid).  Needs N > 0."""
    r = ref.detach().contiguous().float()
    q = query.detach().contiguous().float()
    require_cuda(r, q)
    if r.dim() != 2 or r.shape[1] != 3 or q.dim() != 2 or q.shape[1] != 3:
        raise ValueError(f"nearest_points: ref [M,3] and query [N,3], got {tuple(r.shape)} and {tuple(q.shape)}")
    if method not in ("grid", "brute"):
        raise ValueError(f"nearest_points: method must be 'grid' or 'brute', got {method!r}")
    M, N = int(r.shape[0]), int(q.shape[0])
    if N == 0:
        raise ValueError("nearest_points_launch: no queries")
    if M == 0:
        raise ValueError(f"nearest_points: no reference points for {N} queries")
    dev = q.device
    ws = _byte_workspace(_rawlib.dns_nearest_ws_bytes(M, N), dev, f"nearest_points: {M} reference points / {N} queries are too many (>= 2^31)")
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    idx = torch.empty(N, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.dns_nearest_points(ptr(r), M, ptr(q), N, int(max_rings), 1 if method == "brute" else 0, ptr(ws), ptr(dist),
                                 ptr(idx), ptr(status), stream_ptr()), "dns_nearest_points")
    return dist, idx, status


def nearest_points(ref: torch.Tensor, query: torch.Tensor, method: str = "grid", max_rings: int = NEAREST_MAX_RINGS,
                   return_stats: bool = False):
    """ref [M,3] fp32, query [N,3] fp32 -> (dist [N] fp32, idx [N] int32): for every query the Euclidean distance to the nearest
    reference point and that point's index (``cKDTree(ref).query(query)`` of eval_3d.py:24-42; ties: the smaller index).
    ``method``: "grid" (cell grid of the reference cloud, Chebyshev rings up to ``max_rings``, the queries left over finished by
    the all-pairs kernel) or "brute" (the all-pairs kernel for every query); both return the same values.  ``M == 0`` with
    queries and non-finite coordinates raise ValueError.  One host read (the status words); ``return_stats`` appends
    ``{"brute_queries", "cells"}`` from them."""
    if query.dim() == 2 and query.shape[0] == 0 and query.shape[1] == 3:
        require_cuda(query)
        out = (torch.empty(0, dtype=torch.float32, device=query.device), torch.empty(0, dtype=torch.int32, device=query.device))
        return out + ({"brute_queries": 0, "cells": 0},) if return_stats else out
    dist, idx, status = nearest_points_launch(ref, query, method, max_rings)
    bad, n_brute, cells, _ = (int(x) for x in status.cpu().tolist())
    if bad:
        raise ValueError("nearest_points: non-finite coordinate in " + " and ".join(
            n for b, n in ((1, "ref"), (2, "query")) if bad & b))
    return (dist, idx, {"brute_queries": n_brute, "cells": cells}) if return_stats else (dist, idx)


ICP_STOP_REASONS = ("max_iter", "converged", "few_correspondences", "non_finite")     # status[3] of dns_icp_point_to_point


def _icp_arguments(source, target, max_dist, init, max_iter, relative_fitness, relative_rmse):
    s = source.detach().contiguous().float() if isinstance(source, torch.Tensor) else source
    t = target.detach().contiguous().float() if isinstance(target, torch.Tensor) else target
    require_cuda(s, t)
    if s.dim() != 2 or s.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"icp_point_to_point: source [N,3] and target [M,3], got {tuple(s.shape)} and {tuple(t.shape)}")
    if s.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError(f"icp_point_to_point: an empty cloud ({s.shape[0]} source points, {t.shape[0]} target points)")
    md = float(max_dist)
    if not (md > 0.0 and math.isfinite(md)):
        raise ValueError(f"icp_point_to_point: max_dist must be positive and finite, got {max_dist!r}")
    if int(max_iter) < 0:
        raise ValueError(f"icp_point_to_point: max_iter {max_iter}")
    if not (float(relative_fitness) >= 0.0 and float(relative_rmse) >= 0.0):
        raise ValueError("icp_point_to_point: relative_fitness and relative_rmse must be >= 0")
    t0 = None
    if init is not None:
        m = init.detach().cpu() if isinstance(init, torch.Tensor) else torch.as_tensor(init)
        m = m.to(torch.float64)
        if m.shape != (4, 4) or not bool(torch.isfinite(m).all()):
            raise ValueError("icp_point_to_point: init must be a finite [4,4] matrix")
        t0 = (C.c_double * 16)(*m.reshape(-1).tolist())
    return s, t, md, t0


def icp_point_to_point_launch(source: torch.Tensor, target: torch.Tensor, max_dist: float = 0.1, init=None, max_iter: int = 30,
                              relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_rings: int = NEAREST_MAX_RINGS):
    """``icp_point_to_point`` without its host read: -> (result [38] float64, status [4] int32, both on the device; the layout
    of include/dns_hip.h).  ``init`` is a host matrix (a device tensor is read back: pass a host one to keep this free of
    host reads)."""
    s, t, md, t0 = _icp_arguments(source, target, max_dist, init, max_iter, relative_fitness, relative_rmse)
    N, M = int(s.shape[0]), int(t.shape[0])
    dev = s.device
    ws = _byte_workspace(_rawlib.dns_icp_ws_bytes(M, N), dev, f"icp_point_to_point: {N} source / {M} target points are too many (>= 2^31)")
    result = torch.empty(38, dtype=torch.float64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.dns_icp_point_to_point(ptr(s), N, ptr(t), M, t0, md, int(max_iter), float(relative_fitness), float(relative_rmse),
                                     int(max_rings), ptr(ws), ptr(result), ptr(status), stream_ptr()), "dns_icp_point_to_point")
    return result, status


def icp_point_to_point(source: torch.Tensor, target: torch.Tensor, max_dist: float = 0.1, init=None, max_iter: int = 30,
                       relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, max_rings: int = NEAREST_MAX_RINGS):
    """open3d's ``registration_icp(source, target, max_dist, init, TransformationEstimationPointToPoint(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iter))`` (eval_3d.py:45-59) for source [N,3] and target [M,3]
    fp32 on the device, as one launch sequence (include/dns_hip.h) -> {"transformation": float64 [4,4] on the device (source ->
    target), "fitness", "inlier_rmse", "correspondences", "iterations" (updates applied), "converged", "stop" (one of
    ICP_STOP_REASONS), "brute_queries", "sums" (float64 [17] on the host: n, sum p', sum q, sum q p'^T, sum |p' - q|^2 of the last
    pass)}.  A correspondence is a nearest target point at a distance <= ``max_dist`` of the transformed source point.  CPU
    tensors, wrong shapes, empty clouds, non-finite coordinates and ``max_dist`` <= 0 or not finite raise ValueError.  One host
    read."""
    result, status = icp_point_to_point_launch(source, target, max_dist, init, max_iter, relative_fitness, relative_rmse, max_rings)
    host = torch.cat((result, status.double())).cpu()
    bad, n_brute, _, stop = (int(x) for x in host[38:].tolist())
    if bad:
        raise ValueError("icp_point_to_point: non-finite coordinate in " + " and ".join(
            n for b, n in ((1, "target"), (2, "source")) if bad & b))
    r = host[:38].tolist()
    return {"transformation": result[:16].view(4, 4), "fitness": r[16], "inlier_rmse": r[17], "correspondences": int(r[18]),
            "iterations": int(r[19]), "converged": bool(r[20]), "stop": ICP_STOP_REASONS[stop], "brute_queries": n_brute,
            "sums": host[21:38].numpy().copy()}


def frustum_seen(points: torch.Tensor, w2c: torch.Tensor, H: int, W: int, fx: float, fy: float, cx: float, cy: float):
    """points [P,3] fp32 world, w2c [K,4,4] fp32 world->camera -> seen [P] bool: some pose sees the point under check_proj of
    eval_3d.py:62-88 (cull_mesh.py:53-74) in fp32: x = -cam.x, z' = cam.z + 1e-5, u = (fx x + cx cam.z) / z', v = (fy cam.y +
    cy cam.z) / z'; seen iff -z' >= 0, 0 < u < W, 0 < v < H.  K = 0 sees nothing."""
    pts, w, K = _pose_args("frustum_seen", points, w2c)
    P, intr = int(pts.shape[0]), _intrinsics(fx, fy, cx, cy)
    seen = torch.empty(P, dtype=torch.uint8, device=pts.device)
    check(lib.dns_frustum_seen(ptr(pts), P, ptr(w), K, int(H), int(W), intr, ptr(seen), stream_ptr()), "dns_frustum_seen")
    return seen.bool()


# ----------------------------------------------------------------------------- 2-D evaluation (csrc/image_metrics.hip)
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIDE = 160                 # DNS_MS_SSIM_MIN_SIDE: min(H, W) must be larger
CONFUSION_LDS_CLASSES = 64             # DNS_CONFUSION_LDS_CLASSES: up to here the LDS histogram, above it global integer atomics


def ms_ssim_window() -> torch.Tensor:
    """The eleven fp32 window values the library filters with (host tensor)."""
    w = (C.c_float * 11)()
    _rawlib.dns_ms_ssim_window(w)
    return torch.tensor(list(w), dtype=torch.float32)


def _ms_ssim_arguments(pred, gt, depth):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError("ms_ssim: pred and gt must be tensors")
    if pred.shape != gt.shape:
        raise ValueError(f"ms_ssim: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3:
        raise ValueError(f"ms_ssim: images must be [H,W,3] or [F,H,W,3], got {tuple(pred.shape)}")
    single = pred.dim() == 3
    F, H, W = (1,) + tuple(pred.shape[:2]) if single else tuple(pred.shape[:3])
    if depth is not None and (not isinstance(depth, torch.Tensor) or tuple(depth.shape) != tuple(pred.shape[:-1])):
        raise ValueError(f"ms_ssim: depth must be {tuple(pred.shape[:-1])}, got "
                         f"{tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth)}")
    if min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"ms_ssim: images of {H} x {W}: the smaller side must be larger than {MS_SSIM_MIN_SIDE} "
                         f"(four 2x poolings ahead of an 11-tap window)")
    if F == 0:
        raise ValueError("ms_ssim: no frames")
    p = pred.detach().float().contiguous()
    g = gt.detach().float().contiguous()
    d = None if depth is None else depth.detach().float().contiguous()
    require_cuda(p, g, d)
    return p, g, d, single, int(F), int(H), int(W)


def _ms_ssim_torch(p, g, d, F, H, W):
    """The definition of include/dns_hip.h out of torch ops in fp32 (conv2d, avg_pool2d), for comparison and timing."""
    import torch.nn.functional as Fn
    win = ms_ssim_window().to(p.device)
    x, y = p.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
    kh, kw = win.view(1, 1, 11, 1).repeat(3, 1, 1, 1), win.view(1, 1, 1, 11).repeat(3, 1, 1, 1)
    filt = lambda t: Fn.conv2d(Fn.conv2d(t, kh, groups=3), kw, groups=3)
    terms = []
    for l in range(5):
        mx, my = filt(x), filt(y)
        sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        cs = (2 * sxy + 0.03 ** 2) / (sxx + syy + 0.03 ** 2)
        if l < 4:
            terms.append(cs.flatten(2).mean(-1))
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = Fn.avg_pool2d(x, 2, padding=pad), Fn.avg_pool2d(y, 2, padding=pad)
        else:
            terms.append(((2 * mx * my + 0.01 ** 2) / (mx * mx + my * my + 0.01 ** 2) * cs).flatten(2).mean(-1))
    levels = torch.stack(terms, 1).double()                                   # [F,5,3]
    wts = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=p.device).view(1, 5, 1)
    val = torch.prod(torch.relu(levels) ** wts, 1).mean(1)
    sq = (p - g).double() ** 2
    if d is None:
        n_valid = torch.full((F,), H * W, dtype=torch.int64, device=p.device)
        mse = sq.flatten(1).sum(1) / (3.0 * n_valid)
    else:
        m = d > 0
        n_valid = m.flatten(1).sum(1)
        mse = (sq * m[..., None]).flatten(1).sum(1) / (3.0 * n_valid)
    return val, mse, n_valid, levels


def ms_ssim_launch(pred: torch.Tensor, gt: torch.Tensor, depth: Optional[torch.Tensor] = None, method: str = "fused"):
    """``ms_ssim`` without a host read: -> (ms_ssim [F] float64, mse [F] float64, n_valid [F] int64, levels [F,5,3] float64), all
    on the device; F = 1 for [H,W,3] images."""
    if method not in ("fused", "torch"):
        raise ValueError(f"ms_ssim: method must be 'fused' or 'torch', got {method!r}")
    p, g, d, _, F, H, W = _ms_ssim_arguments(pred, gt, depth)
    if method == "torch":
        return _ms_ssim_torch(p.view(F, H, W, 3), g.view(F, H, W, 3), None if d is None else d.view(F, H, W), F, H, W)
    dev = p.device
    ws = _byte_workspace(_rawlib.dns_ms_ssim_ws_bytes(F, H, W), dev,
                         f"ms_ssim: {F} frames of {H} x {W} are refused (at most 65535 frames, sides <= 32768)")
    val = torch.empty(F, dtype=torch.float64, device=dev)
    mse = torch.empty(F, dtype=torch.float64, device=dev)
    n_valid = torch.empty(F, dtype=torch.int64, device=dev)
    levels = torch.empty(F, 5, 3, dtype=torch.float64, device=dev)
    check(lib.dns_ms_ssim(ptr(p), ptr(g), ptr(d), F, H, W, ptr(ws), ptr(val), ptr(mse), ptr(n_valid), ptr(levels), stream_ptr()),
          "dns_ms_ssim")
    return val, mse, n_valid, levels


def ms_ssim(pred: torch.Tensor, gt: torch.Tensor, depth: Optional[torch.Tensor] = None, method: str = "fused"):
    """``pytorch_msssim.ms_ssim(data_range=1.0, size_average=True)`` (eval_2d.py:302) and the masked MSE of eval_2d.py:299 for
    image pairs pred, gt [H,W,3] or [F,H,W,3] fp32 on the device, in the project's image layout (include/dns_hip.h has the
    definition) -> {"ms_ssim", "mse": float64 [F] (0-d for one image), "n_valid": int64, "levels": float64 [F,5,3] ([5,3])}, device
    tensors.  ``depth`` [H,W] / [F,H,W]: the MSE runs over the pixels with depth > 0 (all pixels without it; NaN where none is
    valid).  ``method="torch"`` composes the same definition from torch ops in fp32.  min(H, W) <= 160, mismatched shapes and CPU
    tensors raise ValueError before anything is launched."""
    single = isinstance(pred, torch.Tensor) and pred.dim() == 3
    val, mse, n_valid, levels = ms_ssim_launch(pred, gt, depth, method)
    if single:
        val, mse, n_valid, levels = val[0], mse[0], n_valid[0], levels[0]
    return {"ms_ssim": val, "mse": mse, "n_valid": n_valid, "levels": levels}


def _labels_int32(t, n_class):
    """Label image -> int32 on the device; whatever is not an integer in [0, n_class) (fractions, NaN, out of range) becomes -1."""
    ok = (t >= 0) & (t < n_class)
    if t.is_floating_point():
        ok = ok & (t == torch.floor(t))
    elif t.dtype == torch.bool:
        t = t.to(torch.int32)
    return torch.where(ok, t, torch.full_like(t, -1)).to(torch.int32).contiguous()


def label_confusion(gt: torch.Tensor, pred: torch.Tensor, n_class: int):
    """Confusion matrix of label images gt, pred of one shape on the device: [N] or [H,W] (one pair) -> (conf [n_class,n_class]
    int64, n_invalid 0-d int64); [F,H,W] (F pairs) -> (conf [F,n_class,n_class], n_invalid [F]).  conf[g,p] counts the pixels with
    gt g and pred p; a pixel whose gt or pred is not an integer in [0, n_class) is counted in n_invalid only.  Integer and
    floating-point label images are accepted (``frames["gt_label"]`` is float, ``render_frame``'s arg-max int64); the conversion
    to int32 runs on the device.  No host read."""
    if not isinstance(gt, torch.Tensor) or not isinstance(pred, torch.Tensor):
        raise ValueError("label_confusion: gt and pred must be tensors")
    require_cuda(gt.contiguous(), pred.contiguous())
    if gt.shape != pred.shape or gt.dim() not in (1, 2, 3):
        raise ValueError(f"label_confusion: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must share a shape [N], [H,W] or [F,H,W]")
    nc = int(n_class)
    if not 1 <= nc <= 4096:
        raise ValueError(f"label_confusion: n_class {n_class} (must be 1..4096)")
    batched = gt.dim() == 3
    F = int(gt.shape[0]) if batched else 1
    if F > 65535:
        raise ValueError(f"label_confusion: {F} frames (must be <= 65535)")
    g, p = _labels_int32(gt.detach(), nc), _labels_int32(pred.detach(), nc)
    N = g.numel() // F if F else 0
    conf = torch.empty(F, nc, nc, dtype=torch.int64, device=g.device)
    n_invalid = torch.empty(F, dtype=torch.int64, device=g.device)
    check(lib.dns_label_confusion(ptr(g), ptr(p), F, N, nc, ptr(conf), ptr(n_invalid), stream_ptr()), "dns_label_confusion")
    return (conf, n_invalid) if batched else (conf[0], n_invalid[0])


# ----------------------------------------------------------------------------- Depth L1 (csrc/mesh_raster.hip)
RASTER_SMALL_BOX = 8                   # RS_SMALL: the largest pixel box a set-up thread draws itself
DEPTH_L1_PARTS = 64                    # DNS_DEPTH_L1_PARTS
RASTER_METHODS = ("auto", "simple")


def _raster_arguments(verts, faces, w2c, H, W, method):
    if not all(isinstance(t, torch.Tensor) for t in (verts, faces, w2c)):
        raise ValueError("rasterize_depth: verts, faces and w2c must be tensors")
    v, w, _ = _pose_args("rasterize_depth", verts, w2c)
    f = faces.detach().contiguous()
    require_cuda(f)
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"rasterize_depth: faces [F,3], got {tuple(f.shape)}")
    if f.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"rasterize_depth: faces must be int32 or int64, got {f.dtype}")
    if method not in RASTER_METHODS:
        raise ValueError(f"rasterize_depth: method must be one of {RASTER_METHODS}, got {method!r}")
    if not (1 <= int(H) <= 32768 and 1 <= int(W) <= 32768):
        raise ValueError(f"rasterize_depth: image {H} x {W} (sides must be 1..32768)")
    return v, f, w


def _check_face_indices(f, P):
    """ValueError when a face holds an index outside [0, P) (one host read)."""
    if f.numel():
        lo, hi = (int(x) for x in torch.stack((f.min(), f.max())).cpu().tolist())
        if lo < 0 or hi >= P:
            raise ValueError(f"rasterize_depth: a face holds a vertex index outside [0, {P}) (min {lo}, max {hi})")


def _raster_launch_arguments(who, check_indices, verts, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, method, stats):
    """The arguments the two rasterisers share, validated once, ``who`` naming the caller in the camera messages: -> (v, f as
    int32, w, z_near, z_far, P, F, V, the flag bits of ``method`` and ``stats``).  ``check_indices``: the checked entry points'
    host read of the face indices, made before anything is allocated or launched."""
    v, f, w = _raster_arguments(verts, faces, w2c, H, W, method)
    if check_indices:
        _check_face_indices(f, int(v.shape[0]))
    zn, zf = float(z_near), float(z_far)
    if not (zn > 0.0 and zf >= zn and math.isfinite(zf)):
        raise ValueError(f"{who}: need 0 < z_near <= z_far < inf, got {z_near!r}, {z_far!r}")
    if not (all(math.isfinite(float(x)) for x in (fx, fy, cx, cy)) and float(fx) != 0.0 and float(fy) != 0.0):
        raise ValueError(f"{who}: the intrinsics must be finite, fx and fy non-zero")
    flags = (1 if method == "simple" else 0) | (2 if stats else 0)
    return v, f.to(torch.int32), w, zn, zf, int(v.shape[0]), int(f.shape[0]), int(w.shape[0]), flags


def _rasterize_depth(check_indices, verts, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, method, stats, list_cap):
    v, f, w, zn, zf, P, F, V, flags = _raster_launch_arguments("rasterize_depth", check_indices, verts, faces, w2c, H, W, fx, fy, cx, cy,
                                                               z_near, z_far, method, stats)
    dev = v.device
    depth = torch.empty(V, int(H), int(W), dtype=torch.float32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    if V == 0:
        return depth, status
    ws = _byte_workspace(_rawlib.dns_rasterize_ws_bytes(F, V, int(H), int(W)), dev,
                         f"rasterize_depth: {F} faces at {H} x {W} are refused (F >= 2^31)")
    check(lib.dns_rasterize_depth(ptr(v), P, ptr(f), F, ptr(w), V, int(H), int(W), _intrinsics(fx, fy, cx, cy), zn, zf, flags, int(list_cap), ptr(ws),
                                  ptr(depth), ptr(status), stream_ptr()), "dns_rasterize_depth")
    return depth, status


def rasterize_depth_launch(verts, faces, w2c, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0, method="auto", stats=False,
                           list_cap=0):
    """``rasterize_depth`` without its host reads: -> (depth [V,H,W] fp32, status [4] int32 on the device; include/dns_hip.h).
    The face indices are NOT validated here (a face with an index outside [0, P) is skipped by the kernel and flagged in
    status[0] bit 1); int64 faces must fit int32.  ``list_cap``: pairs per launch (0: the library's default)."""
    return _rasterize_depth(False, verts, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, method, stats, list_cap)


def rasterize_depth(verts: torch.Tensor, faces: torch.Tensor, w2c: torch.Tensor, H: int, W: int, fx: float, fy: float, cx: float,
                    cy: float, z_near: float = 0.01, z_far: float = 20.0, method: str = "auto", return_stats: bool = False):
    """Depth images of a triangle mesh: verts [P,3] fp32, faces [F,3] int32, w2c [V,4,4] fp32 world->camera in the OpenCV
    convention (x right, y down, z forward) -> depth [V,H,W] fp32: camera-space z of the nearest surface through each pixel
    centre (centres at integer coordinates), 0 where nothing is seen; both faces of a triangle are drawn; nothing nearer than
    ``z_near`` or beyond ``z_far``.  The arithmetic is written out in include/dns_hip.h; the image is the same bits for every
    call and both methods.  ``method``: "auto" (small boxes by the set-up thread, the others by a workgroup each) or "simple"
    (every triangle by its set-up thread).  A face index outside [0, P) and CPU tensors raise ValueError (one host read for the
    indices).  ``return_stats`` appends {"nonfinite": a triangle with a non-finite vertex was skipped, "large": (triangle, view)
    pairs drawn through the list, "small": pairs drawn by their set-up thread} (a second host read)."""
    depth, status = _rasterize_depth(True, verts, faces, w2c, H, W, fx, fy, cx, cy, z_near, z_far, method, return_stats, 0)
    if not return_stats:
        return depth
    bad, large, small, _ = (int(x) for x in status.cpu().tolist())
    return depth, {"nonfinite": bool(bad & 1), "large": large, "small": small}


def depth_l1(a: torch.Tensor, b: torch.Tensor):
    """a, b [V,H,W] fp32 on the device -> err [V] float64 = mean |a - b| over ALL pixels of each view (zeros of the background
    included, as the reference's ``np.abs(gt_depth - ours_depth).mean()``), differences and sums in float64 in a fixed order: the
    same bits for every call.  No host read."""
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
        raise ValueError("depth_l1: a and b must be tensors")
    x, y = a.detach().contiguous().float(), b.detach().contiguous().float()
    require_cuda(x, y)
    if x.dim() != 3 or x.shape != y.shape:
        raise ValueError(f"depth_l1: two stacks [V,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    V, H, W = (int(s) for s in x.shape)
    if V and not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"depth_l1: image {H} x {W} (sides must be 1..32768)")
    err = torch.empty(V, dtype=torch.float64, device=x.device)
    if V == 0:
        return err
    partial = torch.empty(V * DEPTH_L1_PARTS, dtype=torch.float64, device=x.device)
    check(lib.dns_depth_l1(ptr(x), ptr(y), V, H, W, ptr(partial), ptr(err), stream_ptr()), "dns_depth_l1")
    return err


def views_see_any(points: torch.Tensor, w2c: torch.Tensor, H: int, W: int, fx: float, fy: float, cx: float, cy: float):
    """points [N,3] fp32 world, w2c [K,4,4] fp32 world->camera in ``frustum_seen``'s convention -> sees [K] bool: pose k sees at
    least one of the points, under exactly ``frustum_seen``'s projection and inequalities (``frustum_seen`` answers per point,
    this per pose).  No host read."""
    if not isinstance(points, torch.Tensor) or not isinstance(w2c, torch.Tensor):
        raise ValueError("views_see_any: points and w2c must be tensors")
    pts, w, K = _pose_args("views_see_any", points, w2c)
    sees = torch.empty(K, dtype=torch.uint8, device=w.device)
    check(lib.dns_views_see_any(ptr(pts), int(pts.shape[0]), ptr(w), K, int(H), int(W), _intrinsics(fx, fy, cx, cy), ptr(sees),
                                stream_ptr()), "dns_views_see_any")
    return sees.bool()


# ----------------------------------------------------------------------------- headless visualiser (csrc/mesh_render.hip)
RENDER_CULL = (None, "back", "front")
RENDER_SHADE = (None, "headlight")
RENDER_MAX_POINT_SIZE = 16
_RENDER_CULL_FLAGS = {None: 0, "back": 4, "front": 8}          # DNS_RENDER_CULL_BACK, DNS_RENDER_CULL_FRONT
_RENDER_HEADLIGHT = 16                                         # DNS_RENDER_HEADLIGHT


def _render_colors(who, what, colors, n, dev):
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or tuple(colors.shape) != (n, 3):
        got = (tuple(colors.shape), colors.dtype) if isinstance(colors, torch.Tensor) else type(colors).__name__
        raise ValueError(f"{who}: {what} must be a fp32 tensor [{n},3], got {got}")
    c = colors.detach().contiguous()
    require_cuda(c)
    return c


def _render_mesh(check_indices, verts, faces, colors, w2c, H, W, fx, fy, cx, cy, *, z_near, z_far, cull, shade, ambient, background,
                 points, point_colors, point_size, method, list_cap, stats):
    who = "render_mesh"
    v, f, w, zn, zf, P, F, V, flags = _raster_launch_arguments(who, check_indices, verts, faces, w2c, H, W, fx, fy, cx, cy, z_near,
                                                               z_far, method, stats)
    if cull not in RENDER_CULL:
        raise ValueError(f"{who}: cull must be one of {RENDER_CULL}, got {cull!r}")
    if shade not in RENDER_SHADE:
        raise ValueError(f"{who}: shade must be one of {RENDER_SHADE}, got {shade!r}")
    amb = float(ambient)
    if not 0.0 <= amb <= 1.0:
        raise ValueError(f"{who}: ambient must be in [0, 1], got {ambient!r}")
    if isinstance(point_size, bool) or int(point_size) != point_size or not 1 <= int(point_size) <= RENDER_MAX_POINT_SIZE:
        raise ValueError(f"{who}: point_size must be an integer in 1..{RENDER_MAX_POINT_SIZE}, got {point_size!r}")
    bg = tuple(float(x) for x in background)
    if len(bg) != 3 or not all(math.isfinite(x) for x in bg):
        raise ValueError(f"{who}: background must be three finite numbers, got {background!r}")
    dev = v.device
    col = _render_colors(who, "colors", colors, P, dev)
    if (points is None) != (point_colors is None):
        raise ValueError(f"{who}: points and point_colors come together")
    pts = pcol = None
    N = 0
    if points is not None:
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"{who}: points must be a tensor [N,3]")
        pts = points.detach().contiguous().float()
        require_cuda(pts)
        N = int(pts.shape[0])
        pcol = _render_colors(who, "point_colors", point_colors, N, dev)
    H, W = int(H), int(W)
    out = {"color": torch.empty(V, H, W, 3, dtype=torch.float32, device=dev),
           "depth": torch.empty(V, H, W, dtype=torch.float32, device=dev),
           "index": torch.empty(V, H, W, dtype=torch.int32, device=dev),
           "status": torch.zeros(4, dtype=torch.int32, device=dev)}
    if V == 0:
        return out
    ws = _byte_workspace(_rawlib.dns_render_mesh_ws_bytes(F, V, H, W), dev, f"{who}: {F} faces at {H} x {W} are refused (F >= 2^31)")
    flags |= _RENDER_CULL_FLAGS[cull] | (_RENDER_HEADLIGHT if shade else 0)
    check(lib.dns_render_mesh(ptr(v), P, ptr(f), F, ptr(col), ptr(pts), ptr(pcol), N, int(point_size), ptr(w), V, H, W,
                              _intrinsics(fx, fy, cx, cy), zn, zf, flags, amb, (C.c_float * 3)(*bg), int(list_cap or 0), ptr(ws),
                              ptr(out["color"]), ptr(out["depth"]), ptr(out["index"]), ptr(out["status"]), stream_ptr()),
          "dns_render_mesh")
    return out


def render_mesh_launch(verts, faces, colors, w2c, H, W, fx, fy, cx, cy, *, z_near=0.01, z_far=20.0, cull=None, shade=None,
                       ambient=0.3, background=(1, 1, 1), points=None, point_colors=None, point_size=4, method="auto",
                       list_cap=None, stats=False):
    """``render_mesh`` without its host read: the face indices are NOT validated (a face with an index outside [0, P) is skipped
    by the kernel and flagged in status[0] bit 1); int64 faces must fit int32."""
    return _render_mesh(False, verts, faces, colors, w2c, H, W, fx, fy, cx, cy, z_near=z_near, z_far=z_far, cull=cull, shade=shade,
                        ambient=ambient, background=background, points=points, point_colors=point_colors, point_size=point_size,
                        method=method, list_cap=list_cap, stats=stats)


def render_mesh(verts: torch.Tensor, faces: torch.Tensor, colors: torch.Tensor, w2c: torch.Tensor, H: int, W: int, fx: float,
                fy: float, cx: float, cy: float, *, z_near: float = 0.01, z_far: float = 20.0, cull: Optional[str] = None,
                shade: Optional[str] = None, ambient: float = 0.3, background=(1, 1, 1), points: Optional[torch.Tensor] = None,
                point_colors: Optional[torch.Tensor] = None, point_size: int = 4, method: str = "auto",
                list_cap: Optional[int] = None, stats: bool = False):
    """Colour images of a triangle mesh with vertex colours and of a point cloud: verts [P,3] fp32, faces [F,3] int32, colors
    [P,3] fp32, w2c [V,4,4] (``rasterize_depth``'s convention and arguments) -> {"color" [V,H,W,3] fp32, "depth" [V,H,W] fp32,
    "index" [V,H,W] int32, "status" [4] int32}, device tensors.  ``index`` is the face seen through the pixel centre, -1 for the
    background and -2 - k for point k; ``depth`` is ``rasterize_depth``'s image bit for bit when nothing is culled and there are
    no points.  The nearest surface wins; at equal depth the lower face index, and a triangle before a point: the images are the
    same bits for every call, both methods and every ``list_cap``.  Colours are interpolated perspective-correctly.
    ``cull``: None, "back" or "front" -- a face is front-facing when the normal of its winding points at the camera.
    ``shade``: None or "headlight" (colour times ambient + (1 - ambient) |cos| of the angle between the face normal and the pixel
    ray: flat and two-sided).  ``points`` [N,3] with ``point_colors`` [N,3] fp32 are squares of ``point_size`` (1..16) pixels,
    depth-tested against the mesh and each other, never shaded.  ``status``: [0] bit 0 a triangle with a non-finite vertex was
    skipped, bit 2 a non-finite point was; [1] (triangle, view) pairs drawn through the list; [2] pairs drawn by their set-up
    thread (with ``stats``).  The arithmetic is written out in include/dns_hip.h.  A face index outside [0, P), CPU tensors,
    colours that are not fp32 [P,3] / [N,3], an unknown ``cull``, ``shade`` or ``method``, ``point_size`` outside 1..16 and
    ``ambient`` outside [0, 1] raise ValueError (one host read for the indices)."""
    return _render_mesh(True, verts, faces, colors, w2c, H, W, fx, fy, cx, cy, z_near=z_near, z_far=z_far, cull=cull, shade=shade,
                        ambient=ambient, background=background, points=points, point_colors=point_colors, point_size=point_size,
                        method=method, list_cap=list_cap, stats=stats)


# ----------------------------------------------------------------------------- TSDF fusion (csrc/tsdf.hip)
TSDF_UNIT = 16


def tsdf_multiplier(H: int, W: int, cam: dict) -> np.ndarray:
    """[H,W] fp32: the camera-distance multiplier sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) of pixel (v, u), evaluated in
    float64 on the host (numpy: correctly rounded division and square root) and rounded to fp32 once."""
    u = (np.arange(W, dtype=np.float64) - float(cam["cx"])) / float(cam["fx"])
    v = (np.arange(H, dtype=np.float64) - float(cam["cy"])) / float(cam["fy"])
    return np.sqrt((u * u)[None, :] + (v * v)[:, None] + 1.0).astype(np.float32)


def _tsdf_intrinsics(cam):
    return (C.c_double * 4)(float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]))


def tsdf_fuse(depths: torch.Tensor, extrinsic: torch.Tensor, pose: torch.Tensor, cam: dict, voxel_length: float, sdf_trunc: float,
              stride: int = 4, *, table_slots: Optional[int] = None):
    """TSDF fusion of K posed depth images into units of 16^3 voxels (Open3D's ScalableTSDFVolume.integrate per frame, as
    tests/tsdf_ref.py restates it; include/dns_hip.h states every expression).  depths [K,H,W] fp32; extrinsic [K,4,4] float64
    world->camera and pose [K,4,4] float64 = its inverse, both in Open3D's convention (the camera looks along +z); cam
    {'fx','fy','cx','cy'}.  -> (units [B,3] int32, lexicographically sorted; tsdf [B,16,16,16] fp32; weight [B,16,16,16] fp32).
    Frame k is integrated only into the units its pixels (every ``stride``-th row and column, 0 < depth < 1000) touch, in
    ascending k.  No float atomics: the same bits for every call, and for every ``table_slots`` (the first size of the key table;
    a table that turns out too small is doubled and the pass repeated).  One host read per attempt."""
    for name, t, dt in (("depths", depths, torch.float32), ("extrinsic", extrinsic, torch.float64), ("pose", pose, torch.float64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"tsdf_fuse: {name} must be a {dt} tensor")
        if not t.is_cuda:
            raise ValueError(f"tsdf_fuse: {name} must be on the GPU (there is no CPU fallback)")
    if depths.dim() != 3:
        raise ValueError(f"tsdf_fuse: depths must be [K,H,W], got {tuple(depths.shape)}")
    K, H, W = (int(s) for s in depths.shape)
    for name, t in (("extrinsic", extrinsic), ("pose", pose)):
        if tuple(t.shape) != (K, 4, 4):
            raise ValueError(f"tsdf_fuse: {name} must be [{K},4,4], got {tuple(t.shape)}")
    if K > 65535:
        raise ValueError(f"tsdf_fuse: depths holds {K} keyframes; at most 65535 (the frame is 16 bits of a key)")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"tsdf_fuse: stride must be >= 1, got {stride}")
    vl, tr = float(voxel_length), float(sdf_trunc)
    if not (vl > 0 and tr > 0 and math.isfinite(vl) and math.isfinite(tr) and 2 * tr < TSDF_UNIT * vl):
        raise ValueError(f"tsdf_fuse: voxel_length and sdf_trunc must be positive with 2 sdf_trunc < 16 voxel_length, got {vl}, {tr}")
    dev = depths.device
    dep, ext, pos = depths.detach().contiguous(), extrinsic.detach().contiguous(), pose.detach().contiguous()
    empty = (torch.zeros(0, 3, dtype=torch.int32, device=dev), torch.zeros(0, 16, 16, 16, device=dev), torch.zeros(0, 16, 16, 16, device=dev))
    if K == 0 or H == 0 or W == 0:
        return empty
    intr = _tsdf_intrinsics(cam)
    n_samples = K * ((H + stride - 1) // stride) * ((W + stride - 1) // stride)
    cap = int(table_slots) if table_slots is not None else max(4096, min(n_samples, 1 << 26))
    if cap < 8:
        raise ValueError(f"tsdf_fuse: table_slots must be >= 8, got {cap}")
    status = torch.empty(1, dtype=torch.int32, device=dev)
    while True:
        if cap >= 1 << 31:
            raise ValueError("tsdf_fuse: depths touch more than 2^31 (unit, frame) pairs")
        table = torch.empty(cap, dtype=torch.int64, device=dev)
        check(lib.dns_tsdf_touch(ptr(dep), ptr(pos), K, H, W, stride, intr, vl, tr, ptr(table), cap, ptr(status), stream_ptr()),
              "dns_tsdf_touch")
        st = int(status.item())
        if st & 2:
            raise ValueError("tsdf_fuse: pose / voxel_length put a unit index outside 16 bits (|coordinate| >= 32768 * 16 * voxel_length)")
        if not st & 1:
            break
        cap *= 2
    keys = torch.sort(table[table != -1]).values
    if keys.numel() == 0:
        return empty
    uniq, counts = torch.unique_consecutive(keys >> 16, return_counts=True)
    frames = (keys & 0xFFFF).to(torch.int32)
    offset = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
    offset[1:] = torch.cumsum(counts, 0)
    units = torch.stack((uniq >> 32, ((uniq >> 16) & 0xFFFF) - 32768, (uniq & 0xFFFF) - 32768), 1).to(torch.int32).contiguous()
    B = int(units.shape[0])
    if B > 1 << 20:                                                  # 2^32 voxels, 32 GiB of tsdf and weight
        raise ValueError(f"tsdf_fuse: voxel_length gives {B} units of 16^3 voxels (at most 2^20)")
    mult = torch.from_numpy(tsdf_multiplier(H, W, cam)).to(dev)
    tsdf = torch.empty(B, 16, 16, 16, device=dev)
    weight = torch.empty(B, 16, 16, 16, device=dev)
    check(lib.dns_tsdf_integrate(ptr(units), B, ptr(offset), ptr(frames), ptr(dep), ptr(ext), ptr(mult), K, H, W, intr, vl, tr, ptr(tsdf),
                                 ptr(weight), stream_ptr()), "dns_tsdf_integrate")
    return units, tsdf, weight


def tsdf_vertices(units: torch.Tensor, tsdf: torch.Tensor, weight: torch.Tensor, voxel_length: float) -> torch.Tensor:
    """The vertices of the TSDF's zero crossing (Open3D's extract_triangle_mesh().vertices; faces are not built): units [B,3] int32
    sorted as ``tsdf_fuse`` returns them, tsdf / weight [B,16,16,16] fp32 -> [V,3] float64, ordered by unit, voxel, axis, without
    duplicates.  One host read (the total)."""
    for name, t, dt in (("units", units, torch.int32), ("tsdf", tsdf, torch.float32), ("weight", weight, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f"tsdf_vertices: {name} must be a {dt} tensor")
        if not t.is_cuda:
            raise ValueError(f"tsdf_vertices: {name} must be on the GPU (there is no CPU fallback)")
    if units.dim() != 2 or units.shape[1] != 3:
        raise ValueError(f"tsdf_vertices: units must be [B,3], got {tuple(units.shape)}")
    B = int(units.shape[0])
    for name, t in (("tsdf", tsdf), ("weight", weight)):
        if tuple(t.shape) != (B, 16, 16, 16):
            raise ValueError(f"tsdf_vertices: {name} must be [{B},16,16,16], got {tuple(t.shape)}")
    vl = float(voxel_length)
    if not (vl > 0 and math.isfinite(vl)):
        raise ValueError(f"tsdf_vertices: voxel_length must be positive, got {vl}")
    dev = units.device
    if B == 0:
        return torch.zeros(0, 3, dtype=torch.float64, device=dev)
    u, t, w = units.detach().contiguous(), tsdf.detach().contiguous(), weight.detach().contiguous()
    if B > 1:
        key = (u[:, 0].long() << 32) | ((u[:, 1].long() + 32768) << 16) | (u[:, 2].long() + 32768)
        if bool((u.abs().max() > 32767)) or not bool((key[1:] > key[:-1]).all()):
            raise ValueError("tsdf_vertices: units must be distinct, sorted lexicographically and within 16 bits (as tsdf_fuse returns them)")
    count = torch.empty(B, dtype=torch.int64, device=dev)
    check(lib.dns_tsdf_vertex_count(ptr(u), B, ptr(t), ptr(w), ptr(count), stream_ptr()), "dns_tsdf_vertex_count")
    incl = torch.cumsum(count, 0)
    V = int(incl[-1].item())
    verts = torch.empty(V, 3, dtype=torch.float64, device=dev)
    if V:
        offset = (incl - count).contiguous()
        check(lib.dns_tsdf_vertex_emit(ptr(u), B, ptr(t), ptr(w), vl, ptr(offset), ptr(verts), V, stream_ptr()), "dns_tsdf_vertex_emit")
    return verts


# ----------------------------------------------------------------------------- convex hull (csrc/hull.hip)
def convex_hull_launch(points: torch.Tensor, eps: float = 0.0, face_cap: Optional[int] = None):
    """``convex_hull`` with its bookkeeping: -> (faces [F,3] int64, planes [F,4] float64, info) with info = {'max_outside',
    'rounds', 'sweeps', 'scale', 'face_cap'}.  ``face_cap`` bounds the faces ever made (replaced ones included); too small a bound
    is quadrupled and the hull rebuilt."""
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise ValueError("convex_hull: points must be a float32 or float64 tensor")
    if not points.is_cuda:
        raise ValueError("convex_hull: points must be on the GPU (there is no CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"convex_hull: points must be [N,3], got {tuple(points.shape)}")
    N = int(points.shape[0])
    if N < 4:
        raise ValueError(f"convex_hull: points holds {N} points; a hull in 3-D needs at least 4")
    if N >= 1 << 31:
        raise ValueError(f"convex_hull: points holds {N} points (must be < 2^31)")
    eps = float(eps)
    if not (eps >= 0 and math.isfinite(eps)):
        raise ValueError(f"convex_hull: eps must be finite and >= 0, got {eps}")
    pts = points.detach().double().contiguous()
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("convex_hull: points must be finite")
    cap = int(face_cap) if face_cap is not None else 1 << 14
    if cap < 4:
        raise ValueError(f"convex_hull: face_cap must be >= 4, got {cap}")
    st = stream_ptr()
    while True:
        ws = _byte_workspace(_rawlib.dns_convex_hull_ws_bytes(N, cap), pts.device,
                             f"convex_hull: the hull of points needs more than {cap} faces")
        faces = np.empty((cap, 3), np.int32)
        planes = np.empty((cap, 4), np.float64)
        nf = C.c_uint32(0)
        info = (C.c_double * 4)()
        rc = lib.dns_convex_hull(ptr(pts), N, eps, ptr(ws), cap, C.c_void_p(faces.ctypes.data), C.c_void_p(planes.ctypes.data), C.byref(nf),
                                 info, st)
        if rc != 1:
            break
        cap *= 4
    check(rc, "dns_convex_hull")
    F = int(nf.value)
    return (torch.from_numpy(faces[:F].astype(np.int64)).to(pts.device), torch.from_numpy(planes[:F].copy()).to(pts.device),
            {"max_outside": float(info[0]), "rounds": int(info[1]), "sweeps": int(info[2]), "scale": float(info[3]), "face_cap": cap})


def convex_hull(points: torch.Tensor, eps: float = 0.0):
    """The convex hull of points [N,3] (float64, or float32 widened) by quickhull in float64 -> (vertex_index [h] int64 ascending:
    the points that are hull vertices; faces [F,3] int64 into points, outward orientation; planes [F,4] float64: unit outward
    normal n and d, a point is inside when n . x + d <= 0 for every row, which is what ``meshing.inside_planes`` consumes;
    max_outside: the MEASURED maximum of n . x + d over all points and faces).  A face sees a point above ``eps`` (+ 1e-12 of the
    largest coordinate), so the hull under-approximates by at most that much and skips the points that would move it by less.
    Fewer than 4 points, or points within eps of one plane, are a ValueError.  The call reads 40 bytes back and synchronises once
    per inserted point: it cannot be captured into a graph (csrc/hull_topology.hpp)."""
    faces, planes, info = convex_hull_launch(points, eps)
    return torch.unique(faces.reshape(-1)), faces, planes, info["max_outside"]


# ----------------------------------------------------------------------------- image stem (csrc/stem.hip)
STEM_STATS, STEM_EPILOGUE, STEM_STORE = 1, 2, 4          # include/dns_hip.h: flags of dns_stem_forward
_STEM_CACHE = {}


def _stem_constants(conv_weight, bn_weight, bn_bias, running_mean, running_var, eps):
    """The packed [148][64] weight image and the frozen-mode (s, t) [2][64], computed in float64 from the parameters (torch ops on
    the device, no read-back) and cached per parameter version (address and ``_version``: a write through ``.data`` is not seen).
    An entry holds its parameters, so that no other tensor can take their addresses while it lives."""
    params = (conv_weight, bn_weight, bn_bias, running_mean, running_var)
    key = tuple((t.data_ptr(), t._version) for t in params) + (float(eps),)
    hit = _STEM_CACHE.get(key)
    if hit is not None:
        return hit[0], hit[1]
    wpack = torch.zeros(148, 64, device=conv_weight.device)
    wpack[:147] = conv_weight.detach().permute(2, 3, 1, 0).reshape(147, 64)             # row (ky 7 + kx) 3 + c, column o
    s = bn_weight.detach().double() / torch.sqrt(running_var.detach().double() + float(eps))
    t = bn_bias.detach().double() - running_mean.detach().double() * s
    st = torch.stack((s, t)).float().contiguous()
    if len(_STEM_CACHE) >= 8:
        _STEM_CACHE.clear()
    _STEM_CACHE[key] = (wpack, st, params)
    return wpack, st


def stem_out_shape(H: int, W: int):
    """(h, w) of the stem maps of H x W images: conv 7x7, stride 2, padding 3."""
    return (int(H) - 1) // 2 + 1, (int(W) - 1) // 2 + 1


def stem_forward(images: torch.Tensor, conv_weight: torch.Tensor, bn_weight: torch.Tensor, bn_bias: torch.Tensor,
                 running_mean: torch.Tensor, running_var: torch.Tensor, eps: float = 1e-5, *, batch_stats: bool = False,
                 out: Optional[torch.Tensor] = None, batch_apply: str = "inplace") -> torch.Tensor:
    """The image stem (reference models/layers.py:56-58,95-98): conv 7x7 stride 2 pad 3 (``conv_weight`` [64,3,7,7], exact fp32) +
    batch-norm + ReLU of channels-last ``images`` [n,H,W,3] -> channels-last maps [n,h,w,64], h = (H-1)//2 + 1, w = (W-1)//2 + 1:
    the layout ``feature_gather`` and ``keyframe_codes`` read, written once.

    ``batch_stats=False``: the frozen statistics, nn.BatchNorm2d in eval() mode -- y = relu(conv s + t) with
    s = weight / sqrt(running_var + eps), t = bias - running_mean s.  The bits of an image's map depend on the image alone.
    ``batch_stats=True``: nn.BatchNorm2d in TRAIN mode, which is what the reference's never-eval()-ed stem computes: mean and biased
    variance over the n h w values of each channel of THIS call (float64 sums of the fp32 conv values, added in a fixed order: the
    same bits for every call); the running statistics are neither read nor updated.  ``batch_apply``: 'inplace' stores the raw
    convolution and normalises it in place, 'recompute' runs the convolution a second time; both give the same bits.

    ``out``: a contiguous [n,h,w,64] fp32 tensor, e.g. a slice of a [K,h,w,64] stack, written in place and returned.  No host
    read-back; ValueError for a wrong dtype, device, rank, channel count or shape, for non-contiguous ``images`` / ``out``, and for
    batch statistics of a single value (n h w = 1), which torch refuses too."""
    params = (conv_weight, bn_weight, bn_bias, running_mean, running_var)
    for t in (images,) + params + ((out,) if out is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("stem_forward: every tensor must be on the GPU (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"stem_forward: every tensor must be float32, got {t.dtype}")
        if t.device != images.device:
            raise ValueError("stem_forward: all tensors must be on one device")
    if images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"stem_forward: images must be channels-last [n,H,W,3], got {tuple(images.shape)}")
    if not images.is_contiguous():
        raise ValueError("stem_forward: images must be contiguous")
    if tuple(conv_weight.shape) != (64, 3, 7, 7):
        raise ValueError(f"stem_forward: conv_weight must be [64,3,7,7], got {tuple(conv_weight.shape)}")
    for name, t in (("bn_weight", bn_weight), ("bn_bias", bn_bias), ("running_mean", running_mean), ("running_var", running_var)):
        if tuple(t.shape) != (64,) or not t.is_contiguous():
            raise ValueError(f"stem_forward: {name} must be a contiguous [64] tensor, got {tuple(t.shape)}")
    if batch_apply not in ("inplace", "recompute"):
        raise ValueError(f"stem_forward: batch_apply must be 'inplace' or 'recompute', got {batch_apply!r}")
    n, H, W = (int(v) for v in images.shape[:3])
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"stem_forward: images is empty {tuple(images.shape)}")
    h, w = stem_out_shape(H, W)
    if batch_stats and n * h * w == 1:
        raise ValueError("stem_forward: batch statistics need more than one value per channel (n h w = 1)")
    rows = int(_rawlib.dns_stem_partial_rows(n, H, W))
    if rows == 0:
        raise ValueError(f"stem_forward: images {tuple(images.shape)} are too large for one call")
    if out is None:
        out = torch.empty(n, h, w, 64, device=images.device)
    elif tuple(out.shape) != (n, h, w, 64):
        raise ValueError(f"stem_forward: out must be [{n},{h},{w},64], got {tuple(out.shape)}")
    elif not out.is_contiguous():
        raise ValueError("stem_forward: out must be contiguous")
    wpack, st = _stem_constants(*params, eps)
    images = images.detach()
    sp = stream_ptr()
    if not batch_stats:
        check(lib.dns_stem_forward(ptr(images), n, H, W, ptr(wpack), ptr(st), ptr(out), STEM_STORE | STEM_EPILOGUE, None, sp),
              "dns_stem_forward")
        return out
    ws = torch.empty((rows + 256) * 128, dtype=torch.float64, device=images.device)
    level1 = ws[rows * 128:]
    st_b = torch.empty(2, 64, device=images.device)
    inplace = batch_apply == "inplace"
    check(lib.dns_stem_forward(ptr(images), n, H, W, ptr(wpack), None, ptr(out), STEM_STATS | (STEM_STORE if inplace else 0), ptr(ws),
                               sp), "dns_stem_forward")
    check(lib.dns_stem_batch_stats(ptr(ws), n, H, W, ptr(bn_weight.detach()), ptr(bn_bias.detach()), float(eps), ptr(level1), ptr(st_b),
                                   sp), "dns_stem_batch_stats")
    if inplace:
        check(lib.dns_stem_normalise(ptr(out), n * h * w, ptr(st_b), sp), "dns_stem_normalise")
    else:
        check(lib.dns_stem_forward(ptr(images), n, H, W, ptr(wpack), ptr(st_b), ptr(out), STEM_STORE | STEM_EPILOGUE, None, sp),
              "dns_stem_forward")
    return out


# ----------------------------------------------------------------------------- LPIPS (csrc/lpips.hip, csrc/conv_plan.hpp)
CONV_RELU, CONV_SCALE_INPUT = 1, 2                      # include/dns_hip.h: flags of dns_conv_cl
LPIPS_MIN_SIDE = 31                                     # smaller images leave the second pool empty
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
# AlexNet `features`: (state-dict index, Cin, Cout, kernel, stride, pad, pooled input)
LPIPS_LAYERS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True),
                (8, 384, 256, 3, 1, 1, False), (10, 256, 256, 3, 1, 1, False))
LPIPS_METHODS = ("fused", "torch")
# what ``method=None`` means for device tensors: at one pair of 680 x 1200 the fused kernels are slower than the library's
# convolutions (1.54 against 1.27 ms); "fused" is the choice for fixed bits, batches and no first-call search
LPIPS_DEFAULT = "torch"


def conv_out_extent(size: int, ks: int, stride: int, pad: int) -> int:
    return (int(size) + 2 * int(pad) - int(ks)) // int(stride) + 1


def pool_out_extent(size: int) -> int:
    """max pool 3x3, stride 2, no padding, floor mode"""
    return (int(size) - 3) // 2 + 1


def lpips_feature_shapes(H: int, W: int):
    """[(h, w, C)] of the five LPIPS features of an H x W image."""
    out, h, w = [], int(H), int(W)
    for _, _, cout, ks, stride, pad, pooled in LPIPS_LAYERS:
        if pooled:
            h, w = pool_out_extent(h), pool_out_extent(w)
        h, w = conv_out_extent(h, ks, stride, pad), conv_out_extent(w, ks, stride, pad)
        out.append((h, w, cout))
    return out


def conv_pack(weight: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """The packed weight image of ``dns_conv_cl`` (include/dns_hip.h) for ``weight`` [Cout,Cin,k,k] on the device:
    [Cout/64][chunks][k per chunk, padded to even][64], built by torch ops, no read-back."""
    cout, cin, ks, ks2 = (int(v) for v in weight.shape)
    shape = (C.c_uint32 * 4)()
    check(_rawlib.dns_conv_pack_shape(cin, cout, ks, int(stride), int(pad), shape), "dns_conv_pack_shape")
    cb, chunks, kc_pad, ck = (int(v) for v in shape)
    ncs = cin // ck
    w = weight.detach().float().reshape(cb, 64, ncs, ck, ks, ks).permute(0, 4, 2, 5, 3, 1)       # cb, ky, cs, kx, c, o
    pack = torch.zeros(cb, chunks, kc_pad, 64, device=weight.device)
    pack[:, :, :ks * ck] = w.reshape(cb, ks * ncs, ks * ck, 64)
    return pack.contiguous()


def _conv_arguments(who, x, weight, bias, stride, pad):
    for t in (x, weight) + ((bias,) if bias is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{who}: every tensor must be on the GPU (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: every tensor must be float32, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"{who}: all tensors must be on one device")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"{who}: x must be a contiguous channels-last [n,H,W,Cin] tensor, got {tuple(x.shape)}")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != x.shape[3]:
        raise ValueError(f"{who}: weight must be [Cout,{int(x.shape[3])},k,k], got {tuple(weight.shape)}")
    cout, cin, ks = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    if bias is not None and (tuple(bias.shape) != (cout,) or not bias.is_contiguous()):
        raise ValueError(f"{who}: bias must be a contiguous [{cout}] tensor, got {tuple(bias.shape)}")
    n, H, W = (int(v) for v in x.shape[:3])
    stride, pad = int(stride), int(pad)
    if cout % 64 != 0 or not (1 <= ks <= 11) or not (1 <= stride <= 4) or not (0 <= pad < ks):
        raise ValueError(f"{who}: Cout {cout} must be a multiple of 64, the kernel {ks} at most 11, the stride {stride} at most 4 and "
                         f"the padding {pad} below the kernel size")
    if n < 1 or H + 2 * pad < ks or W + 2 * pad < ks:
        raise ValueError(f"{who}: x {tuple(x.shape)} is empty or smaller than the kernel")
    return n, H, W, cin, cout, ks, stride, pad


def _launch_conv(x, n, H, W, cin, wpack, bias, cout, ks, stride, pad, flags, sp):
    h, w = conv_out_extent(H, ks, stride, pad), conv_out_extent(W, ks, stride, pad)
    out = torch.empty(n, h, w, cout, device=x.device)
    check(lib.dns_conv_cl(ptr(x), n, H, W, cin, ptr(wpack), ptr(bias), cout, ks, stride, pad, flags, ptr(out), sp), "dns_conv_cl")
    return out


def conv_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, pad: int = 0, relu: bool = True, *,
            scale_input: bool = False, wpack: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Channels-last convolution + bias + optional ReLU (keeping a NaN): ``x`` [n,H,W,Cin] fp32, ``weight`` [Cout,Cin,k,k] (Cout a
    multiple of 64, k <= 11, stride <= 4, pad < k) -> [n,h,w,Cout]; exact fp32 products and fp32 accumulation in a fixed order, so
    the bits of an image's map depend on the image and the parameters alone.  ``scale_input``: the LPIPS input scaling
    (include/dns_hip.h) is applied to the 3-channel ``x`` as it is read, the zero padding staying zero.  ``wpack``:
    ``conv_pack(weight, stride, pad)`` where the caller keeps it.  ValueError for CPU tensors and refused shapes, before any launch."""
    n, H, W, cin, cout, ks, stride, pad = _conv_arguments("conv_cl", x, weight, bias, stride, pad)
    if scale_input and cin != 3:
        raise ValueError(f"conv_cl: scale_input is the scaling of a 3-channel image, x has {cin} channels")
    if wpack is None:
        wpack = conv_pack(weight, stride, pad)
    flags = (CONV_RELU if relu else 0) | (CONV_SCALE_INPUT if scale_input else 0)
    return _launch_conv(x.detach(), n, H, W, cin, wpack, None if bias is None else bias.detach(), cout, ks, stride, pad, flags,
                        stream_ptr())


def _launch_pool(x, sp):
    n, h, w, c = (int(v) for v in x.shape)
    out = torch.empty(n, pool_out_extent(h), pool_out_extent(w), c, device=x.device)
    check(lib.dns_max_pool_cl(ptr(x), n, h, w, c, ptr(out), sp), "dns_max_pool_cl")
    return out


def max_pool_cl(x: torch.Tensor) -> torch.Tensor:
    """Max pool 3x3, stride 2, no padding, floor mode, of channels-last ``x`` [n,h,w,C] fp32 (C a multiple of 4, sides >= 3) ->
    [n,(h-3)//2+1,(w-3)//2+1,C]; a NaN in a window wins, as in F.max_pool2d."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("max_pool_cl: x must be on the GPU (there is no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"max_pool_cl: x must be a contiguous float32 [n,h,w,C] tensor, got {x.dtype} {tuple(x.shape)}")
    n, h, w, c = (int(v) for v in x.shape)
    if n < 1 or h < 3 or w < 3 or c < 4 or c % 4 != 0:
        raise ValueError(f"max_pool_cl: x {tuple(x.shape)}: sides must be at least 3 and C a multiple of 4")
    return _launch_pool(x.detach(), stream_ptr())


def _launch_head(fa, fb, lin, F, h, w, c, sp):
    part = torch.empty(F, int(_rawlib.dns_lpips_head_blocks(h, w)), dtype=torch.float64, device=fa.device)
    check(lib.dns_lpips_head(ptr(fa), ptr(fb), ptr(lin), F, h, w, c, ptr(part), sp), "dns_lpips_head")
    return part


def _launch_finish(parts, hs, ws, F, sp):
    L = len(parts)
    lp = torch.empty(F, dtype=torch.float64, device=parts[0].device)
    layers = torch.empty(F, L, dtype=torch.float64, device=parts[0].device)
    pa = (C.c_void_p * L)(*[int(p.data_ptr()) for p in parts])
    check(lib.dns_lpips_finish(pa, (C.c_uint32 * L)(*hs), (C.c_uint32 * L)(*ws), L, F, ptr(lp), ptr(layers), sp), "dns_lpips_finish")
    return lp, layers


def lpips_head(feat_pred: torch.Tensor, feat_gt: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """One layer of the LPIPS head: features [F,h,w,C] fp32 channels-last of the two images (C a multiple of 64, at most 512) and
    ``lin`` [C] -> d [F] float64 on the device: the mean over pixels of sum_c lin_c (n(f_pred)_c - n(f_gt)_c)^2,
    n(f) = f / (|f| + 1e-10), in float64 from the fp32 features, every sum in a fixed order."""
    for t in (feat_pred, feat_gt, lin):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("lpips_head: every tensor must be on the GPU (there is no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("lpips_head: every tensor must be contiguous float32")
    if feat_pred.dim() != 4 or feat_pred.shape != feat_gt.shape:
        raise ValueError(f"lpips_head: features must be two [F,h,w,C] tensors, got {tuple(feat_pred.shape)} and {tuple(feat_gt.shape)}")
    F, h, w, c = (int(v) for v in feat_pred.shape)
    if F < 1 or F > 65535 or h < 1 or w < 1 or c % 64 != 0 or not (64 <= c <= 512) or tuple(lin.shape) != (c,):
        raise ValueError(f"lpips_head: features {tuple(feat_pred.shape)}, lin {tuple(lin.shape)}: C must be a multiple of 64 up to 512 "
                         f"and lin [C]")
    sp = stream_ptr()
    part = _launch_head(feat_pred.detach(), feat_gt.detach(), lin.detach(), F, h, w, c, sp)
    return _launch_finish([part], [h], [w], F, sp)[1][:, 0]


class LpipsWeights:
    """The parameters of LPIPS (AlexNet): ``convs`` = five (weight [Cout,Cin,k,k], bias [Cout]) pairs, ``lins`` = five [C] vectors,
    fp32.  ``on(device)`` returns (and keeps) the copies on a device together with the packed weight images of the fused path, made
    once per device."""

    def __init__(self, convs, lins):
        convs = [(torch.as_tensor(w).detach().float().contiguous(), torch.as_tensor(b).detach().float().contiguous()) for w, b in convs]
        lins = [torch.as_tensor(l).detach().float().reshape(-1).contiguous() for l in lins]
        if len(convs) != 5 or len(lins) != 5:
            raise ValueError(f"LpipsWeights: five convolutions and five lin vectors, got {len(convs)} and {len(lins)}")
        for l, ((w, b), lin, (_, cin, cout, ks, _, _, _)) in enumerate(zip(convs, lins, LPIPS_LAYERS)):
            if tuple(w.shape) != (cout, cin, ks, ks) or tuple(b.shape) != (cout,) or tuple(lin.shape) != (cout,):
                raise ValueError(f"LpipsWeights: layer {l}: weight {tuple(w.shape)}, bias {tuple(b.shape)}, lin {tuple(lin.shape)} are "
                                 f"not [{cout},{cin},{ks},{ks}], [{cout}], [{cout}]")
        self.convs, self.lins = convs, lins
        self._on = {}

    def on(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._on.get(device)
        if hit is None:
            convs = [(w.to(device), b.to(device)) for w, b in self.convs]
            lins = [l.to(device) for l in self.lins]
            packs = None
            if device.type == "cuda":
                packs = [conv_pack(w, stride, pad) for (w, _), (_, _, _, _, stride, pad, _) in zip(convs, LPIPS_LAYERS)]
            hit = self._on[device] = (convs, lins, packs)
        return hit


def _lpips_arguments(pred, gt, weights):
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError("lpips: pred and gt must be tensors")
    if pred.shape != gt.shape:
        raise ValueError(f"lpips: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3:
        raise ValueError(f"lpips: images must be [H,W,3] or [F,H,W,3], got {tuple(pred.shape)}")
    if pred.device != gt.device:
        raise ValueError("lpips: pred and gt must be on one device")
    if not isinstance(weights, LpipsWeights):
        raise ValueError("lpips: weights must be an LpipsWeights (evaluation.load_lpips_weights)")
    F, H, W = (1,) + tuple(pred.shape[:2]) if pred.dim() == 3 else tuple(pred.shape[:3])
    if min(H, W) < LPIPS_MIN_SIDE:
        raise ValueError(f"lpips: images of {H} x {W}: both sides must be at least {LPIPS_MIN_SIDE} (the second 3x3 pool would be empty)")
    if F == 0 or 2 * F > 65535:
        raise ValueError(f"lpips: {F} pairs (1..32767)")
    p = pred.detach().float().contiguous().view(F, H, W, 3)
    g = gt.detach().float().contiguous().view(F, H, W, 3)
    return p, g, int(F), int(H), int(W)


def _lpips_torch(p, g, weights, channels_last=False):
    """The definition of include/dns_hip.h out of torch ops in fp32 (F.conv2d, F.max_pool2d), as the lpips package evaluates it.
    ``channels_last``: the library's other memory format (tools/time_lpips.py times both).  The library's convolutions are free to
    round an image differently at another batch position or in another call, so identical images need not give exactly 0 here."""
    import torch.nn.functional as Fn
    convs, lins, _ = weights.on(p.device)
    shift = torch.tensor(LPIPS_SHIFT, device=p.device).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, device=p.device).view(1, 3, 1, 1)
    F = p.shape[0]
    x = torch.cat((p, g)).permute(0, 3, 1, 2)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x = torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))       # a NaN stays
    x = (2.0 * x - 1.0 - shift) / scale
    ds = []
    for (w, b), lin, (_, _, _, _, stride, pad, pooled) in zip(convs, lins, LPIPS_LAYERS):
        if pooled:
            x = Fn.max_pool2d(x, 3, 2)
        x = torch.relu(Fn.conv2d(x, w, b, stride=stride, padding=pad))                           # torch's relu keeps a NaN
        n = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
        ds.append(((n[:F] - n[F:]) ** 2 * lin.view(1, -1, 1, 1)).sum(1).flatten(1).mean(1))
    layers = torch.stack(ds, 1).double()
    return layers.sum(1), layers


def lpips_launch(pred: torch.Tensor, gt: torch.Tensor, weights: LpipsWeights, method: Optional[str] = None):
    """``lpips`` without a host read: -> (lpips [F] float64, layers [F,5] float64) on the tensors' device; F = 1 for [H,W,3] images."""
    if method is not None and method not in LPIPS_METHODS:
        raise ValueError(f"lpips: method must be None, 'fused' or 'torch', got {method!r}")
    p, g, F, H, W = _lpips_arguments(pred, gt, weights)
    if method is None:
        method = LPIPS_DEFAULT if p.is_cuda else "torch"
    if method == "torch":
        return _lpips_torch(p, g, weights)
    require_cuda(p, g)
    convs, lins, packs = weights.on(p.device)
    sp = stream_ptr()
    x = torch.cat((p, g))                                 # pred and gt as one batch of 2F images: twice the tiles per launch
    n, h, w = 2 * F, H, W
    parts, hs, ws = [], [], []
    for l, ((wt, b), lin, pack, (_, cin, cout, ks, stride, pad, pooled)) in enumerate(zip(convs, lins, packs, LPIPS_LAYERS)):
        if pooled:
            x = _launch_pool(x, sp)
            h, w = pool_out_extent(h), pool_out_extent(w)
        x = _launch_conv(x, n, h, w, cin, pack, b, cout, ks, stride, pad, CONV_RELU | (CONV_SCALE_INPUT if l == 0 else 0), sp)
        h, w = int(x.shape[1]), int(x.shape[2])
        parts.append(_launch_head(x[:F], x[F:], lin, F, h, w, cout, sp))
        hs.append(h), ws.append(w)
    return _launch_finish(parts, hs, ws, F, sp)


def lpips(pred: torch.Tensor, gt: torch.Tensor, weights: LpipsWeights, method: Optional[str] = None):
    """LPIPS (AlexNet; the definition of include/dns_hip.h: lpips 0.1.4 as torchmetrics 0.11.1 calls it with ``normalize=True``, what
    eval_2d.py:304 evaluates) of image pairs pred, gt [H,W,3] or [F,H,W,3] fp32 in [0,1], in the project's image layout ->
    {"lpips": float64 [F] (0-d for one image), "layers": float64 [F,5] ([5])} on the tensors' device.  ``method="fused"``: the HIP
    kernels (convolutions in exact fp32 in a fixed order, head in float64; the same bits for every call and every batch);
    ``method="torch"``: the same definition composed of F.conv2d / F.max_pool2d in fp32, which also runs on CPU tensors (on the
    device its bits are the library's: identical images need not give exactly 0, and its first call searches for algorithms for
    seconds); None: ``LPIPS_DEFAULT`` for device tensors ("torch": faster at one frame-size pair, "fused" is faster from a few pairs
    on), "torch" for CPU tensors.  Sides below 31, mismatched shapes, a last dimension other
    than 3 and, for "fused", CPU tensors raise ValueError before anything is launched.

    The weights come from the caller (``evaluation.load_lpips_weights``); the arithmetic is held to a float64 restatement of the
    published definition (tests/lpips_ref.py), not to values written by the lpips package, which is not available here."""
    single = isinstance(pred, torch.Tensor) and pred.dim() == 3
    val, layers = lpips_launch(pred, gt, weights, method)
    if single:
        val, layers = val[0], layers[0]
    return {"lpips": val, "layers": layers}


# ----------------------------------------------------------------------------- frame preparation (csrc/frame_prep.hip, csrc/frame_prep_plan.hpp)
PREPARE_FRAMES_METHODS = ("kernel", "torch")
PREPARE_FRAMES_DEFAULT = "kernel"
LABEL_VALUES = 65536                         # entries of a label look-up table and of label_first_seen's result


class FramePrepTables:
    """The resampling tables of ``prepare_frames`` for one set of image sizes (include/dns_hip.h, "frame preparation"): built on the
    host by the library (``dns_frame_prep_tables``), copied to ``device`` once.  ``words``: the host blob (int32 numpy);
    ``dev``: its copy on the device; ``H``, ``W``: the size of a prepared frame."""

    def __init__(self, color_hw, depth_hw, label_hw=None, crop_size=None, crop_edge=0, device="cuda"):
        from ._lib import DnsFramePrepDims
        pair = lambda v, what: self._pair(v, what)
        self.color_hw, self.depth_hw = pair(color_hw, "color_hw"), pair(depth_hw, "depth_hw")
        self.label_hw = None if label_hw is None else pair(label_hw, "label_hw")
        self.crop_size = None if crop_size is None else pair(crop_size, "crop_size")
        self.edge = int(crop_edge)
        if self.edge < 0:
            raise ValueError(f"frame_prep_tables: crop_edge {crop_edge}")
        self.stage_hw = self.crop_size or self.depth_hw
        lh, lw = self.label_hw or (0, 0)
        self.dims = DnsFramePrepDims(*self.color_hw, *self.depth_hw, lh, lw, *self.stage_hw, self.edge)
        n = int(_rawlib.dns_frame_prep_table_words(C.byref(self.dims)))
        if n == 0:
            raise ValueError(f"frame_prep_tables: sizes refused: colour {self.color_hw}, depth {self.depth_hw}, labels {self.label_hw}, "
                             f"crop_size {self.crop_size}, crop_edge {self.edge} (sides 1..32768, 2 crop_edge below both output sides)")
        self.words = np.empty(n, dtype=np.int32)
        check(_rawlib.dns_frame_prep_tables(C.byref(self.dims), self.words.ctypes.data_as(C.c_void_p), n), "dns_frame_prep_tables")
        self.H, self.W = self.stage_hw[0] - 2 * self.edge, self.stage_hw[1] - 2 * self.edge
        self.dev = torch.from_numpy(self.words).to(torch.device(device))
        self.device = self.dev.device
        self._parts = {}

    @staticmethod
    def _pair(v, what):
        try:
            h, w = (int(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"frame_prep_tables: {what} must be (H, W), got {v!r}") from None
        if h < 1 or w < 1:
            raise ValueError(f"frame_prep_tables: {what} {v!r}")
        return h, w

    def parts(self, device=None):
        """The tables by name, as views of the blob on ``device`` (default: the tables' own): ``cv_x`` / ``cv_y`` / ``tb_x`` /
        ``tb_y`` = (index int64, weights fp32 [.,2]) of the cv2 and torch linear stages, ``tn_x`` / ``tn_y`` / ``cn_x`` / ``cn_y`` =
        the index of the torch and cv2 nearest stages (csrc/frame_prep_plan.hpp states the layout)."""
        device = self.device if device is None else torch.device(device)
        if device in self._parts:
            return self._parts[device]
        blob = self.dev if device == self.device else torch.from_numpy(self.words).to(device)
        (_, _), (Hd, Wd), (Hs, Ws) = self.color_hw, self.depth_hw, self.stage_hw
        out, o = {}, 0
        for name, n in (("cv_x", Wd), ("cv_y", Hd), ("tb_x", Ws), ("tb_y", Hs)):
            out[name] = (blob[o:o + n].long(), blob[o + n:o + 3 * n].view(torch.float32).reshape(n, 2))
            o += 3 * n
        for name, n in (("tn_x", Ws), ("tn_y", Hs), ("cn_x", Wd), ("cn_y", Hd)):
            out[name] = blob[o:o + n].long()
            o += n
        assert o == blob.numel()
        self._parts[device] = out
        return out


def frame_prep_tables(color_hw, depth_hw, label_hw=None, crop_size=None, crop_edge=0, device="cuda") -> FramePrepTables:
    """Tables for colour images of ``color_hw``, depth images of ``depth_hw``, label images of ``label_hw`` (None: no labels),
    ``cfg['cam']['crop_size']`` (None: not set) and ``cfg['cam']['crop_edge']``."""
    return FramePrepTables(color_hw, depth_hw, label_hw, crop_size, crop_edge, device)


def _frame_prep_args(color, depth, label, lut, tables, method):
    """Argument checks of prepare_frames, ahead of any launch -> (color, depth, label, n, single, method)."""
    if not isinstance(tables, FramePrepTables):
        raise ValueError("prepare_frames: tables must come from ops.frame_prep_tables")
    if not isinstance(color, torch.Tensor) or not isinstance(depth, torch.Tensor):
        raise ValueError("prepare_frames: color and depth must be tensors")
    if method is None:
        method = PREPARE_FRAMES_DEFAULT if color.is_cuda else "torch"
    if method not in PREPARE_FRAMES_METHODS:
        raise ValueError(f"prepare_frames: method {method!r} (one of {PREPARE_FRAMES_METHODS})")
    if color.dtype != torch.uint8 or color.dim() not in (3, 4) or color.shape[-1] != 3:
        raise ValueError(f"prepare_frames: color must be uint8 [n,Hc,Wc,3] or [Hc,Wc,3], got {color.dtype} {tuple(color.shape)}")
    single = color.dim() == 3
    if depth.dtype != torch.uint16 or depth.dim() != color.dim() - 1:
        raise ValueError(f"prepare_frames: depth must be uint16 [n,Hd,Wd] ([Hd,Wd] for one frame), got {depth.dtype} {tuple(depth.shape)}")
    if label is not None:
        if not isinstance(label, torch.Tensor) or label.dtype not in (torch.uint8, torch.uint16) or label.dim() != depth.dim():
            raise ValueError("prepare_frames: label must be a uint8 or uint16 tensor [n,Hl,Wl] ([Hl,Wl] for one frame) or None")
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.int32 or tuple(lut.shape) != (LABEL_VALUES,):
            raise ValueError(f"prepare_frames: lut must be an int32 [{LABEL_VALUES}] tensor")
    if single:
        color, depth, label = color[None], depth[None], None if label is None else label[None]
    n = int(color.shape[0])
    if tuple(color.shape[1:3]) != tables.color_hw or tuple(depth.shape) != (n,) + tables.depth_hw:
        raise ValueError(f"prepare_frames: colour {tuple(color.shape)} / depth {tuple(depth.shape)} for tables of colour "
                         f"{tables.color_hw} and depth {tables.depth_hw}, n = {n}")
    if (label is None) != (tables.label_hw is None) or (label is not None and tuple(label.shape) != (n,) + tables.label_hw):
        raise ValueError(f"prepare_frames: label {None if label is None else tuple(label.shape)} for tables of labels {tables.label_hw}, n = {n}")
    if n > 65535:
        raise ValueError(f"prepare_frames: {n} frames (must be <= 65535)")
    ts = [color, depth] + ([label, lut] if label is not None else [])
    if any(t.device != color.device for t in ts):
        raise ValueError("prepare_frames: color, depth, label and lut must live on one device")
    if any(not t.is_contiguous() for t in ts):
        raise ValueError("prepare_frames: color, depth, label and lut must be contiguous")
    if method == "kernel":
        require_cuda(*ts)
        if tables.dev.device != color.device:
            raise ValueError(f"prepare_frames: the tables live on {tables.dev.device}, the images on {color.device}")
    return color, depth, label, n, single, method


def _prepare_frames_torch(color, depth, label, lut, tables, png_depth_scale, scale, bgr):
    """The stages of include/dns_hip.h composed of torch ops on whole images (fp32 products and sums; their fusion is the library's)."""
    t = tables.parts(color.device)
    e, (Hs, Ws) = tables.edge, tables.stage_hw
    # the two fp32 divisions, correctly rounded: torch turns a division by a Python scalar into a product with its reciprocal on the
    # device, and the device's fp32 quotient need not be the IEEE one.  A float64 quotient of two fp32 numbers rounded to fp32 is (53
    # >= 2 24 + 2 bits: the second rounding cannot change the result), and a tensor divisor keeps the division a division.
    div = lambda x, by: (x.to(torch.float64) / torch.full((1,), float(np.float32(by)), dtype=torch.float64, device=x.device)).to(torch.float32)
    c = div(color, 255.0)
    if bgr:
        c = c.flip(-1)

    def linear(img, ix, wx, iy, wy, src_h, src_w):
        x1, y1 = (ix + 1).clamp(max=src_w - 1), (iy + 1).clamp(max=src_h - 1)
        h = img[:, :, ix] * wx[:, 0, None] + img[:, :, x1] * wx[:, 1, None]
        return h[:, iy] * wy[:, 0, None, None] + h[:, y1] * wy[:, 1, None, None]

    if tables.color_hw != tables.depth_hw:
        c = linear(c, *t["cv_x"], *t["cv_y"], *tables.color_hw)
    if tables.stage_hw != tables.depth_hw:
        c = linear(c, *t["tb_x"], *t["tb_y"], *tables.depth_hw)
    d = div(depth, png_depth_scale) * float(np.float32(scale))
    d = d[:, t["tn_y"]][:, :, t["tn_x"]]
    crop = lambda img: img[:, e:Hs - e, e:Ws - e].contiguous()
    lab = None
    if label is not None:
        lab = label.to(torch.int64)[:, t["cn_y"]][:, :, t["cn_x"]]
        lab = lut.to(torch.int64)[lab][:, t["tn_y"]][:, :, t["tn_x"]]
        lab = crop(lab)
    return crop(c), crop(d), lab


def prepare_frames(color: torch.Tensor, depth: torch.Tensor, label: Optional[torch.Tensor], lut: Optional[torch.Tensor],
                   tables: FramePrepTables, png_depth_scale: float, scale: float = 1.0, bgr: bool = False, method: Optional[str] = None):
    """``BaseDataset.__getitem__`` (datas/slam_datasets.py:85-149) on the raw images of n frames: color uint8 [n,Hc,Wc,3] (``bgr``:
    channel order B, G, R, as cv2.imread returns), depth uint16 [n,Hd,Wd], label uint8 / uint16 [n,Hl,Wl] or None, lut int32 [65536]
    (the class of every raw label value; None without labels) -> (color fp32 [n,H,W,3] in RGB, depth fp32 [n,H,W], label int64
    [n,H,W] or None).  Inputs without the frame dimension give outputs without it.  The stages, their order and their rounding are
    the ones include/dns_hip.h states.

    ``method="kernel"``: one launch (csrc/frame_prep.hip); a frame's bits depend on nothing but the frame.  ``method="torch"``: the
    same definition composed of torch ops over whole images, which also runs on CPU tensors; depth and label are the kernel's, its
    colour may differ in the last bits where the library fuses a product with a sum.  None: ``PREPARE_FRAMES_DEFAULT`` for device
    tensors, "torch" for CPU tensors.  Wrong dtypes, shapes that do not match the tables, non-contiguous tensors, mixed devices
    and, for "kernel", CPU tensors raise ValueError before anything is launched."""
    color, depth, label, n, single, method = _frame_prep_args(color, depth, label, lut, tables, method)
    pds, sc = float(png_depth_scale), float(scale)
    if not (math.isfinite(pds) and pds != 0.0 and float(np.float32(pds)) != 0.0 and math.isfinite(sc)):
        raise ValueError(f"prepare_frames: png_depth_scale {png_depth_scale}, scale {scale}")
    if method == "torch":
        oc, od, ol = _prepare_frames_torch(color, depth, label, lut, tables, pds, sc, bool(bgr))
    else:
        dev = color.device
        oc = torch.empty(n, tables.H, tables.W, 3, dtype=torch.float32, device=dev)
        od = torch.empty(n, tables.H, tables.W, dtype=torch.float32, device=dev)
        ol = None if label is None else torch.empty(n, tables.H, tables.W, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            check(lib.dns_prepare_frames(ptr(color), int(bool(bgr)), ptr(depth), ptr(label), 0 if label is None else label.element_size(),
                                         ptr(lut) if label is not None else None, C.byref(tables.dims), ptr(tables.dev),
                                         tables.dev.numel(), n, pds, sc, ptr(oc), ptr(od), ptr(ol), stream_ptr()), "dns_prepare_frames")
    if single:
        oc, od, ol = oc[0], od[0], None if ol is None else ol[0]
    return oc, od, ol


def label_first_seen(labels: torch.Tensor, method: Optional[str] = None) -> torch.Tensor:
    """labels uint8 / uint16 of any shape (frames concatenated, row-major) -> int32 [65536]: for every value the smallest flat index
    at which it occurs, -1 for a value that does not occur.  ``cal_class_n``'s ``set(label_data.flatten())`` iterates in an order
    that depends on the first occurrences of the distinct values alone, so this is all of a label image the class numbering needs.
    ``method="kernel"``: an integer atomic minimum on the device (the same for every call); ``"torch"``: a scatter-reduce, also on
    CPU tensors; None: "kernel" for device tensors, "torch" for CPU tensors."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("label_first_seen: labels must be a uint8 or uint16 tensor")
    if method is None:
        method = "kernel" if labels.is_cuda else "torch"
    if method not in PREPARE_FRAMES_METHODS:
        raise ValueError(f"label_first_seen: method {method!r} (one of {PREPARE_FRAMES_METHODS})")
    if not labels.is_contiguous():
        raise ValueError("label_first_seen: labels must be contiguous")
    n = labels.numel()
    if n >= 1 << 31:
        raise ValueError(f"label_first_seen: {n} pixels (must be < 2^31)")
    if method == "torch":
        big = torch.full((LABEL_VALUES,), 1 << 31, dtype=torch.int64, device=labels.device)
        big.scatter_reduce_(0, labels.reshape(-1).to(torch.int64), torch.arange(n, device=labels.device), "amin")
        return torch.where(big == 1 << 31, torch.full_like(big, -1), big).to(torch.int32)
    require_cuda(labels)
    first = torch.empty(LABEL_VALUES, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        check(lib.dns_label_first_seen(ptr(labels), labels.element_size(), n, ptr(first), stream_ptr()), "dns_label_first_seen")
    return first


# ---------------------------------------------------------------------------------------------------------------------------------
# keyframe overlap and frame_vis's sheet (csrc/keyframes.hip, csrc/vis_panels.hip; include/dns_hip.h, ABI v29)
def keyframe_overlap(points: torch.Tensor, c2w: torch.Tensor, H: int, W: int, fx: float, fy: float, cx: float, cy: float,
                     edge: int = 10, eps: float = 1e-5) -> torch.Tensor:
    """The projection block of ``keyframe_selection_overlap`` (slams/mapping.py:208-226) for all keyframes in one launch and without
    a host read: points fp32 [P,3], c2w fp32 [n,4,4] (camera-to-world) -> int32 [n], per keyframe the number of points that project
    more than ``edge`` pixels inside the H x W image with z < 0.  The arithmetic is float64, one rounding per operation, in the order
    include/dns_hip.h states; tests/keyframe_overlap_ref.py restates it in numpy and the counts are equal to it.  A point or pose
    with a non-finite entry, and a singular pose, count nothing.  ``P == 0`` gives zeros and ``n == 0`` an empty tensor, without a
    launch."""
    require_cuda(points, c2w)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"keyframe_overlap: points must be fp32 [P,3], got {points.dtype} {tuple(points.shape)}")
    if c2w.dtype != torch.float32 or c2w.dim() != 3 or tuple(c2w.shape[1:]) != (4, 4):
        raise ValueError(f"keyframe_overlap: c2w must be fp32 [n,4,4], got {c2w.dtype} {tuple(c2w.shape)}")
    if points.device != c2w.device:
        raise ValueError("keyframe_overlap: points and c2w are on different devices")
    P, n = points.shape[0], c2w.shape[0]
    if P == 0 or n == 0:
        return torch.zeros(n, dtype=torch.int32, device=points.device)
    out = torch.empty(n, dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        check(lib.dns_keyframe_overlap(ptr(points), P, ptr(c2w), n, int(H), int(W), float(fx), float(fy), float(cx), float(cy),
                                       int(edge), float(eps), ptr(out), stream_ptr()), "dns_keyframe_overlap")
    return out


def vis_panels(gt_color: torch.Tensor, est_color: torch.Tensor, gt_depth: torch.Tensor, est_depth: torch.Tensor,
               gt_label: torch.Tensor, est_label: torch.Tensor, label_lut: Optional[torch.Tensor] = None, max_label: float = 101,
               gap: int = 8, background: int = 255):
    """``fig_plot``'s 3 x 3 sheet (utils/common.py:682-745) on the device: rows depth, colour, label; columns input, generated,
    |difference|; panels at native resolution, ``gap`` pixels of ``background`` between them -> (uint8 [3H + 2 gap, 3W + 2 gap, 3],
    vmax), vmax a 0-dim fp32 device tensor: the largest finite positive ``gt_depth`` (0 without one), which scales the depth row.
    Colours fp32 [H,W,3], depths fp32 [H,W]; labels [H,W] of any integer or float dtype (taken as int32), mapped through
    ``label_lut`` (int32 [n]: the class -> label table; entries outside it stay as they are) and scaled by ``max_label``.  The byte
    rules are include/dns_hip.h's: scalar panels are matplotlib's ``plasma(Normalize(0, vmax)(x), bytes=True)``, a non-finite scalar
    pixel takes the background colour (matplotlib leaves it transparent).  Titles, axes and the JPEG are not rebuilt.  No host read."""
    require_cuda(gt_color, est_color, gt_depth, est_depth, gt_label, est_label, label_lut)
    if gt_depth.dim() != 2:
        raise ValueError(f"vis_panels: gt_depth must be [H,W], got {tuple(gt_depth.shape)}")
    H, W = gt_depth.shape
    if H < 1 or W < 1:
        raise ValueError("vis_panels: an empty image")
    for name, t, shape in (("gt_color", gt_color, (H, W, 3)), ("est_color", est_color, (H, W, 3)), ("gt_depth", gt_depth, (H, W)),
                           ("est_depth", est_depth, (H, W))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"vis_panels: {name} must be fp32 {shape}, got {t.dtype} {tuple(t.shape)}")
    labels = []
    for name, t in (("gt_label", gt_label), ("est_label", est_label)):
        if tuple(t.shape) != (H, W):
            raise ValueError(f"vis_panels: {name} must be [{H},{W}], got {tuple(t.shape)}")
        labels.append(t if t.dtype == torch.int32 else t.to(torch.int32))
    if label_lut is not None and (label_lut.dtype != torch.int32 or label_lut.dim() != 1 or label_lut.numel() == 0):
        raise ValueError("vis_panels: label_lut must be a non-empty int32 vector")
    dev = gt_depth.device
    if any(t is not None and t.device != dev for t in (gt_color, est_color, est_depth, gt_label, est_label, label_lut)):
        raise ValueError("vis_panels: tensors on different devices")
    gap, background = int(gap), int(background)
    if not (0 <= gap <= 4096 and 0 <= background <= 255):
        raise ValueError(f"vis_panels: gap {gap} (0..4096), background {background} (0..255)")
    out = torch.empty(3 * H + 2 * gap, 3 * W + 2 * gap, 3, dtype=torch.uint8, device=dev)
    vmax = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dns_vis_panels(ptr(gt_color), ptr(est_color), ptr(gt_depth), ptr(est_depth), ptr(labels[0]), ptr(labels[1]),
                                 ptr(label_lut), 0 if label_lut is None else label_lut.numel(), H, W, float(max_label), gap, background,
                                 ptr(out), ptr(vmax), stream_ptr()), "dns_vis_panels")
    return out, vmax
