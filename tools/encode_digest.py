"""SHA-256 of what the point-encoding kernels and the fused tracker write, one line per output tensor, for comparing two trees.

Everything that evaluates the encoding's arithmetic (csrc/dev_encode.hpp: cell and fraction, corner weights, level gather and
Jacobian, OneBlob forward and backward) is run on seeded inputs through what every tree has -- the C ABI behind ``ops.lib``,
``TrackStep.run_fused`` and ``dns_slam_amd.synthetic`` -- and every output is printed as ``<phases> <case> <tensor> <sha256>``.
Each case runs twice in the process; an output whose two digests differ (sums of float atomics: the table gradient) is printed
as ``unstable`` and says nothing.  Two trees that compute the same bits print the same text: run it on both and ``diff``.
The tiled encoder's phase split is read from DNS_ENC_PHASES once per process: run the tool a second time with
``DNS_ENC_PHASES=1,1`` for the other setting the host can pick (the first column of every line names the setting).

    python tools/encode_digest.py [--out FILE] [--only SUBSTRING]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dns_slam_amd import ops  # noqa: E402
from dns_slam_amd._lib import check, ptr, stream_ptr  # noqa: E402

DEV = "cuda"
GRIDS = ((16, 592), (12, 64))          # dense + hashed levels; dense levels that wrap through % size
BOUND = ((-1.5, 2.0), (-0.5, 1.75), (0.25, 4.0))
SPLIT_HI_ONLY, SPLIT_PLAIN = 1, 2      # include/dns_hip.h DNS_SPLIT_*


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def points(P, n_bins, seed):
    """Normalised coordinates: uniform in [-0.2, 1.2); rows [0, 64) exactly on bin edges, rows [64, 96) with |x| in [4, 5]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, 3, generator=g) * 1.4 - 0.2
    if P >= 96:
        x[:64] = (torch.randint(-n_bins, 2 * n_bins, (64, 3), generator=g).float() / n_bins)
        far = 4.0 + torch.rand(32, 3, generator=g)
        x[64:96] = torch.where(torch.rand(32, 3, generator=g) < 0.5, -far, far)
    return x


def world(x):
    """Points whose fp64 normalisation by BOUND lands on (about) x: the forward cases with a bound encode these and digest the
    kernel's own x_out; the backward cases are given the normalised x itself, with BOUND only as the scale of d_x."""
    b = torch.tensor(BOUND, dtype=torch.float64)
    return (b[:, 0] + x.double() * (b[:, 1] - b[:, 0])).float()


def off(t, n_floats):
    return C.c_void_p(t.data_ptr() + 4 * n_floats)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device=DEV, dtype=dtype)


# ---- cases: every function returns {tensor name: tensor}
def fwd(form, x, table, meta, n_bins, bound, dydx):
    P, pe, gd = x.shape[0], 3 * n_bins, meta.out_dim
    b6 = ops._bound6(torch.tensor(BOUND, dtype=torch.float64)) if bound else None
    src = (world(x) if bound else x).to(DEV).contiguous()
    out = {"x": z(P, 3)} if bound else {}
    jac = z(meta.n_levels * 3 * P * 2) if dydx else None
    tp, mp = ptr(table), C.byref(meta.c)
    if form == "tiled":                                    # OneBlob | grid in one buffer
        o = out["rows"] = z(P, pe + gd)
        args = (tp, mp, ptr(out.get("x")), ptr(o), pe + gd, off(o, pe), pe + gd)
    elif form == "grid":
        o = out["grid"] = z(P, gd)
        args = (tp, mp, ptr(out.get("x")), None, 0, ptr(o), gd)
    elif form == "pe_wide":                                # OneBlob alone into rows wider than 3 n_bins
        o = out["rows"] = z(P, pe + 21)
        args = (None, None, ptr(out.get("x")), ptr(o), pe + 21, None, 0)
    else:                                                  # separate buffers: the untiled form
        a, b = out["pe"], out["grid"] = z(P, pe), z(P, gd)
        args = (tp, mp, ptr(out.get("x")), ptr(a), pe, ptr(b), gd)
    if dydx:
        out["dydx"] = jac
    check(ops.lib.dns_encode_fwd(ptr(src), b6, P, n_bins, *args, ptr(jac), stream_ptr()), "dns_encode_fwd")
    return out


def fwd_split(form, x, table, meta, n_bins, bound, dydx):
    P, K = x.shape[0], 3 * n_bins + meta.out_dim
    b6 = ops._bound6(torch.tensor(BOUND, dtype=torch.float64)) if bound else None
    src = (world(x) if bound else x).to(DEV).contiguous()
    flags = {"hilo_f32": 0, "hi": SPLIT_HI_ONLY, "plain_f32": SPLIT_PLAIN, "plain": SPLIT_PLAIN}[form]
    out = {"x": z(P, 3), "xs": z(P, 2 * K, dtype=torch.float16), "xexp": z(P, dtype=torch.int32)}
    if form.endswith("f32"):
        out["f32"] = z(P, K)
    if dydx:
        out["dydx"] = z(meta.n_levels * 3 * P * 2)
    check(ops.lib.dns_encode_fwd_split(ptr(src), b6, P, n_bins, ptr(table), C.byref(meta.c), ptr(out["x"]), ptr(out.get("f32")), K,
                                       ptr(out["xs"]), 2 * K, ptr(out["xexp"]), flags, ptr(out.get("dydx")), stream_ptr()),
          "dns_encode_fwd_split")
    return out


def indices(x, meta):
    rows = z(x.shape[0], meta.n_levels, 8, dtype=torch.int32)
    check(ops.lib.dns_hashgrid_indices(ptr(x.to(DEV).contiguous()), x.shape[0], C.byref(meta.c), ptr(rows), stream_ptr()),
          "dns_hashgrid_indices")
    return {"rows": rows}


def bwd(form, x, table, meta, n_bins, bound, seed, scatter=None):
    """d_x (forms jacobian / regather / pe_wide / untiled) or d_table (form table, scatter = (flags, queue cap))."""
    P, pe, gd = x.shape[0], 3 * n_bins, meta.out_dim
    b6 = ops._bound6(torch.tensor(BOUND, dtype=torch.float64)) if bound else None
    xd = x.to(DEV).contiguous()
    g = torch.Generator().manual_seed(seed)
    tp, mp = ptr(table), C.byref(meta.c)
    jac = None
    if form == "jacobian":
        jac = fwd("tiled", x, table, meta, n_bins, False, True)["dydx"]
    if form == "pe_wide":
        gy = torch.randn(P, pe + 21, generator=g).to(DEV)
        grads = (None, None, ptr(gy), pe + 21, None, 0)
    elif form == "untiled":
        ga, gb = torch.randn(P, pe, generator=g).to(DEV), torch.randn(P, gd, generator=g).to(DEV)
        grads = (tp, mp, ptr(ga), pe, ptr(gb), gd)
    else:
        gy = torch.randn(P, pe + gd, generator=g).to(DEV)
        grads = (tp, mp, ptr(gy), pe + gd, off(gy, pe), pe + gd)
    if form == "table":
        flags, cap = scatter
        out = {"d_table": z(meta.total_rows * 2)}
        ws = z(int(ops.lib.dns_encode_bwd_ws_floats(P, mp, flags, cap)))
        check(ops.lib.dns_encode_bwd(ptr(xd), b6, P, n_bins, *grads, ptr(out["d_table"]), None, None, ptr(ws), flags, cap, stream_ptr()),
              "dns_encode_bwd")
    else:
        out = {"d_x": z(P, 3)}
        check(ops.lib.dns_encode_bwd(ptr(xd), b6, P, n_bins, *grads, None, ptr(out["d_x"]), ptr(jac), None, 0, 0, stream_ptr()),
              "dns_encode_bwd")
    return out


def randomise_(params, seed):
    """Every parameter a distinct seeded value within its own magnitude (equal-shaped networks start out identical)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in params:
            if p.numel():
                p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * max(float(p.detach().abs().max()), 1e-3)).to(p.device))


def scene(nn, nl):
    """A 4-frame synthetic scene with its decoder, built from dns_slam_amd.synthetic alone (the 60 x 80 scene of the GPU tests)."""
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=0)
    cfg = synthetic.default_cfg(n_pixels=400, n_samples_ray=32, n_surface_ray=15, n_frames=4, hash_size=14, voxel_size=0.08,
                                n_neurons=nn, n_hidden_layers=nl, smooth_pts=12)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    randomise_(dec.parameters(), 11)
    with torch.no_grad():
        dec.pe_fn.grid_fn.params.mul_(2000.0)            # the U(-1e-4, 1e-4) init would hide the grid in rounding noise
    return cfg, bound, cam, frames, dec


def track(nn, nl, nu, ns, code):
    """TrackStep.run_fused at the shapes of test_track_step_fused_kernel_equals_the_launch_sequence: 250 rays, 3 iterations."""
    from dns_slam_amd.fused_step import TrackStep
    from dns_slam_amd.tracking import Tracker
    cfg, bound, cam, frames, dec = scene(nn, nl)
    cfg["tracking"]["n_pixels"] = 250
    cfg["training"]["n_samples_ray"], cfg["training"]["n_surface_ray"] = nu, ns
    cur = {k: frames[k][2] for k in ("gt_color", "gt_depth", "gt_label")}
    c2w = frames["est_c2w"][2].clone()
    c2w[:3, 3] += torch.tensor([0.02, -0.01, 0.015], dtype=c2w.dtype)
    n_it, N = 3, 250
    feats = (torch.rand(N, nu + ns, 32, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV) if code else None
    g = torch.Generator().manual_seed(9)
    tracker = Tracker(cfg, dec, bound, cam, device=DEV)
    tracker.border = 5
    tracker.static_shapes = True
    H, W, b = tracker.H, tracker.W, tracker.border
    draws = (torch.randint((H - 2 * b) * (W - 2 * b), (n_it, N), generator=g), torch.rand(n_it, tracker.n_surface_ray, generator=g),
             torch.rand(n_it, tracker.n_surface_ray, generator=g))
    with tracker.frozen_scene():
        ts = TrackStep(tracker, cur, c2w, features=feats)
        assert ts.fused_supported()
        cam7, best = ts.run_fused(n_it, graph=False, draws=draws)
        torch.cuda.synchronize()
        return {"cam7": cam7.clone(), "best": torch.as_tensor(best).clone(), "Q": ts.Q.clone(), "T": ts.T.clone(),
                "fused_out": ts.fused_out.clone()}


def cases():
    yn = {False: "", True: " bound"}
    for hs, res in GRIDS:
        meta = ops.GridMeta(hs, res)
        table = (torch.rand(meta.total_rows * 2, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
        for P in (300, 1):
            tag = f"grid({hs},{res}) P={P}"
            for n_bins in (16, 4):
                x = points(P, n_bins, 7)
                for bound in (False, True):
                    for form, jacs in (("tiled", (False, True)), ("grid", (True,)), ("pe_wide", (False,)), ("untiled", (True,))):
                        for jac in jacs:
                            yield (f"fwd {form}{' dydx' if jac else ''} n_bins={n_bins}{yn[bound]} {tag}",
                                   lambda a=(form, x, table, meta, n_bins, bound, jac): fwd(*a))
                    for form in ("jacobian", "regather", "pe_wide", "untiled"):
                        yield (f"bwd {form} n_bins={n_bins}{yn[bound]} {tag}",
                               lambda a=(form, x, table, meta, n_bins, bound, 11): bwd(*a))
            for n_bins in (16, 8):                         # (the split rows need 3 n_bins % 8 == 0)
                x = points(P, n_bins, 7)
                for bound in (False, True):
                    for form, jac in (("hilo_f32", True), ("hi", False), ("plain_f32", False), ("plain", True)):
                        yield (f"fwd_split {form}{' dydx' if jac else ''} n_bins={n_bins}{yn[bound]} {tag}",
                               lambda a=(form, x, table, meta, n_bins, bound, jac): fwd_split(*a))
            yield f"indices {tag}", lambda a=(points(P, 16, 7), meta): indices(*a)
    # d_table: the scatter forms of tests/test_gpu_kernels.py::test_encode_forward_backward
    meta = ops.GridMeta(16, 592)
    table = (torch.rand(meta.total_rows * 2, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    x = points(3000, 16, 8)
    for name, flags, cap in (("auto", ops.SCATTER_AUTO, 0), ("q", ops.SCATTER_QUEUES, 0), ("q cap 64", ops.SCATTER_QUEUES, 64),
                             ("a", ops.SCATTER_ATOMIC, 0), ("b", ops.SCATTER_BINNED, 0), ("r", ops.SCATTER_AUTO | ops.SCATTER_REPLAY, 0),
                             ("l", ops.SCATTER_AUTO | ops.SCATTER_LISTS, 0), ("l cap 64", ops.SCATTER_AUTO | ops.SCATTER_LISTS, 64)):
        yield (f"bwd d_table {name} grid(16,592) P=3000",
               lambda a=("table", x, table, meta, 16, False, 12, (flags, cap)): bwd(*a))
    for nn, nl, nu, ns in ((64, 2, 32, 15), (32, 1, 22, 10)):
        for code in (False, True):
            yield f"track run_fused(3) {nn}x{nl} S={nu + ns}{' code' if code else ''}", lambda a=(nn, nl, nu, ns, code): track(*a)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the lines to this file instead of stdout")
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    phases = "phases=" + os.environ.get("DNS_ENC_PHASES", "default")
    n = unstable = 0
    for name, run in cases():
        if args.only is not None and args.only not in name:
            continue
        runs = []
        for _ in range(2):
            res = run()
            torch.cuda.synchronize()
            runs.append({k: digest(v) for k, v in res.items()})
        for k in runs[0]:
            same = runs[0][k] == runs[1][k]
            out.write(f"{phases} | {name} | {k} | {runs[0][k] if same else 'unstable'}\n")
            n += 1
            unstable += not same
    if args.out:
        out.close()
    print(f"{n} lines, {unstable} unstable", file=sys.stderr)


if __name__ == "__main__":
    main()
