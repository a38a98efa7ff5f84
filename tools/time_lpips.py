"""ops.lpips (csrc/lpips.hip) at the reference's frame size: one pair of 680 x 1200 images and a batch of 8 pairs, method="fused"
against method="torch" (the same definition composed of F.conv2d / F.max_pool2d, in the library's two memory formats) in ONE
process, alternating them, timed with device events after a warm-up: median and spread (min .. max) of ``--reps`` repetitions.
The first call of each method (code objects, the library's search for an algorithm) is timed apart, by the host clock round a
synchronise.  Then every kernel of the fused path on its own: the convolutions with the operations their shapes need
(2 n h w Cout k k Cin) against the 157 TFLOP/s of the fp32 matrix instruction, the pools and the heads with the bytes they must move
against the HBM rate.  Then evaluation.render_metrics of one H x W frame with and without ``lpips=`` (fused).

    python tools/time_lpips.py [--H 680] [--W 1200] [--reps 20] [--batch 8] [--no-render] [--out profiles/lpips_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import evaluation, ops, synthetic          # noqa: E402

MFMA_F32_TFLOPS = 157.0
HBM_GBS = 8000.0
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def random_weights(seed):
    """He-normal convolutions, bias 0.1 randn, lin uniform in [0, 0.1] (what tests/lpips_ref.py draws)"""
    g = torch.Generator().manual_seed(seed)
    convs = [(torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (ks * ks * cin)) ** 0.5, torch.randn(cout, generator=g) * 0.1)
             for _, cin, cout, ks, _, _, _ in ops.LPIPS_LAYERS]
    lins = [torch.rand(cout, generator=g) * 0.1 for _, _, cout, _, _, _, _ in ops.LPIPS_LAYERS]
    return ops.LpipsWeights(convs, lins)


def alternate(fns, reps, warm=3):
    """ms per call of every function, called in turn: [(median, min, max)]"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        t = [a.elapsed_time(b) for a, b in ev[k]]
        out.append((statistics.median(t), min(t), max(t)))
    return out


def first_call(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def fmt(r):
    return f"{r[0]:.3f} ms ({r[1]:.3f} .. {r[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_time.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    H, W = a.H, a.W
    wts = random_weights(0)
    shapes = ops.lpips_feature_shapes(H, W)
    flops = 0
    for (h, w, c), (_, cin, cout, ks, _, _, _) in zip(shapes, ops.LPIPS_LAYERS):
        flops += 2 * h * w * cout * ks * ks * cin
    say(f"{torch.cuda.get_device_name()}: ops.lpips, images {H} x {W}, features {shapes}, {2 * flops / 1e9:.1f} GFLOP per pair "
        f"(two images); {a.reps} alternating repetitions after 3 warm-up calls, device events: median (min .. max)")
    g = torch.Generator(device=dev).manual_seed(0)
    for F in (1, a.batch):
        gt = torch.rand(F, H, W, 3, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(F, H, W, 3, device=dev, generator=g)).clamp(0, 1)
        fused = lambda: ops.lpips_launch(pred, gt, wts, method="fused")
        t_nchw = lambda: ops._lpips_torch(pred, gt, wts, channels_last=False)
        t_nhwc = lambda: ops._lpips_torch(pred, gt, wts, channels_last=True)
        say(f"F = {F}: first call: fused {first_call(fused):.0f} ms, torch (contiguous) {first_call(t_nchw):.0f} ms, "
            f"torch (channels_last) {first_call(t_nhwc):.0f} ms  [host clock round a synchronise]")
        rf, rc, rl = alternate([fused, t_nchw, t_nhwc], a.reps)
        vf, vt = fused()[0], t_nchw()[0]
        best = min(rc, rl)
        say(f"F = {F}: fused {fmt(rf)} = {2 * F * flops / rf[0] / 1e9:.1f} TFLOP/s end to end; torch contiguous {fmt(rc)}, "
            f"torch channels_last {fmt(rl)}; faster torch / fused = {best[0] / rf[0]:.2f}; "
            f"lpips[0] fused {float(vf[0]):.9f} torch {float(vt[0]):.9f}")
        if F != 1:
            continue
        # the kernels of the fused path one by one, on the maps of this pair (2 images per launch)
        convs, lins, packs = wts.on(torch.device(dev))
        sp = ops.stream_ptr()
        x = torch.cat((pred, gt))
        n, h, w = 2, H, W
        for l, ((wt, b), lin, pack, (_, cin, cout, ks, stride, pad, pooled)) in enumerate(zip(convs, lins, packs, ops.LPIPS_LAYERS)):
            if pooled:
                xin = x
                r, = alternate([lambda: ops._launch_pool(xin, sp)], a.reps)
                x = ops._launch_pool(xin, sp)
                nbytes = (xin.numel() + x.numel()) * 4
                say(f"  pool before conv{l + 1}: {tuple(xin.shape)} -> {tuple(x.shape)}: {fmt(r)}, {nbytes / r[0] / 1e6:.0f} GB/s "
                    f"({100 * nbytes / r[0] / 1e6 / HBM_GBS:.0f} % of {HBM_GBS:.0f})")
                h, w = int(x.shape[1]), int(x.shape[2])
            flags = ops.CONV_RELU | (ops.CONV_SCALE_INPUT if l == 0 else 0)
            xin, hh, ww = x, h, w
            r, = alternate([lambda: ops._launch_conv(xin, n, hh, ww, cin, pack, b, cout, ks, stride, pad, flags, sp)], a.reps)
            x = ops._launch_conv(xin, n, hh, ww, cin, pack, b, cout, ks, stride, pad, flags, sp)
            h, w = int(x.shape[1]), int(x.shape[2])
            fl = 2 * n * h * w * cout * ks * ks * cin
            tiles = n * ((h + 7) // 8) * ((w + 31) // 32) * (cout // 64)
            say(f"  conv{l + 1}: {tuple(xin.shape)} -> {tuple(x.shape)}, K = {ks * ks * cin}, {tiles} workgroups: {fmt(r)}, "
                f"{fl / r[0] / 1e9:.1f} TFLOP/s ({100 * fl / r[0] / 1e9 / MFMA_F32_TFLOPS:.0f} % of {MFMA_F32_TFLOPS:.0f})")
            feat = x
            r, = alternate([lambda: ops._launch_head(feat[:1], feat[1:], lin, 1, h, w, cout, sp)], a.reps)
            nbytes = feat.numel() * 4
            say(f"  head{l}: {tuple(feat.shape[1:])}: {fmt(r)}, {nbytes / r[0] / 1e6:.0f} GB/s ({100 * nbytes / r[0] / 1e6 / HBM_GBS:.0f} % of "
                f"{HBM_GBS:.0f})")
    if not a.no_render:
        from dns_slam_amd.decoder import Decoder
        from dns_slam_amd.mapping import Mapper
        from util import randomise_
        cam = synthetic.camera(H=H, W=W, fx=W / 2.0, fy=W / 2.0)
        bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=1)
        cfg = synthetic.default_cfg(n_neurons=32, n_hidden_layers=1)
        dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
        mapper = Mapper(cfg, dec, bound, cam, device=dev)
        mapper.set_decoder(frames)
        randomise_(dec, 1)
        randomise_([mapper.fine_decoders.pool], 2)
        jit = [mapper.draw_jitter(1)]
        fns = [lambda: evaluation.render_metrics(mapper, frames, indices=[3], jitters=jit),
               lambda: evaluation.render_metrics(mapper, frames, indices=[3], jitters=jit, lpips=wts, lpips_method="fused")]
        r0, r1 = alternate(fns, max(a.reps // 5, 2), warm=1)
        say(f"render_metrics, one frame of {H} x {W}, chunks of {mapper.cfg['mapping'].get('n_pts_batch', 1000)} rays: without lpips= "
            f"{fmt(r0)}, with lpips= (fused) {fmt(r1)}")
    say(f"peak memory {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
