"""The 2-D code of a rendered frame's samples (csrc/frame_codes.hip, ops.frame_codes) at the reference's scale: stem maps of
340 x 600 x 64, R = 3 (frame_vis) and R = 1 (novel_view_render) views, a chunk of 1000 rays x 47 samples (the reference's
n_pts_batch) and one of 65 536 rays, both Merge shapes -- method="fused" against method="launches" in ONE process, alternating
the two, timed with device events after a warm-up: median and spread (min .. max) of ``--reps`` repetitions.  Both methods are
handed the views' origins (``origins=``, computed once, as render_frame does per frame), so neither inverts a pose inside the
timed call.  Bytes and
operations are taken from the shapes: per point 12 B read and 4 hid B written are compulsory (the maps stay in cache); per (point,
view) pair the Merge network is 2 (n_in nn + (nl - 1) nn^2 + nn hid) fp32-grade operations = three times as many f16 matrix
operations.  Then a whole Mapper.render_frame of H x W with and without ``refer_frames``.

    python tools/time_frame_codes.py [--H 680] [--W 1200] [--reps 20] [--rays 1000 65536] [--no-render] [--tiles]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic                      # noqa: E402
from dns_slam_amd.common import get_quad_from_c2w            # noqa: E402
from dns_slam_amd.decoder import Decoder                     # noqa: E402
from dns_slam_amd.encoder import ResNet                      # noqa: E402
from dns_slam_amd.mapping import Mapper                      # noqa: E402
from util import randomise_                                  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, nargs="+", default=[1000, 65536])
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--tiles", action="store_true", help="also time the fused kernel at every tile size")
    a = ap.parse_args()
    dev = "cuda:0"
    H, W = a.H, a.W
    cam = synthetic.camera(H=H, W=W, fx=W / 2.0, fy=W / 2.0)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=1)
    enc = ResNet(seed=0, backend="hip").to(dev)
    views = [3, 2, 1]                                            # the frame itself first: R = 1 is novel_view_render's view
    stem = enc.forward_channels_last(frames["gt_color"][views].to(dev))
    w2c = torch.inverse(frames["est_c2w"][views].to(dev).float()).contiguous()
    print(f"{torch.cuda.get_device_name()}: images {H} x {W}, stem maps {tuple(stem.shape[1:])} ({stem[0].numel() * 4 / 1e6:.0f} MB per view)")
    i = 3
    mappers = {}
    for nn, nl in ((32, 1), (64, 2)):
        cfg = synthetic.default_cfg(n_neurons=nn, n_hidden_layers=nl)
        dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
        mapper = Mapper(cfg, dec, bound, cam, device=dev)
        mapper.set_decoder(frames)
        randomise_(dec, 1)
        randomise_([mapper.fine_decoders.pool], 2)
        mappers[(nn, nl)] = mapper
        merge, net = dec.merge, dec.merge.decoder
        n_in, hid = net.n_input_dims, net.n_output_dims
        flop_pair = 2 * (n_in * nn + (nl - 1) * nn * nn + nn * hid)
        for n_rays in a.rays:
            g = torch.Generator().manual_seed(n_rays)
            pix = torch.randint(0, H * W, (n_rays,), generator=g).to(dev)
            c2w = frames["est_c2w"][i]
            f = lambda t: t.to(dev).float().contiguous()[None]
            jit = mapper.draw_jitter(1)
            res = ops.raygen_sample(get_quad_from_c2w(c2w).to(dev)[None], c2w[:3, 3].to(dev).float()[None], pix, f(frames["gt_color"][i]),
                                    f(frames["gt_depth"][i]), f(frames["gt_label"][i]), (mapper.fx, mapper.fy, mapper.cx, mapper.cy),
                                    mapper.bound, (0, H, 0, W), n_rays, mapper.t_uniform, jit[0], jit[1])
            pts = res[2].reshape(-1, 3).contiguous()
            P = pts.shape[0]
            for R in (3, 1):
                org = torch.inverse(w2c[:R])[:, :3, 3].contiguous()       # once per frame, as render_frame passes it
                call = lambda m: ops.frame_codes(pts, w2c[:R], stem[:R], cam, H, W, merge, method=m, origins=org)
                cf, cl = call("fused"), call("launches")
                diff = float((cf - cl).abs().max() / cl.abs().max())
                K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])
                valid = float(ops.feature_gather(pts, w2c[:R], K, stem[:R], H, W)[1].float().mean())
                (tf, tf0, tf1), (tl, tl0, tl1) = alternate([lambda: call("fused"), lambda: call("launches")], a.reps)
                pairs = P * R
                if a.tiles:
                    tt = alternate([(lambda t=t: ops.frame_codes(pts, w2c[:R], stem[:R], cam, H, W, merge, method="fused", origins=org, tile=t))
                                    for t in (32, 64, 128)], a.reps)
                    print("    fused by tile size: " + ", ".join(f"{t}: {m:.3f} ms ({lo:.3f} .. {hi:.3f})" for t, (m, lo, hi) in zip((32, 64, 128), tt)))
                print(f"Merge {nn} x {nl}, {n_rays} rays x {P // n_rays} = {P} points, R = {R} ({100 * valid:.0f} % of the pairs valid): "
                      f"fused {tf:.3f} ms ({tf0:.3f} .. {tf1:.3f}), launches {tl:.3f} ms ({tl0:.3f} .. {tl1:.3f}), ratio {tl / tf:.2f}; "
                      f"fused: {pairs / tf / 1e6:.2f} G pairs/s, {pairs * flop_pair / tf / 1e9:.1f} TFLOP/s fp32-grade "
                      f"(x 3 as f16 matrix operations: {3 * pairs * flop_pair / tf / 1e9:.0f}), {P * (12 + 4 * hid) / tf / 1e6:.1f} GB/s compulsory, "
                      f"{pairs * valid * 4 * 64 * 4 / tf / 1e6:.0f} GB/s of taps; max |fused - launches| = {diff:.1e} of the scale")
    if a.no_render:
        return
    mapper = mappers[(32, 1)]
    mapper.encoder = enc
    args = (frames["gt_color"][i], frames["gt_depth"][i], frames["gt_label"][i], frames["est_c2w"][i])
    jit = mapper.draw_jitter(1)
    for R in (3, 1):
        refer = {"stem": stem[:R], "est_c2w": frames["est_c2w"][views[:R]]}
        fns = [lambda: mapper.render_frame(*args, jitter=jit),
               lambda: mapper.render_frame(*args, jitter=jit, refer_frames=refer, code_method="fused"),
               lambda: mapper.render_frame(*args, jitter=jit, refer_frames=refer, code_method="launches")]
        res = alternate(fns, max(a.reps // 5, 2), warm=1)
        for name, (t, t0, t1) in zip(("no 2-D code", "refer_frames, fused", "refer_frames, launches"), res):
            print(f"render_frame {H} x {W}, chunks of {mapper.cfg['mapping'].get('n_pts_batch', 1000)} rays, Merge 32 x 1, R = {R}, {name}: "
                  f"{t:.1f} ms ({t0:.1f} .. {t1:.1f})")
    print(f"peak memory {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")


if __name__ == "__main__":
    main()
