"""Point masks (csrc/mesh_masks.hip, ops.point_masks) at the reference's scale: the res^3 query grid of the synthetic room against
K keyframes of H x W, in each mode -- frustum only, depth limit, depth test (pass 1, the chunk maxima, and pass 2 separately from
the library's kernel spans) -- in ms, against the torch composition of the same mode (tests/point_masks_ref.py on the device: the
reference's per-chunk, per-keyframe loop with grid_sample), with the number of points on which the two differ.

    python tools/time_point_masks.py [--res 256] [--kf 50] [--H 680] [--W 1200] [--chunk 500000] [--reps 5] [--no-torch]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic      # noqa: E402
import point_masks_ref                       # noqa: E402


def timed(fn, reps):
    """ms per call between device events, after one warm-up call; the last result"""
    out = fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--chunk", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    cam = synthetic.camera(H=a.H, W=a.W, fx=a.W / 2.0, fy=a.W / 2.0)
    bound, cam, frames = synthetic.make_scene(a.kf, cam=cam, seed=1)
    b = bound.numpy()
    ax = [torch.tensor(np.linspace(b[i][0] - 0.05, b[i][1] + 0.05, a.res), device=dev).float() for i in range(3)]
    n = torch.arange(a.res ** 3, device=dev)
    pts = torch.stack((ax[0][(n // a.res) % a.res], ax[1][n // (a.res * a.res)], ax[2][n % a.res]), 1).contiguous()
    del n
    P = pts.shape[0]
    w2c = torch.inverse(frames["est_c2w"].to(dev)).float()
    dep = frames["gt_depth"].to(dev).float().contiguous()
    md = dep.reshape(a.kf, -1).max(1).values
    print(f"{P} points ({a.res}^3) x {a.kf} keyframes of {a.H} x {a.W}, chunk {a.chunk}, {torch.cuda.get_device_name()}")
    modes = (("frustum only", {}), ("depth limit", {"max_depth": md}), ("depth test", {"depths": dep, "chunk": a.chunk}))
    for name, kw in modes:
        t, cls = timed(lambda: ops.point_masks(pts, w2c, cam, a.H, a.W, **kw), a.reps)
        share = [float((cls == c).float().mean()) * 100 for c in (1, 2, 0)]
        line = (f"  {name:13s} {t:9.3f} ms   {t * 1e6 / (P * a.kf):6.3f} ns per point and keyframe   seen / forecast / unseen "
                f"{share[0]:.1f} / {share[1]:.1f} / {share[2]:.1f} %")
        print(line)
        if name == "depth test":
            ops.timer.arm(kernels=True)
            ops.point_masks(pts, w2c, cam, a.H, a.W, **kw)
            torch.cuda.synchronize()
            ops.timer.disarm()
            for _, kern, ms, _, _ in ops.timer.kernel_spans:
                print(f"  {'':13s} {ms:9.3f} ms   {kern}")
        if a.no_torch:
            continue
        tt, ref = timed(lambda: point_masks_ref.point_masks_ref(pts, w2c, cam, a.H, a.W, **kw), 1)
        rc = point_masks_ref.classes(ref[0], ref[1])
        bad = cls != rc
        print(f"  {'':13s} {tt:9.1f} ms   torch composition ({tt / t:.0f} x); {int(bad.sum())} points differ, "
              f"{int((bad & ~ref[3]).sum())} of them away from a threshold ({int(ref[3].sum())} flagged)")


if __name__ == "__main__":
    main()
