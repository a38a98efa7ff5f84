"""The scene bound from keyframes (Mesher.get_bound_from_frames: csrc/tsdf.hip, csrc/hull.hip) at the reference's scale: K synthetic
keyframes of H x W at the reference's TSDF parameters (voxel_length 4 / 512, sdf_trunc 0.04, stride 4), phase by phase -- touch
(with the torch compaction and sort of its keys), integrate, vertices, hull (with its round count) and the hull's check passes --
in ms between device events after a warm-up, plus the library's kernel spans per kernel.  The host yardstick, run once, is the
numpy restatement (tests/tsdf_ref.py) and scipy.spatial.ConvexHull on the same data; its results are compared with the device's.
There is no speed gate.

    python tools/time_bound.py [--kf 50] [--H 680] [--W 1200] [--reps 3] [--eps 0] [--no-host | --host-only]

--host-only runs the yardstick alone and needs no GPU.
"""
import argparse
import collections
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic      # noqa: E402
from dns_slam_amd.meshing import open3d_poses  # noqa: E402


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
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    vl, tr = 4.0 / 512.0, 0.04
    cam = synthetic.camera(H=a.H, W=a.W, fx=a.W / 2.0, fy=a.W / 2.0)
    bound, cam, frames = synthetic.make_scene(a.kf, cam=cam, seed=1)
    kfs = [{"est_c2w": frames["est_c2w"][i], "gt_depth": frames["gt_depth"][i]} for i in range(a.kf)]
    ext, pose, centres = open3d_poses(kfs)
    if a.host_only:
        print(f"{a.kf} keyframes of {a.H} x {a.W}, voxel_length {vl}, sdf_trunc {tr}: host yardstick only")
        host(a, frames["gt_depth"].float().numpy(), ext, pose, centres, cam, vl, tr, None)
        return
    dep = frames["gt_depth"].to(dev).float().contiguous()
    e, p = torch.from_numpy(ext).to(dev), torch.from_numpy(pose).to(dev)
    print(f"{a.kf} keyframes of {a.H} x {a.W}, voxel_length {vl}, sdf_trunc {tr}, hull eps {a.eps}, {torch.cuda.get_device_name()}")

    t_fuse, (units, tsdf, weight) = timed(lambda: ops.tsdf_fuse(dep, e, p, cam, vl, tr), a.reps)
    t_vert, verts = timed(lambda: ops.tsdf_vertices(units, tsdf, weight, vl), a.reps)
    pts = torch.cat((torch.from_numpy(centres).to(dev), verts))
    t_hull, (faces, planes, info) = timed(lambda: ops.convex_hull_launch(pts, a.eps), a.reps)
    print(f"  units {units.shape[0]}, vertices {verts.shape[0]}, hull faces {faces.shape[0]}, vertices {torch.unique(faces).numel()}, "
          f"rounds {info['rounds']}, check passes {info['sweeps']}, max_outside {info['max_outside']:.3g}")
    print(f"  tsdf_fuse     {t_fuse:9.3f} ms   (touch, key compaction and sort, integrate)")
    print(f"  tsdf_vertices {t_vert:9.3f} ms   (count, prefix, emit)")
    print(f"  convex_hull   {t_hull:9.3f} ms   ({t_hull * 1e3 / max(info['rounds'], 1):.1f} us per round)")
    # per kernel, from the library's spans (one more call each, timing on)
    ops.timer.arm(kernels=True)
    u2, t2, w2 = ops.tsdf_fuse(dep, e, p, cam, vl, tr)
    ops.tsdf_vertices(u2, t2, w2, vl)
    ops.convex_hull_launch(pts, a.eps)
    torch.cuda.synchronize()
    calls = ops.timer.disarm()
    per = collections.OrderedDict()
    for _, kern, ms, _, _ in ops.timer.kernel_spans:
        n, t = per.get(kern, (0, 0.0))
        per[kern] = (n + 1, t + ms)
    for kern, (n, t) in per.items():
        print(f"  {'':13s} {t:9.3f} ms   {kern} x {n}")
    for name, (n, t, _) in calls.items():
        print(f"  {'':13s} {t:9.3f} ms   {name} (entry point, events around the call)")
    if not a.no_host:
        host(a, dep.cpu().numpy(), ext, pose, centres, cam, vl, tr, (units, tsdf, weight, verts, faces, planes, info))


def host(a, depths, ext, pose, centres, cam, vl, tr, device):
    """numpy restatement + scipy's hull, once; compared with the device's results when there are any."""
    import hull_ref
    import tsdf_ref
    t0 = time.time()
    ref = tsdf_ref.fuse(depths, ext, pose, cam, vl, tr)
    t1 = time.time()
    print(f"  host: numpy fuse {t1 - t0:.1f} s ({len(ref['units'])} units, {len(ref['pairs'])} (unit, frame) pairs)", flush=True)
    rv = tsdf_ref.vertices(ref["units"], ref["tsdf"], ref["weight"], vl)
    t2 = time.time()
    print(f"  host: numpy vertices {t2 - t1:.1f} s ({len(rv)})", flush=True)
    hp = np.concatenate((centres, rv))
    hull = hull_ref.scipy_hull(hp)
    t3 = time.time()
    print(f"  host: scipy ConvexHull {t3 - t2:.2f} s ({len(hull.vertices)} vertices, {len(hull.equations)} faces)")
    if device is None:
        return
    units, tsdf, weight, verts, faces, planes, info = device
    same = (np.array_equal(units.cpu().numpy(), ref["units"]) and np.array_equal(tsdf.cpu().numpy().view(np.uint32), ref["tsdf"].view(np.uint32))
            and np.array_equal(weight.cpu().numpy(), ref["weight"]) and np.array_equal(verts.cpu().numpy().view(np.uint64), rv.view(np.uint64)))
    print(f"  device == restatement bit for bit: {same}")
    print("  hull acceptance:", hull_ref.accept(hp, a.eps, torch.unique(faces).cpu().numpy(), faces.cpu().numpy(), planes.cpu().numpy(),
                                             info["max_outside"], hull))


if __name__ == "__main__":
    main()
