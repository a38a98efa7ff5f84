"""Mesher.extract at 256^3 with 50 keyframes on the synthetic room: ms per phase (grid query, keyframe projection, marching
cubes, vertex query, PLY write), plus the marching cubes and the keyframe projection alone.

    python tools/time_mesh.py [--res 256] [--kf 50] [--reps 3] [--once]      (--once: one extraction, for a profiler run)
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic                      # noqa: E402
from dns_slam_amd.decoder import Decoder                     # noqa: E402
from dns_slam_amd.mapping import Mapper                      # noqa: E402
from dns_slam_amd.meshing import Mesher, write_ply           # noqa: E402
from util import randomise_                                  # noqa: E402


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    cam = synthetic.camera(H=120, W=160, fx=120.0, fy=120.0)
    bound, cam, frames = synthetic.make_scene(a.kf, cam=cam, seed=1)
    cfg = synthetic.default_cfg()
    dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
    mapper = Mapper(cfg, dec, bound, cam, device=dev)
    mapper.set_decoder(frames)
    randomise_(dec, 1)
    randomise_([mapper.fine_decoders.pool], 2)
    cfg["meshing"] = {"resolution": a.res, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True}
    kfs = [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i]}
           for i in range(a.kf)]
    m = Mesher(cfg, mapper)
    if a.once:
        v, f, c, l = m.extract(kfs)
        torch.cuda.synchronize()
        print(f"extract: {v.shape[0]} vertices, {f.shape[0]} faces")
        return
    reps = a.reps
    kf = m._keyframes(kfs)
    grid = m.get_grid_uniform()
    P = a.res ** 3
    pts = m.grid_points(grid["xyz"], 0, P)
    t_proj, (lab, _) = timed(lambda: ops.keyframe_project(pts, kf[0], kf[1], kf[2], m.cam), reps)
    t_occ, _ = timed(lambda: mapper.eval_occupancy(pts, lab, rule_chunk=16384), reps)
    t_evp, _ = timed(lambda: mapper.eval_points(pts, None, lab, rule_chunk=16384), 1)
    t_grid, (vol, _) = timed(lambda: m.grid_occupancy(kfs, kf=kf), reps)
    x, y, z = grid["xyz"]
    mc = lambda: ops.marching_cubes(vol, 0.0, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
    t_mc, (v, f) = timed(mc, reps)
    t_clean, (v1, f1) = timed(lambda: m.clean(v, f, kf), reps)
    t_vq, (c, l) = timed(lambda: m.vertex_query(v1, kf), reps)
    t_ext, _ = timed(lambda: m.extract(kfs), reps)
    vn, fn, cn, ln = v1.cpu().numpy(), f1.cpu().numpy(), c.cpu().numpy(), l.cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        t = time.perf_counter()
        write_ply(os.path.join(d, "mesh.ply"), vn, fn, cn, ln)
        t_ply = (time.perf_counter() - t) * 1e3
    # marching cubes on a smooth field of the same size (a sphere): the kernels alone
    ax = torch.linspace(-1, 1, a.res, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sph = (0.6 - (X * X + Y * Y + Z * Z).sqrt()).contiguous()
    sp = float(ax[1] - ax[0])
    t_mc_s, (vs, fs) = timed(lambda: ops.marching_cubes(sph, 0.0, (-1, -1, -1), (sp, sp, sp)), reps * 3)
    print(f"grid {a.res}^3 = {P} points, {a.kf} keyframes, {torch.cuda.get_device_name()}")
    print(f"  keyframe projection (grid, alone)          {t_proj:8.2f} ms")
    print(f"  eval_occupancy (grid, alone)               {t_occ:8.2f} ms   (eval_points on the same points: {t_evp:.2f} ms)")
    print(f"  grid query (points + projection + occ.)    {t_grid:8.2f} ms")
    print(f"  marching cubes (query volume)              {t_mc:8.2f} ms   {v.shape[0]} vertices, {f.shape[0]} faces")
    print(f"  clean (projection of the vertices + compaction) {t_clean:5.2f} ms   {v1.shape[0]} vertices, {f1.shape[0]} faces kept")
    print(f"  vertex query (projection + eval_points)    {t_vq:8.2f} ms")
    print(f"  extract (all of the above, end to end)     {t_ext:8.2f} ms")
    print(f"  PLY write                                  {t_ply:8.2f} ms")
    print(f"  marching cubes, sphere {a.res}^3 (count + scan + emit + one host read) {t_mc_s:.3f} ms   {vs.shape[0]} vertices")


if __name__ == "__main__":
    main()
