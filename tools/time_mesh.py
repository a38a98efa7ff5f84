"""Mesher.extract at 256^3 with 50 keyframes on the synthetic room: ms per phase (grid query, keyframe projection, marching
cubes, clean, component filter, vertex query, PLY write), plus the marching cubes and the keyframe projection alone, and the
component pass against its host yardstick (scipy.sparse.csgraph.connected_components on the same mesh) and against a
device sort of the 3F edge keys (the first step of the sort-based alternative to the edge table).

    python tools/time_mesh.py [--res 256] [--kf 50] [--reps 3] [--once]      (--once: one extraction with the component
    filter, for a profiler run)
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
    cfg["meshing"] = {"resolution": a.res, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True,
                      "remove_small_geometry_threshold": 0.2}
    kfs = [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i]}
           for i in range(a.kf)]
    m = Mesher(cfg, mapper)
    if a.once:
        v, f, c, l = m.extract(kfs, components="small")
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
    thr = m.remove_small_geometry_threshold * m.scale * m.scale
    torch.cuda.synchronize()
    t = time.perf_counter()
    m.filter_components(v1, f1, min_area=thr)
    torch.cuda.synchronize()
    t_cc_cold = (time.perf_counter() - t) * 1e3
    t_cc, (v2, f2) = timed(lambda: m.filter_components(v1, f1, min_area=thr), reps)
    t_cc_op, (_, _, n_comp) = timed(lambda: ops.mesh_components(v1, f1), reps)
    fa, fb = f1.long(), f1.long().roll(-1, 1)
    t_sort, _ = timed(lambda: torch.sort(((torch.minimum(fa, fb) << 32) | torch.maximum(fa, fb)).reshape(-1)), reps)
    t_vq, (c, l) = timed(lambda: m.vertex_query(v1, kf), reps)
    t_ext, _ = timed(lambda: m.extract(kfs), reps)
    t_ext_cc, _ = timed(lambda: m.extract(kfs, components="small"), reps)
    import mesh_cc_ref                                       # host yardstick: numpy adjacency + scipy's connected_components
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f1n = f1.cpu().numpy()
    t = time.perf_counter()
    adj = mesh_cc_ref.face_adjacency(f1n)
    t_adj = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    n_host, _ = connected_components(coo_matrix((np.ones(len(adj), np.int8), (adj[:, 0], adj[:, 1])), shape=(len(f1n),) * 2),
                                     directed=False)
    t_scipy = (time.perf_counter() - t) * 1e3
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
    print(f"  components (filter, min_area {thr:g})         {t_cc:8.2f} ms   (first call {t_cc_cold:.2f} ms)   {f1.shape[0]} faces in, "
          f"{n_comp} components, {f2.shape[0]} faces kept")
    print(f"    ops.mesh_components alone                {t_cc_op:8.2f} ms   (sort of its {3 * f1.shape[0]} edge keys alone: {t_sort:.2f} ms)")
    print(f"    host: numpy face adjacency {t_adj:.1f} ms + scipy connected_components {t_scipy:.1f} ms ({n_host} components)")
    print(f"  vertex query (projection + eval_points)    {t_vq:8.2f} ms")
    print(f"  extract (without the component filter)     {t_ext:8.2f} ms")
    print(f"  extract (components='small')               {t_ext_cc:8.2f} ms")
    print(f"  PLY write                                  {t_ply:8.2f} ms")
    print(f"  marching cubes, sphere {a.res}^3 (count + scan + emit + one host read) {t_mc_s:.3f} ms   {vs.shape[0]} vertices")


if __name__ == "__main__":
    main()
