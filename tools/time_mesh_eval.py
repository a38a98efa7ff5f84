"""Mesh evaluation on the 256^3 mesh tools/time_mesh.py builds (the synthetic room, cleaned) and a perturbed copy of it: ms for
the surface sampling, ops.nearest_points at 200 000 x 200 000 (grid, and the all-pairs kernel alone), scipy's cKDTree on the
host for the same clouds, metrics_3d, and ops.frustum_seen at the mesh's vertex count x 2000 poses.

    python tools/time_mesh_eval.py [--res 256] [--kf 50] [--n 200000] [--poses 2000] [--reps 5] [--once]
    (--once: one metrics_3d and one frustum pass, for a profiler run)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import evaluation as E, ops, synthetic    # noqa: E402
from dns_slam_amd.decoder import Decoder                     # noqa: E402
from dns_slam_amd.mapping import Mapper                      # noqa: E402
from dns_slam_amd.meshing import Mesher                      # noqa: E402
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
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
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
    v, f, _, _ = Mesher(cfg, mapper).extract(kfs)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    v2 = v + torch.randn(v.shape, device=dev, generator=g) * 0.01         # the "reconstruction": 1 cm of noise per coordinate
    # trajectory: the keyframe poses repeated with a small drift, in the trajectory file's convention (cull_mesh flips y, z)
    base = torch.stack([torch.as_tensor(frames["est_c2w"][i]) for i in range(a.kf)]).double().numpy()
    c2w = base[np.arange(a.poses) % a.kf].copy()
    c2w[:, :3, 3] += np.random.default_rng(0).normal(size=(a.poses, 3)) * 0.05
    c2w[:, :3, 1:3] *= -1.0
    w2c = torch.from_numpy(E.world_to_camera(c2w)).to(dev)
    H, W = 2 * int(cam["H"]), 2 * int(cam["W"])
    K = (2 * cam["fx"], 2 * cam["fy"], 2 * cam["cx"] + 0.5, 2 * cam["cy"] + 0.5)
    if a.once:
        m = E.metrics_3d(v2, f, v, f, n_samples=a.n)
        seen = ops.frustum_seen(v, w2c, H, W, *K)
        torch.cuda.synchronize()
        print(m, int(seen.sum()))
        return
    reps = a.reps
    t_samp, (gt, _) = timed(lambda: E.sample_surface(v, f, a.n, generator=g), reps)
    rec, _ = E.sample_surface(v2, f, a.n, generator=g)
    t_grid, (d, i, st) = timed(lambda: ops.nearest_points(gt, rec, return_stats=True), reps)
    t_grid_l, _ = timed(lambda: ops.nearest_points_launch(gt, rec), reps)
    t_brute, (db, ib) = timed(lambda: ops.nearest_points(gt, rec, method="brute"), 2)
    same = bool(torch.equal(d.view(torch.int32), db.view(torch.int32)) and torch.equal(i, ib))
    t_met, m = timed(lambda: E.metrics_3d(v2, f, v, f, n_samples=a.n), reps)
    t_fr, seen = timed(lambda: ops.frustum_seen(v, w2c, H, W, *K), reps)
    t_cull, (_, fc) = timed(lambda: E.cull_mesh(v, f, c2w, H, W, *K), reps)
    from scipy.spatial import cKDTree
    gh, rh = gt.cpu().numpy().astype(np.float64), rec.cpu().numpy().astype(np.float64)
    t = time.perf_counter()
    tree = cKDTree(gh)
    t_build = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    dh, _ = tree.query(rh)
    t_query = (time.perf_counter() - t) * 1e3
    worst = float((np.abs(d.cpu().numpy() - dh) / np.maximum(dh, 1e-300)).max() / 2.0 ** -24)
    print(f"mesh {a.res}^3: {v.shape[0]} vertices, {f.shape[0]} faces; {a.n} samples per cloud; {torch.cuda.get_device_name()}")
    print(f"  sample_surface                              {t_samp:9.3f} ms")
    print(f"  nearest_points, grid                        {t_grid:9.3f} ms   ({t_grid_l:.3f} ms without the host read; "
          f"{st['cells']} cells, {st['brute_queries']} queries finished by the all-pairs pass)")
    print(f"  nearest_points, all-pairs kernel alone      {t_brute:9.3f} ms   (same distances and indices: {same})")
    print(f"  host: cKDTree build {t_build:.1f} ms + query {t_query:.1f} ms = {t_build + t_query:9.1f} ms   (device against host: "
          f"worst {worst:.2f} units of 2^-24)")
    print(f"  metrics_3d (2 samplings, 2 nearest passes)  {t_met:9.3f} ms   {m}")
    print(f"  frustum_seen, {v.shape[0]} vertices x {a.poses} poses   {t_fr:9.3f} ms   ({int(seen.sum())} seen)")
    print(f"  cull_mesh (pose inverse on the host + frustum + face rule) {t_cull:9.3f} ms   ({fc.shape[0]} of {f.shape[0]} faces kept)")


if __name__ == "__main__":
    main()
