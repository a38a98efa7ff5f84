"""The ICP alignment (evaluation.align_transformation = ops.icp_point_to_point) on the vertex clouds of the 256^3 mesh
tools/time_mesh.py builds (the synthetic room, cleaned) and of a noisy, slightly moved copy of it: ms for the registration, for
its parts (grid build + one pass; a further pass), and for the two things it is measured against:

    - the host restatement (tests/icp_ref.py: scipy's cKDTree built once, one query per pass) on the same clouds: the build and
      ONE query are timed and the query is multiplied by the number of passes;
    - the same number of passes out of the pieces the library had before: ops.nearest_points_launch (which rebuilds the grid on
      every call) on the transformed cloud, the correspondence sums and the rigid update with torch ops, no host read inside.

    python tools/time_icp.py [--res 256] [--kf 50] [--reps 3] [--once]
    (--once: one align_transformation, for a profiler run)
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
import icp_ref                                               # noqa: E402


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def from_pieces(src, tgt, max_dist, passes):
    """`passes` evaluations and passes - 1 updates out of nearest_points_launch and torch ops (float64 sums, SVD Kabsch)."""
    T = torch.eye(4, dtype=torch.float64, device=src.device)
    tgt64 = tgt.double()
    for k in range(passes):
        p32 = E.apply_transform(src, T)
        d, idx, _ = ops.nearest_points_launch(tgt, p32)
        w = (d <= max_dist).double()[:, None]
        p, q = p32.double(), tgt64[idx.long()]
        n = w.sum()
        mp, mq = (w * p).sum(0) / n, (w * q).sum(0) / n
        if k == passes - 1:
            break
        H = ((p - mp) * w).T @ (q - mq)
        U, _, Vt = torch.linalg.svd(H)
        D = torch.eye(3, dtype=torch.float64, device=src.device)
        D[2, 2] = torch.sign(torch.linalg.det(Vt.T @ U.T))
        R = Vt.T @ D @ U.T
        upd = torch.eye(4, dtype=torch.float64, device=src.device)
        upd[:3, :3], upd[:3, 3] = R, mq - R @ mp
        T = upd @ T
    return T


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
    v, _, _, _ = Mesher(cfg, mapper).extract(kfs)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    motion = icp_ref.rigid((1.0, 2.0, 3.0), 1.0, (0.02, -0.01, 0.015))
    noisy = v + torch.randn(v.shape, device=dev, generator=g) * 0.01     # the "reconstruction": 1 cm of noise, then moved
    rec = E.apply_transform(noisy, np.linalg.inv(motion))
    if a.once:
        T, info = E.align_transformation(rec, v, return_info=True)
        print({k: info[k] for k in ("fitness", "inlier_rmse", "iterations", "converged", "brute_queries")})
        return
    th = 0.1
    t_icp, (T, info) = timed(lambda: E.align_transformation(rec, v, th, return_info=True), a.reps)
    passes = info["iterations"] + 1
    t_one, _ = timed(lambda: ops.icp_point_to_point_launch(rec, v, th, max_iter=0), a.reps)
    t_11, _ = timed(lambda: ops.icp_point_to_point_launch(rec, v, th, max_iter=10, relative_fitness=0.0, relative_rmse=0.0), a.reps)
    t_nn, _ = timed(lambda: ops.nearest_points_launch(v, rec), a.reps)
    t_pieces, Tp = timed(lambda: from_pieces(rec, v, th, passes), 1)
    vh, rh = v.cpu().numpy().astype(np.float64), rec.cpu().numpy()
    t = time.perf_counter()
    tree = icp_ref.cKDTree(vh)
    t_build = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    tree.query(icp_ref.transform32(np.eye(4), rh).astype(np.float64))
    t_query = (time.perf_counter() - t) * 1e3
    err = float((T.cpu() @ torch.from_numpy(motion).inverse() - torch.eye(4, dtype=torch.float64)).abs().max())
    print(f"ICP on {rec.shape[0]} source x {v.shape[0]} target vertices (mesh {a.res}^3), max_dist {th}; {torch.cuda.get_device_name()}")
    print(f"  align_transformation (one host read)         {t_icp:9.3f} ms   ({info['iterations']} updates, {passes} passes, "
          f"converged {info['converged']}, fitness {info['fitness']:.4f}, rmse {info['inlier_rmse']:.5f}, |T G^-1 - I| {err:.2e}, "
          f"{info['brute_queries']} queries finished by the all-pairs pass)")
    print(f"  grid build + pass 0 (max_iter = 0)           {t_one:9.3f} ms")
    print(f"  a further pass ((11 passes - 1 pass) / 10)   {(t_11 - t_one) / 10:9.3f} ms   (11 passes: {t_11:.3f} ms)")
    print(f"  one nearest_points_launch, same clouds       {t_nn:9.3f} ms")
    print(f"  {passes} passes out of nearest_points + torch ops  {t_pieces:9.3f} ms   (|T - T_icp| "
          f"{float((Tp - T).abs().max()):.2e})")
    print(f"  host: cKDTree build {t_build:.1f} ms + {passes} x query {t_query:.1f} ms = {t_build + passes * t_query:9.1f} ms   "
          f"(one query measured)")


if __name__ == "__main__":
    main()
