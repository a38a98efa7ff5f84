"""Accuracy (cm), completion (cm) and completion ratio (%) of a reconstructed mesh against a ground-truth mesh: the
reference's eval_3d.py (calc_3d_metric), preceded by its cull_mesh.py when a trajectory is given.

    python tools/eval_mesh.py --rec A.ply --gt B.ply [--align [--align-threshold 0.1]]
                              [--traj T --H 680 --W 1200 --fx 600 --fy 600 --cx 599.5 --cy 339.5]
                              [--n 200000] [--dist-th 0.05] [--seed 0]
                              [--depth-l1 [--n-imgs 1000] [--unseen FILE.npy]]

--align: register the vertices of --rec to those of --gt first (the reference's get_align_transformation: point-to-point ICP from
    the identity, correspondence distance 0.1, its default in calc_3d_metric); the transformation, fitness and inlier rmse go to
    stderr.  Off by default here: without it the meshes are measured as they are.
--depth-l1: also print "Depth L1" (cm), the reference's calc_2d_metric: --n-imgs views of 500 x 500 drawn (from --seed) inside the
    ground-truth mesh's axis-aligned box scaled as the reference scales its oriented box, rejecting the views that see a point of
    the cloud --unseen (an [N,3] .npy file, the reference's *_pc_unseen.npy); with --align the registered reconstruction is used.
--traj: text file of camera-to-world poses, 16 numbers per line; the faces of --rec no pose sees are dropped first.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dns_slam_amd import evaluation as E                     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rec", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--traj")
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--fx", type=float, default=600.0)
    ap.add_argument("--fy", type=float, default=600.0)
    ap.add_argument("--cx", type=float, default=599.5)
    ap.add_argument("--cy", type=float, default=339.5)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--dist-th", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--align-threshold", type=float, default=0.1)
    ap.add_argument("--depth-l1", action="store_true")
    ap.add_argument("--n-imgs", type=int, default=1000)
    ap.add_argument("--unseen")
    a = ap.parse_args()
    dev = "cuda:0"
    rec, gt = E.read_ply(a.rec), E.read_ply(a.gt)
    rv, rf = torch.from_numpy(rec["verts"]).to(dev), torch.from_numpy(rec["faces"]).to(dev)
    gv, gf = torch.from_numpy(gt["verts"]).to(dev), torch.from_numpy(gt["faces"]).to(dev)
    if a.traj:
        n_faces = rf.shape[0]
        rv, rf = E.cull_mesh(rv, rf, E.load_poses(a.traj), a.H, a.W, a.fx, a.fy, a.cx, a.cy)
        print(f"culled {n_faces - rf.shape[0]} of {n_faces} faces", file=sys.stderr)
    m = E.calc_3d_metric(rv, rf, gv, gf, align=a.align, threshold=a.align_threshold, n_samples=a.n, dist_th=a.dist_th, seed=a.seed)
    if a.align:
        icp = m["icp"]
        print("transformation:", file=sys.stderr)
        for row in m["transformation"].cpu().tolist():
            print("  " + " ".join(f"{x: .9f}" for x in row), file=sys.stderr)
        print(f"fitness {icp['fitness']:.6f}, inlier rmse {icp['inlier_rmse']:.6f} ({icp['correspondences']} correspondences, "
              f"{icp['iterations']} updates, {'converged' if icp['converged'] else 'not converged'})", file=sys.stderr)
    print("accuracy: ", m["accuracy_cm"])
    print("completion: ", m["completion_cm"])
    print("completion ratio: ", m["completion_ratio_pct"])
    if a.depth_l1:
        import numpy as np
        unseen = torch.from_numpy(np.load(a.unseen).astype(np.float32).reshape(-1, 3)).to(dev) if a.unseen else None
        rv2 = E.apply_transform(rv, m["transformation"]) if a.align else rv
        d = E.calc_2d_metric(rv2, rf, gv, gf, align=False, n_imgs=a.n_imgs, unseen_pts=unseen, seed=a.seed)
        print("Depth L1: ", d["depth_l1_cm"])


if __name__ == "__main__":
    main()
