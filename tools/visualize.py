"""Frames of a finished run: the reference's visualizer.py --save_rendering without a window.  For every frame i = 0 .. idx of the
checkpoint the mesh ``{output}/mesh/{i:05d}_mesh.ply`` (when there is one), the estimated (red) and ground-truth (black) camera
and, every tenth frame, the two trajectories are drawn from the viewer pose of the first estimated camera, and written to
``{output}/tmp_rendering/%06d.png`` (dns_slam_amd/visualize.py; one frame per i, numbered from 1).

    python tools/visualize.py OUTPUT [--ckpt FILE] [--scale 1.0] [--no_gt_traj] [--labels [--classes N]]
                              [--H 720 --W 1280 --fov 60] [--cam_scale 0.1] [--every 1]

OUTPUT: the run's folder.  --ckpt: the checkpoint (default: the first file of OUTPUT, in sorted order, with 'pt' in its name, as
    the reference picks it), a torch file with ``estimate_c2w_list`` and ``gt_c2w_list`` [n,4,4] and ``idx``.
--scale: the configuration's ``scale``; the translations of both pose lists are divided by it (visualizer.py:62-63).
--labels: colour the mesh by the PLY's ``label`` property (meshing.label_colors) instead of its vertex colours, with a palette of
    --classes (default: the largest label + 1) colours spread over the hue circle.
--every: draw only every n-th frame.
The reference's --vis_input_frame (an OpenCV window of the input stream) and its ffmpeg call are not rebuilt; to join the frames:
    ffmpeg -f image2 -r 30 -i OUTPUT/tmp_rendering/%06d.png -y OUTPUT/vis.mp4
"""
import argparse
import colorsys
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dns_slam_amd import evaluation as E, meshing             # noqa: E402
from dns_slam_amd.visualize import Frontend                    # noqa: E402


def hue_palette(n):
    """uint8 [n,3]: n colours spread over the hue circle (class 0 first)."""
    return np.array([[int(round(255 * c)) for c in colorsys.hsv_to_rgb(k / max(n, 1), 0.65, 0.95)] for k in range(n)], np.uint8).reshape(-1, 3)


def find_checkpoint(output):
    names = [f for f in sorted(os.listdir(output)) if "pt" in f and os.path.isfile(os.path.join(output, f))]
    if not names:
        raise SystemExit(f"no checkpoint (a file with 'pt' in its name) in {output}; pass --ckpt")
    return os.path.join(output, names[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("output")
    ap.add_argument("--ckpt")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no_gt_traj", action="store_true")
    ap.add_argument("--labels", action="store_true")
    ap.add_argument("--classes", type=int, default=0)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--cam_scale", type=float, default=0.1)
    ap.add_argument("--every", type=int, default=1)
    a = ap.parse_args(argv)
    path = a.ckpt or find_checkpoint(a.output)
    print("Get ckpt :", path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    est = np.array(torch.as_tensor(ckpt["estimate_c2w_list"]).double().numpy())
    gt = np.array(torch.as_tensor(ckpt["gt_c2w_list"]).double().numpy())
    n = int(ckpt["idx"])
    est[:, :3, 3] /= a.scale
    gt[:, :3, 3] /= a.scale
    shutil.rmtree(os.path.join(a.output, "tmp_rendering"), ignore_errors=True)       # viz.py:57-58
    front = Frontend(a.output, init_pose=est[0], cam_scale=a.cam_scale, near=0, estimate_c2w_list=est, gt_c2w_list=gt, H=a.H, W=a.W,
                     fov_deg=a.fov)
    written = 0
    for i in range(0, n + 1):
        meshfile = os.path.join(a.output, "mesh", f"{i:05d}_mesh.ply")
        if os.path.isfile(meshfile):
            if a.labels:
                m = E.read_ply(meshfile)
                if "labels" not in m:
                    raise SystemExit(f"--labels: {meshfile} has no label property")
                n_class = a.classes or int(m["labels"].max(initial=0)) + 1
                front.update_mesh(m["verts"], m["faces"], meshing.label_colors(m["labels"], hue_palette(n_class)))
            else:
                front.update_mesh(meshfile)
        front.update_pose(1, est[i], gt=False)
        if not a.no_gt_traj:
            front.update_pose(1, gt[i], gt=True)
        if i % 10 == 0:
            front.update_cam_trajectory(i, gt=False)
            if not a.no_gt_traj:
                front.update_cam_trajectory(i, gt=True)
        if i % max(a.every, 1) == 0:
            front.save_frame()
            written += 1
    print(f"{written} frames in {os.path.join(a.output, 'tmp_rendering')}")


if __name__ == "__main__":
    main()
