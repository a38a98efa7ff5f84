#!/usr/bin/env python3
"""Runs a sequence end to end: trajectory, map, meshes, checkpoints and frame_vis sheets from a configuration file.

    python tools/run_slam.py CONFIG [--frames N] [--out DIR] [--stem] [--device cuda]

CONFIG: a yaml file with the reference's keys (configs/synthetic.yaml runs the box room of dns_slam_amd/synthetic.py and needs no
dataset on disk; `dataset: replica` / `scannet` read cfg['dataset_dir'] / dataset / scene through dns_slam_amd.datasets).
--frames: the first N frames only.  --out: replaces cfg['out_dir'].  --stem: a frozen image stem (encoder.ResNet, seed 0) feeds
the 2-D branch.  The output folder holds output_front.txt, output_back_fine.txt, model_{idx}.pt, model.pt, {idx:05d}.png and
mesh/{idx:05d}_mesh.ply; `python tools/visualize.py FOLDER` draws it.
"""
import argparse
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config")
    ap.add_argument("--frames", type=int)
    ap.add_argument("--out")
    ap.add_argument("--stem", action="store_true")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    if a.out:
        cfg["out_dir"] = a.out
    import torch
    from dns_slam_amd import evaluation
    from dns_slam_amd.slam import DNS_SLAM
    if not torch.cuda.is_available():
        raise SystemExit("run_slam: no GPU visible; dns_slam_amd has no CPU path")
    if cfg.get("dataset") == "synthetic" and a.frames:
        cfg.setdefault("synthetic", {})["n_frames"] = a.frames
    encoder = None
    if a.stem:
        from dns_slam_amd.encoder import ResNet
        encoder = ResNet(seed=0).to(a.device)
    slam = DNS_SLAM(cfg, device=a.device, encoder=encoder, n_img=a.frames)
    print(f"{slam.n_img} frames of {slam.cam['H']} x {slam.cam['W']}, {len(slam.plan)} events -> {slam.out_dir}")
    slam.run(on_event=lambda ev, payload: print(" ".join(str(v) for v in ev)) if cfg.get("verbose", True) else None)
    t = slam.timing
    print(f"done: {t['total']:.2f} s (tracking {t['track']:.2f}, mapping {t['map']:.2f}, everything else {t['total'] - t['track'] - t['map']:.2f})")
    ate = evaluation.evaluate_ate(slam.gt_c2w_list, slam.estimate_c2w_list)
    print(f"ATE rmse {ate['absolute_translational_error.rmse']:.4f} m over {ate['compared_pose_pairs']} poses")
    print("model:", os.path.join(slam.out_dir, "model.pt"))


if __name__ == "__main__":
    main()
