#!/usr/bin/env python3
"""The driver's costs, measured on the device:

    python tools/time_slam.py [--items 1,2,3,4] [--reps 20] [--run-reps 2] [--out profiles/slam_time.txt]

1. A 40-frame synthetic run at 480 x 640 (slam.DNS_SLAM on synthetic.SyntheticSequence, outputs off): wall time split into tracking,
   mapping and everything else -- the driver's own share -- and the ATE (evaluation.evaluate_ate).  ``--run-reps`` whole runs after
   one uncounted warm-up run.
2. Mapper.set_target_refer_frames with 50 keyframes at 680 x 1200 and n_joint_optimize_frames = 7: keyframes.KeyframeBank on the
   device against host keyframes (the reference's CPU tensors), the same seeds, host clock around the call + a synchronise.
3. ops.keyframe_overlap against the torch block of Mapper.keyframe_selection_overlap at 1600 points x {50, 400} keyframes, poses on
   the device for both, each including the [n] read the selection needs (host clock).
4. ops.vis_panels against the same sheet composed of torch ops (device events).
Items 2-4: the two sides are called in turn; median and min .. max of ``--reps`` repetitions after 3 warm-up rounds.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"


def alternate_wall(fns, reps, warm=3):
    """ms per call (host clock, synchronised) of every function, called in turn: [(median, min, max)]"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(v), min(v), max(v)) for v in t]


def alternate_events(fns, reps, warm=3):
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
    return [(statistics.median(t), min(t), max(t)) for t in ([a.elapsed_time(b) for a, b in pairs] for pairs in ev)]


def fmt(r):
    return f"{r[0]:9.3f} ms ({r[1]:.3f} .. {r[2]:.3f})"


def run_cfg(seq, out_dir):
    from dns_slam_amd import synthetic
    cfg = synthetic.default_cfg(n_pixels=2000, n_samples_ray=32, n_surface_ray=15, n_frames=5, hash_size=16, voxel_size=0.04,
                                smooth_pts=32, track_pixels=500, track_iters=20)
    cam = seq.cam
    cfg["cam"] = {**{k: cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy")}, "crop_edge": 0}
    cfg.update({"back_end": {"bound": synthetic.ROOM0_BOUND}, "bound_divisible": 0.32, "scale": 1, "scene": "time_slam", "out_dir": out_dir,
                "sync_method": "strict", "verbose": False, "const_speed_assumption": True, "use_gt_camera": False})
    cfg["mapping"].update({"n_iters": 30, "n_iters_first": 100, "optimize_every_n_frames": 5, "choose_keyframe_every": 5, "vis_every": 0,
                           "mesh_every": 0, "checkpoint_every": 0, "start_optimize_idx": 10, "n_pts_batch": 1 << 16})
    return cfg


def item1(say, reps, tmp):
    from dns_slam_amd import evaluation, synthetic
    from dns_slam_amd.slam import DNS_SLAM
    t0 = time.perf_counter()
    seq = synthetic.SyntheticSequence(n=40, H=480, W=640, fx=500.0, step=0.02)
    say(f"1. 40-frame run at 480 x 640 (frames rendered on the host in {time.perf_counter() - t0:.1f} s, not counted)")
    rows = []
    for r in range(-1, reps):                              # run -1 warms every shape up (first launches, allocator) and is not counted
        torch.manual_seed(max(r, 0))
        np.random.seed(max(r, 0))
        slam = DNS_SLAM(run_cfg(seq, os.path.join(tmp, f"run{r}")), device=DEV, dataset=seq)
        torch.cuda.synchronize()
        slam.run()
        torch.cuda.synchronize()
        t = slam.timing
        ate = evaluation.evaluate_ate(slam.gt_c2w_list, slam.estimate_c2w_list)["absolute_translational_error.rmse"]
        if r < 0:
            continue
        other = t["total"] - t["track"] - t["map"]
        rows.append((t["total"], t["track"], t["map"], other, ate))
        say(f"   run {r}: total {t['total']:.2f} s = tracking {t['track']:.2f} + mapping {t['map']:.2f} + everything else {other:.2f} "
            f"({100 * other / t['total']:.1f} %); ATE rmse {ate:.4f} m; {len(slam.keyframe_list)} keyframes, {len(slam.events)} events")
    med = [statistics.median(c) for c in zip(*rows)]
    say(f"   median of {reps}: total {med[0]:.2f} s, tracking {med[1]:.2f}, mapping {med[2]:.2f}, everything else {med[3]:.2f} s "
        f"({100 * med[3] / med[0]:.1f} %), ATE rmse {med[4]:.4f} m")


def item2(say, reps):
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.keyframes import KeyframeBank
    from dns_slam_amd.mapping import Mapper
    H, W, K = 680, 1200, 50
    cam = synthetic.camera(H=H, W=W, fx=600.0, fy=600.0)
    bound = synthetic.load_bound(synthetic.ROOM0_BOUND)
    cfg = synthetic.default_cfg(n_pixels=200, n_frames=7, hash_size=12, voxel_size=0.16, smooth_pts=8)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    g = torch.Generator().manual_seed(0)
    color, depth = torch.rand(H, W, 3, generator=g), torch.rand(H, W, generator=g) * 5
    label = torch.randint(0, 8, (H, W), generator=g).float()
    pose = synthetic.make_pose(0.3)
    mappers = []
    for storage in ("device", "host"):
        m = Mapper(cfg, dec, bound, cam, device=DEV)
        if storage == "device":
            bank = KeyframeBank(K, H, W, 8, DEV)
            for k in range(K):
                bank.add(k, color, depth, label, pose, pose)
            m.keyframe_dict, m.keyframe_list = bank.as_list(), bank.frame_idx
        else:
            for k in range(K):
                m.keyframe_list.append(k)
                m.keyframe_dict.append({"gt_color": color.clone(), "gt_depth": depth.clone(), "gt_label": label.clone(),
                                        "gt_c2w": pose.clone(), "est_c2w": pose.clone()})
        m.mapping_mode = "global"
        mappers.append(m)
    cur = (color.to(DEV), depth.to(DEV), label.to(DEV), pose.to(DEV), pose.to(DEV))
    state = {"n": 0, "bytes": 0}

    def call(m):
        def fn():
            np.random.seed(state["n"] // 2)                 # the same picks for the two sides of a round
            state["n"] += 1
            idx, tf, rf = m.set_target_refer_frames(*cur)
            state["targets"] = len(idx)
        return fn

    res = alternate_wall([call(m) for m in mappers], reps)
    per_frame = H * W * 4
    say(f"2. set_target_refer_frames, {K} keyframes at {H} x {W}, n_joint_optimize_frames 7 ({state['targets']} targets in the last call; a "
        f"target's images are {5 * per_frame / 1e6:.1f} MB, its two reference colours {6 * per_frame / 1e6:.1f} MB)")
    say(f"   device bank   {fmt(res[0])}")
    say(f"   host keyframes{fmt(res[1])}   ratio {res[1][0] / res[0][0]:.2f}")


def item3(say, reps):
    from dns_slam_amd import ops, synthetic
    cam = synthetic.camera(H=680, W=1200, fx=600.0, fy=600.0)
    H, W, fx, fy, cx, cy = (cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy"))
    g = torch.Generator().manual_seed(1)
    pts = ((torch.rand(1600, 3, generator=g) - 0.5) * 6).to(DEV)
    say("3. keyframe overlap, 1600 points, poses on the device, the [n] read included")
    for n in (50, 400):
        poses = torch.stack([synthetic.make_pose(0.3 + 0.01 * k, center=(0.0, 0.0, 0.0)) for k in range(n)]).to(DEV)

        def torch_block():
            w2c = torch.linalg.inv(poses)
            c = torch.einsum("kij,nj->kni", w2c[:, :3, :3], pts) + w2c[:, None, :3, 3]
            x, y, zc = -c[..., 0], c[..., 1], c[..., 2]
            z = zc + 1e-5
            u, v = (fx * x + cx * zc) / z, (fy * y + cy * zc) / z
            inside = (u < W - 10) & (u > 10) & (v < H - 10) & (v > 10) & (z < 0)
            return inside.float().mean(dim=1).cpu().numpy()

        def kernel():
            return ops.keyframe_overlap(pts, poses, H, W, fx, fy, cx, cy).cpu().numpy() / 1600.0

        a, b = torch_block(), kernel()
        res = alternate_wall([kernel, torch_block], reps)
        say(f"   n = {n:3d}: kernel {fmt(res[0])}   torch block {fmt(res[1])}   ratio {res[1][0] / res[0][0]:.2f}   "
            f"(largest difference of the fractions {np.abs(a - b).max():.2e})")


def torch_sheet(gc, ec, gd, ed, gl, el, lut, table, max_label=101.0, gap=8, background=255):
    """ops.vis_panels composed of torch ops (same rules)."""
    H, W = gd.shape

    def scalar(x, vmax):
        t = (x / vmax) * 256.0
        idx = torch.where(t >= 0, torch.where(t >= 256.0, torch.full_like(t, 255.0), t), torch.zeros_like(t)).long()
        idx = torch.where(vmax == 0, torch.zeros_like(idx), idx)
        out = table[idx]
        return torch.where(torch.isfinite(x)[..., None], out, torch.full_like(out, background))

    colour = lambda x: (torch.nan_to_num(x, nan=0.0).clamp(0, 1) * 255.0).to(torch.uint8)
    ok = torch.isfinite(gd) & (gd > 0)
    vmax = torch.where(ok, gd, torch.zeros_like(gd)).max()
    gl, el = lut[gl.long()], lut[el.long()]
    ml = torch.tensor(max_label, device=gd.device)
    rows = [[scalar(gd, vmax), scalar(ed, vmax), scalar((gd - ed).abs(), vmax)],
            [colour(gc), colour(ec), colour((gc - ec).abs())],
            [scalar(gl.float(), ml), scalar(el.float(), ml), scalar((gl - el).abs().float(), ml)]]
    out = torch.full((3 * H + 2 * gap, 3 * W + 2 * gap, 3), background, dtype=torch.uint8, device=gd.device)
    for r in range(3):
        for c in range(3):
            out[r * (H + gap):r * (H + gap) + H, c * (W + gap):c * (W + gap) + W] = rows[r][c]
    return out


def item4(say, reps):
    from dns_slam_amd import ops
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_plasma_lut
    table = torch.as_tensor(gen_plasma_lut.parse_header(os.path.join(ROOT, "dns_slam_amd", "csrc", "plasma_lut.hpp"))).to(DEV)
    lut = (torch.arange(8, dtype=torch.int32) * 10 + 1).to(DEV)
    say("4. frame_vis sheet (bytes written: 27 H W + the gaps; read: 32 H W)")
    for H, W in ((480, 640), (680, 1200)):
        g = torch.Generator().manual_seed(2)
        gc, ec = torch.rand(H, W, 3, generator=g).to(DEV), torch.rand(H, W, 3, generator=g).to(DEV)
        gd = (torch.rand(H, W, generator=g) * 5).to(DEV)
        ed = gd + 0.1
        gl, el = torch.randint(0, 8, (H, W), generator=g).to(DEV), torch.randint(0, 8, (H, W), generator=g).to(DEV)
        a = ops.vis_panels(gc, ec, gd, ed, gl, el, label_lut=lut)[0]
        b = torch_sheet(gc, ec, gd, ed, gl, el, lut, table)
        same = bool(torch.equal(a, b))
        res = alternate_events([lambda: ops.vis_panels(gc, ec, gd, ed, gl, el, label_lut=lut), lambda: torch_sheet(gc, ec, gd, ed, gl, el, lut, table)], reps)
        moved = (27 + 32) * H * W
        say(f"   {H} x {W}: kernel {fmt(res[0])} ({moved / res[0][0] / 1e9:.2f} TB/s of the compulsory bytes)   torch ops {fmt(res[1])}   "
            f"ratio {res[1][0] / res[0][0]:.1f}   sheets equal: {same}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--items", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_time.txt"))
    ap.add_argument("--tmp", help="folder for the runs' outputs (default: a temporary one)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_slam: no GPU visible; a timing on the CPU says nothing about the device")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/time_slam.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    items = {int(v) for v in a.items.split(",")}
    if 3 in items:
        item3(say, a.reps)
    if 4 in items:
        item4(say, a.reps)
    if 2 in items:
        item2(say, max(3, a.reps // 4))
    if 1 in items:
        import tempfile
        item1(say, a.run_reps, a.tmp or tempfile.mkdtemp(prefix="time_slam_"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
