"""GPU: slam.DNS_SLAM.run on a synthetic sequence (tests/slam_synth.py): eight frames of 48 x 64, a few tracker and mapper
iterations, tens of rays.

Run A: the example configuration of tests/test_slam_schedule.py -- events, trajectory invariants, keyframe bank, logs, checkpoints,
mesh and frame_vis sheets.  Run B: no outputs; the driver's trajectory against the same loop spelled here from public
Tracker.track_frame / Mapper.optimize calls with HOST keyframes (the reference's storage), which is run twice from the same seeds:
the driver may differ from it by at most 4 x the largest difference between those two runs (equality, if the path is deterministic
at this size; the factor is there because one pair of runs samples the float-atomic spread thinly).

Run B's size is chosen so that the path IS deterministic.  Measured on an MI355X with three tracker iterations and bundle adjustment
on (nine runs each of the loop and of driver variants, device and host keyframes, kernel and torch overlap block): most pairs of runs
agree to 0 .. 2e-8, but a run in three (plain) or nine (stem) leaves its cluster by 1.8e-6 / 1.1e-5 -- driver and loop alike, the
host-keyframe torch-block driver, which IS the loop, included.  The cause is a pose entry that rounds to the neighbouring float32
(5.96e-8 at frame 3, the first frame whose pose the float-atomic sums of the scene gradients reach through Adam's second step) and
is then doubled from frame to frame by the constant-speed rule: 6e-8 x 2^5 = 1.9e-6.  A bound of 4 x one pair's spread fails whenever
the pair has no such event and the driver has one.  So run B tracks with TWO iterations (Adam's first step is lr g / (|g| + eps): a relative
error of 1e-7 in g moves it by 1e-10 of lr, far below a float32 step of the pose; the keep-best pose is the initial pose or that step) and maps with start_optimize_idx beyond the sequence (the mapper leaves the
poses alone): the trajectory then depends on the scene only through signs and the keep-best comparison, spread and difference are 0,
and a driver that orders frames, keyframes or reference views differently from the loop still lands on other poses.  Run C keeps
bundle adjustment on and three tracker iterations and holds the driver to the loop within a bound derived from that event."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slam_synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


# ------------------------------------------------------------------------------------------------------------------------- run A
@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    from dns_slam_amd.slam import DNS_SLAM
    out = str(tmp_path_factory.mktemp("run_a"))
    seq = slam_synth.SynthSequence(n=8)
    cfg = slam_synth.run_cfg(seq, out)
    _seed(3)
    slam = DNS_SLAM(cfg, device=DEV, dataset=seq)
    seen = []
    _seed(4)
    slam.run(on_event=lambda ev, payload: seen.append((ev, payload)))
    return slam, seq, cfg, seen


def test_run_a_events_are_the_schedule(run_a):
    from dns_slam_amd.slam import schedule
    slam, seq, cfg, seen = run_a
    want = schedule(8, cfg)
    assert slam.events == want and [ev for ev, _ in seen] == want
    assert want[:3] == [("keyframe", 0), ("map", 1, 6, ("overlap",)), ("vis", 1)] and want[-1] == ("checkpoint", "model.pt")
    maps = [p for ev, p in seen if ev[0] == "map"]
    assert len(maps) == 4 and all({"loss_camera_tensor", "p_loss", "d_loss"} <= set(p) for p in maps)


def test_run_a_trajectory(run_a):
    from dns_slam_amd.slam import pose_init
    slam, seq, cfg, seen = run_a
    est, gt = slam.estimate_c2w_list, slam.gt_c2w_list
    assert tuple(est.shape) == (8, 4, 4) and not est.is_cuda and not gt.is_cuda
    for i in range(8):
        assert torch.equal(gt[i], seq[i][4].float())
    assert torch.equal(est[0], gt[0]) and torch.equal(est[1], gt[1])
    assert bool(torch.isfinite(est).all())
    assert torch.equal(est[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(8, 4))
    tracks = [(ev, p) for ev, p in seen if ev[0] == "track"]
    assert [ev[1] for ev, _ in tracks] == [2, 3, 4, 5, 6, 7]
    # the estimates as they stood when frame idx was tracked: a mapped frame's estimate is refined AFTER its own tracking and BEFORE
    # the next frame's, so the final list is the one the next frame saw
    for ev, p in tracks:
        idx = ev[1]
        assert torch.equal(p["init_c2w"], pose_init(est[idx - 1], est[idx - 2], idx)), idx
        assert p["camera_tensor"].shape == (7,) and bool(torch.isfinite(p["loss"]))
    err = (est[:, :3, 3] - gt[:, :3, 3]).norm(dim=1)
    print("run A translation error per frame", [round(float(e), 4) for e in err])
    assert float(err.max()) < 0.25                                         # a few iterations do not wander off


def test_run_a_keyframes_and_bank(run_a):
    slam, seq, cfg, seen = run_a
    assert slam.keyframe_list == [0, 3, 6] and slam.mapper.keyframe_list is slam.keyframe_list
    assert len(slam.bank) == 3 and slam.bank.capacity == 3 and slam.mapper.keyframe_dict is slam.bank.as_list()
    for i, kf in enumerate(slam.keyframe_dict):
        assert set(kf) == {"gt_color", "gt_depth", "gt_label", "gt_c2w", "est_c2w"}
        for key in kf:
            assert kf[key].is_cuda and kf[key].data_ptr() == getattr(slam.bank, key)[i].data_ptr()
            assert torch.equal(kf[key], getattr(slam.bank, key)[i])        # a view of the storage (run C: optimize's rebind lands in it)
        f = slam.keyframe_list[i]
        assert torch.equal(kf["gt_color"].cpu(), seq[f][1]) and torch.equal(kf["gt_c2w"].cpu(), seq[f][4].float())
        assert slam.bank.present[i].cpu().tolist() == [bool((seq[f][3] == c).any()) for c in range(8)]
    assert torch.equal(slam.keyframe_dict[0]["est_c2w"].cpu(), seq[0][4].float())
    assert (slam.mapper.overlap_scorer is not None) == slam.overlap_kernel
    # Mapper.optimize REBINDS kf["est_c2w"] after bundle adjustment: the assignment lands in the bank's table, the dict keeps the view
    kf, old = slam.keyframe_dict[1], slam.keyframe_dict[1]["est_c2w"].clone()
    new = old.clone()
    new[0, 3] += 0.5
    kf["est_c2w"] = new.clone()
    assert torch.equal(slam.bank.est_c2w[1], new) and kf["est_c2w"].data_ptr() == slam.bank.est_c2w[1].data_ptr()
    kf["est_c2w"] = old
    assert torch.equal(slam.bank.est_c2w[1], old)


def test_run_a_files(run_a):
    from dns_slam_amd import evaluation
    from dns_slam_amd.checkpoint import Checkpoint
    from dns_slam_amd.decoder import Decoder
    slam, seq, cfg, seen = run_a
    out = slam.out_dir
    assert len(open(os.path.join(out, "output_front.txt")).read().splitlines()) == 6
    back = open(os.path.join(out, "output_back_fine.txt")).read().splitlines()
    assert len(back) == 4 and all("Current frame:" in line and "ATE:" in line for line in back)
    H, W = seq.cam["H"], seq.cam["W"]
    for idx in (1, 3, 6, 7):
        raw = open(os.path.join(out, f"{idx:05d}.png"), "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n"
        assert (int.from_bytes(raw[16:20], "big"), int.from_bytes(raw[20:24], "big")) == (3 * W + 16, 3 * H + 16)
    for name, idx, n_kf in (("model_3.pt", 3, 2), ("model_6.pt", 6, 3), ("model.pt", 7, 3)):
        dec = Decoder(cfg["model"], slam.bound, 8).to(DEV)
        rest = Checkpoint(out, device="cpu", decoder=dec).load(name)
        assert {"scene", "idx", "fine_decoders", "keyframe_dict", "keyframe_list", "estimate_c2w_list", "gt_c2w_list"} <= set(rest)
        assert int(rest["idx"]) == idx and list(rest["keyframe_list"]) == [0, 3, 6][:n_kf] and len(rest["keyframe_dict"]) == n_kf
        assert tuple(rest["estimate_c2w_list"].shape) == (8, 4, 4)
        assert all(not v.is_cuda for kf in rest["keyframe_dict"] for v in kf.values())
    assert torch.equal(rest["estimate_c2w_list"], slam.estimate_c2w_list)
    assert torch.equal(dec.pe_fn.grid_fn.params.cpu(), slam.decoder.pe_fn.grid_fn.params.detach().cpu())
    mesh = evaluation.read_ply(os.path.join(out, "mesh", "00006_mesh.ply"))
    assert mesh["verts"].shape[1] == 3 and mesh["faces"].shape[1] == 3
    assert [ev for ev, _ in seen if ev[0] == "mesh"] == [("mesh", 6)]


# ------------------------------------------------------------------------------------------------------------------------- run B
def _hand_loop(seq, cfg, encoder):
    """The reference's two loops under 'strict' from public calls, with host keyframes; returns the trajectory [8,4,4] (the keyframes' final
    est_c2w are left in ``_hand_loop.keyframe_poses``)."""
    from dns_slam_amd.common import get_camera_from_tensor
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.mapping import Mapper
    from dns_slam_amd.slam import pose_init
    from dns_slam_amd.tracking import Tracker
    from dns_slam_amd import synthetic
    m = cfg["mapping"]
    n_img, every, kf_every = len(seq), m["optimize_every_n_frames"], m["choose_keyframe_every"]
    _seed(3)
    bound = synthetic.load_bound(cfg["back_end"]["bound"], cfg["bound_divisible"], cfg["scale"])
    dec = Decoder(cfg["model"], bound, seq.n_class).to(DEV)
    mapper = Mapper(cfg, dec, bound, seq.cam, device=DEV)
    mapper.encoder = encoder
    tracker = Tracker(cfg, dec, bound, seq.cam, device=DEV)
    est = torch.zeros(n_img, 4, 4)
    frame = lambda i: tuple(t.to(DEV) for t in seq[i][1:4]) + (seq[i][4].float(),)
    _seed(4)
    c0, d0, l0, p0 = frame(0)
    est[0] = p0
    mapper.keyframe_list.append(0)
    mapper.keyframe_dict.append({"gt_color": c0.cpu(), "gt_depth": d0.cpu(), "gt_label": l0.cpu(), "gt_c2w": p0, "est_c2w": p0.clone()})
    est[1] = seq[1][4].float()
    refer_color = pre_color = None
    refer_c2w = None
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    for idx in range(1, n_img):
        color, depth, label, gt = frame(idx)
        if idx >= 2:
            if every == 1:
                refer_color, refer_c2w = pre_color, est[idx - 1].clone()
            init = pose_init(est[idx - 1], est[idx - 2], idx)
            features = refer = None
            if encoder is not None:
                features = encoder(torch.stack((refer_color, color), 0)[None])
                refer = {"est_w2c": torch.stack((torch.inverse(refer_c2w), torch.inverse(init))).to(DEV), "follow": (False, True)}
            cam7, _ = tracker.track_frame({"gt_color": color, "gt_depth": depth, "gt_label": label}, init, features=features,
                                          refer_frames=refer)
            est[idx] = torch.cat([get_camera_from_tensor(cam7.detach().cpu()), bottom], 0)
            pre_color = color
        if idx == 1 or idx % every == 0 or idx == n_img - 1:
            cur = est[idx].clone()
            passes = [(m["n_iters_first"], "overlap")] if idx == 1 else [(m["n_iters"] // 2, "overlap"), (m["n_iters"] // 2, "global")]
            for iters, mode in passes:
                mapper.mapping_mode = mode
                cur, _ = mapper.optimize(iters, idx, color, depth, label, gt.to(DEV), cur)
            if mapper.is_BA:
                est[idx] = cur.detach().cpu()
            if idx == 1:
                refer_color = pre_color = color
                refer_c2w = est[1].clone()
                est[1] = gt
            if (idx % kf_every == 0 or idx == n_img - 2) and idx not in mapper.keyframe_list:
                mapper.keyframe_list.append(idx)
                mapper.keyframe_dict.append({"gt_color": color.cpu(), "gt_depth": depth.cpu(), "gt_label": label.cpu(), "gt_c2w": gt,
                                             "est_c2w": cur.detach().cpu()})
    _hand_loop.keyframe_poses = torch.stack([kf["est_c2w"].detach().cpu().float() for kf in mapper.keyframe_dict])
    return est


@pytest.mark.parametrize("stem", [False, True], ids=["plain", "stem"])
def test_run_b_driver_equals_the_hand_written_loop(stem, tmp_path):
    from dns_slam_amd.encoder import ResNet
    from dns_slam_amd.slam import DNS_SLAM
    seq = slam_synth.SynthSequence(n=8)
    cfg = slam_synth.run_cfg(seq, str(tmp_path), vis_every=0, mesh_every=0, checkpoint_every=0, start_optimize_idx=100)
    cfg["tracking"]["n_iters"] = 2
    encoder = ResNet(seed=2).to(DEV) if stem else None
    a = _hand_loop(seq, cfg, encoder)
    b = _hand_loop(seq, cfg, encoder)
    spread = float((a - b).abs().max())
    _seed(3)
    slam = DNS_SLAM(cfg, device=DEV, dataset=seq, encoder=encoder)
    _seed(4)
    est = slam.run()
    diff = float((est - a).abs().max())
    print(f"run B ({'stem' if stem else 'plain'}): loop spread {spread:.3e}, driver - loop {diff:.3e}")
    assert bool(torch.isfinite(a).all()) and not torch.equal(a[2:], slam.gt_c2w_list[2:])
    assert slam.keyframe_list == [0, 3, 6]
    assert diff <= 4.0 * spread


# ------------------------------------------------------------------------------------------------------------------------- run C
# The largest pose entries of the sequence are translations in [2, 4): one float32 step there is 2^-22 = 2.38e-7.
ULP_POSE = 2.0 ** -22
# Run C's bound.  A run differs from another run of the SAME code by single-step rounding events of pose entries (the float-atomic
# sums of the scene gradients reach a pose through Adam's second and later steps); the earliest can occur at frame 3, the first frame
# mapped with bundle adjustment, and the constant-speed rule pose_init = prev inverse(prev2) prev doubles a difference per frame over
# the 5 frames that follow: 2^5.  Four such events of one step each: 4 x 2^-22 x 2^5 = 3.05e-5.  Nine runs of the loop measured
#  left their cluster by at most 1.8e-6 without and 1.1e-5 with the stem.  A driver that orders frames, picks keyframes
# or builds reference views differently moves poses by whole optimiser steps (BA_cam_lr = 5e-4, cam_lr = 1e-3), 16 times the bound.
RUN_C_BOUND = 4 * ULP_POSE * 2 ** 5


@pytest.mark.parametrize("stem", [False, True], ids=["plain", "stem"])
def test_run_c_bundle_adjustment_on_stays_with_the_loop(stem, tmp_path):
    """Run B's comparison with bundle adjustment ON (start_optimize_idx = 2) and three tracker iterations: the configuration in which
    the device bank, the pose write-through and the kernel scorer matter.  Trajectory AND the keyframes' final poses against the
    host-keyframe loop, inside RUN_C_BOUND (derived above from the float32 step of a pose entry, not from the driver)."""
    from dns_slam_amd.encoder import ResNet
    from dns_slam_amd.slam import DNS_SLAM
    seq = slam_synth.SynthSequence(n=8)
    cfg = slam_synth.run_cfg(seq, str(tmp_path), vis_every=0, mesh_every=0, checkpoint_every=0)
    assert cfg["mapping"]["start_optimize_idx"] == 2 and cfg["tracking"]["n_iters"] == 3
    encoder = ResNet(seed=2).to(DEV) if stem else None
    a = _hand_loop(seq, cfg, encoder)
    kf_a = _hand_loop.keyframe_poses
    _seed(3)
    slam = DNS_SLAM(cfg, device=DEV, dataset=seq, encoder=encoder)
    added = {}
    _seed(4)
    est = slam.run(on_event=lambda ev, p: added.update({ev[1]: slam.bank.est_c2w[len(slam.bank) - 1].cpu().clone()}) if ev[0] == "keyframe" else None)
    diff = float((est - a).abs().max())
    kf_diff = float((slam.bank.est_c2w.cpu() - kf_a).abs().max())
    moved = [f for i, f in enumerate(slam.keyframe_list) if not torch.equal(slam.bank.est_c2w[i].cpu(), added[f])]
    print(f"run C ({'stem' if stem else 'plain'}): driver - loop {diff:.3e}, keyframe poses {kf_diff:.3e}, bound {RUN_C_BOUND:.3e}; "
          f"keyframes whose pose bundle adjustment rebound: {moved}")
    assert slam.keyframe_list == [0, 3, 6] and tuple(kf_a.shape) == (3, 4, 4)
    assert diff <= RUN_C_BOUND and kf_diff <= RUN_C_BOUND
    # Mapper.optimize's rebind kf["est_c2w"] = ... landed in the bank's table: a keyframe's pose is no longer the one add() was given
    assert moved and 0 not in moved
    for i, kf in enumerate(slam.keyframe_dict):
        assert kf["est_c2w"].data_ptr() == slam.bank.est_c2w[i].data_ptr()


def test_use_gt_camera_fills_every_frame(tmp_path):
    """use_gt_camera: no frame is tracked, and estimate_c2w_list / gt_c2w_list hold the ground truth of EVERY frame, mapped or not
    (tracking.py:272-273,369-370), with bundle adjustment off; the mapper still runs on its frames."""
    from dns_slam_amd.slam import DNS_SLAM, schedule
    seq = slam_synth.SynthSequence(n=6)
    cfg = slam_synth.run_cfg(seq, str(tmp_path), vis_every=0, mesh_every=0, checkpoint_every=0, start_optimize_idx=100)
    cfg["use_gt_camera"] = True
    _seed(3)
    slam = DNS_SLAM(cfg, device=DEV, dataset=seq)
    est = slam.run()
    assert slam.events == schedule(6, cfg) and not [e for e in slam.events if e[0] == "track"]
    assert [e[1] for e in slam.events if e[0] == "map"] == [1, 3, 5]
    want = torch.stack([seq[i][4].float() for i in range(6)])
    assert torch.equal(est, want) and torch.equal(slam.gt_c2w_list, want)
