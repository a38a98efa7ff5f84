"""GPU: ops.keyframe_overlap (csrc/keyframes.hip) against its numpy restatement (tests/keyframe_overlap_ref.py).  Both sides compute
the same float64 operations in the same order, so the counts are EQUAL, at the image borders too; and Mapper's
keyframe_selection_overlap picks the same keyframes with and without the bank's scorer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_overlap_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAM = kr.CAM


def _gpu(points, poses, **kw):
    from dns_slam_amd import ops
    cam = dict(CAM)
    cam.update(kw)
    out = ops.keyframe_overlap(torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32)).reshape(-1, 3).to(DEV),
                               torch.as_tensor(np.ascontiguousarray(poses, dtype=np.float32)).reshape(-1, 4, 4).to(DEV), **cam)
    assert out.dtype == torch.int32 and out.is_cuda
    return out.cpu().numpy()


def _ref(points, poses, **kw):
    cam = dict(CAM)
    cam.update(kw)
    return kr.overlap_counts(points, poses, **cam)


@pytest.mark.parametrize("n", [1, 2, 65])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1600])
def test_counts_equal_the_restatement(P, n):
    pts, poses = kr.box_points(P, 100 + P, half=2.5), kr.circle_poses(n)
    want = _ref(pts, poses)
    got = _gpu(pts, poses)
    print("P", P, "n", n, "sum", int(want.sum()))
    assert np.array_equal(got, want)
    if P >= 257:
        assert want.sum() > 0


def _step(x, k):
    """x fp32 moved by k float32 steps."""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def _border_points(pose, target_u, target_v):
    """World points whose projection by `pose` lands on (target_u, target_v) up to the rounding of the fp32 coordinates, and the
    points a few float32 steps of each coordinate around them."""
    cam = CAM
    zc = -1.5
    ze = zc + 1e-5
    xc = -(target_u * ze - cam["cx"] * zc) / cam["fx"]               # u = (fx (-x) + cx zc) / ze with the flip undone
    yc = (target_v * ze - cam["cy"] * zc) / cam["fy"]
    world = (pose.astype(np.float64) @ np.array([xc, yc, zc, 1.0]))[:3].astype(np.float32)
    out = []
    for axis in range(3):
        for k in range(-4, 5):
            p = world.copy()
            p[axis] = _step(p[axis], k)
            out.append(p)
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("pose_id", ["identity", "circle"])
def test_points_within_float32_steps_of_the_four_borders(pose_id):
    pose = np.eye(4, dtype=np.float32) if pose_id == "identity" else kr.circle_poses(5)[3]
    edge, H, W = 10, CAM["H"], CAM["W"]
    mid_u, mid_v = W / 2.0, H / 2.0
    groups = {"left": (edge, mid_v), "right": (W - edge, mid_v), "top": (mid_u, edge), "bottom": (mid_u, H - edge)}
    flips = 0
    for name, (tu, tv) in groups.items():
        pts = _border_points(pose, float(tu), float(tv))
        u, v, _, ok = kr.project(pts, pose, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
        assert ok
        moved = u if name in ("left", "right") else v
        target = np.float32(tu if name in ("left", "right") else tv)
        steps = np.abs(moved.astype(np.float32) - target) / np.spacing(target)
        assert steps.min() <= 4, f"{name}: no point within 4 float32 steps of the border ({steps.min()})"
        # every point on its own: a count of 0 or 1 per launch is the point's inside flag
        want = np.array([_ref(p[None], pose[None])[0] for p in pts])
        got = np.array([_gpu(p[None], pose[None])[0] for p in pts])
        print(pose_id, name, "inside flags", want.tolist())
        assert np.array_equal(got, want)
        flips += int(0 < want.sum() < len(pts))
        assert np.array_equal(_gpu(pts, pose[None]), _ref(pts, pose[None]))
    assert flips >= 2, "the sweeps must cross borders"


def test_all_points_behind_the_camera():
    pose = np.eye(4, dtype=np.float32)[None]
    pts = kr.box_points(300, 1, half=1.0) + np.float32([0, 0, 3.0])          # z > 0: behind a camera that looks along -z
    assert _ref(pts, pose).tolist() == [0]
    assert _gpu(pts, pose).tolist() == [0]


def test_z_plus_eps_changing_sign():
    pose = np.eye(4, dtype=np.float32)[None]
    z = np.float32(-1e-5) * (1.0 + np.linspace(-2e-3, 2e-3, 81, dtype=np.float32))
    z = np.concatenate([z, np.float32([-5e-6, -2e-5, -1e-3, -1e-2])])
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1).astype(np.float32)
    ze = kr.project(pts, pose[0], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])[2]
    assert (ze > 0).any() and (ze < 0).any()
    want = np.array([_ref(p[None], pose)[0] for p in pts])
    got = np.array([_gpu(p[None], pose)[0] for p in pts])
    assert np.array_equal(got, want) and want.sum() >= 1 and want[-4] == 0 and want[-2] == 1


def test_non_finite_and_singular_inputs_count_nothing():
    poses = kr.circle_poses(4).copy()
    pts = kr.box_points(257, 3, half=2.5)
    clean = _ref(pts, poses)
    assert clean.sum() > 0
    bad = pts.copy()
    bad[5, 1], bad[70, 0], bad[200, 2] = np.nan, np.inf, -np.inf
    want = _ref(bad, poses)
    assert np.array_equal(_gpu(bad, poses), want) and (want <= clean).all()
    poses[1, 0, 3] = np.nan                     # a NaN pose
    poses[2, 2] = poses[2, 1]                   # a singular pose
    want = _ref(pts, poses)
    assert want[1] == 0 and want[2] == 0 and want[0] == clean[0] and want[3] == clean[3]
    assert np.array_equal(_gpu(pts, poses), want)
    assert _gpu(np.full((64, 3), np.nan, np.float32), poses).tolist() == [0, 0, 0, 0]


def test_a_non_rigid_pose():
    rng = np.random.default_rng(8)
    poses = kr.circle_poses(3).astype(np.float64)
    poses[:, :3, :3] *= rng.uniform(0.5, 1.5, size=(3, 1, 3))          # scaled and sheared axes
    poses[:, 3] = [[0.01, -0.02, 0.03, 1.1], [0, 0, 0.05, 0.9], [0.02, 0, 0, 1.0]]      # a projective bottom row
    poses = poses.astype(np.float32)
    pts = kr.box_points(1600, 9, half=2.5)
    want = _ref(pts, poses)
    assert want.sum() > 0
    assert np.array_equal(_gpu(pts, poses), want)


def test_two_calls_give_the_same_bits_and_other_cameras():
    pts, poses = kr.box_points(1600, 4, half=2.5), kr.circle_poses(65)
    a, b = _gpu(pts, poses), _gpu(pts, poses)
    assert np.array_equal(a, b)
    other = dict(H=37, W=91, fx=61.3, fy=58.9, cx=44.2, cy=17.7, edge=3, eps=1e-4)
    assert np.array_equal(_gpu(pts, poses, **other), _ref(pts, poses, **other))


def test_empty_inputs():
    from dns_slam_amd import ops
    poses = torch.as_tensor(kr.circle_poses(3)).to(DEV)
    out = ops.keyframe_overlap(torch.zeros(0, 3, device=DEV), poses, **CAM)
    assert out.shape == (3,) and out.dtype == torch.int32 and out.tolist() == [0, 0, 0]
    out = ops.keyframe_overlap(torch.zeros(5, 3, device=DEV), torch.zeros(0, 4, 4, device=DEV), **CAM)
    assert out.shape == (0,) and out.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.keyframe_overlap(torch.zeros(5, 3), poses, **CAM)


def test_mapper_selection_is_the_same_with_and_without_the_scorer():
    """Mapper.keyframe_selection_overlap under the same seeds, with overlap_scorer unset (the torch block, float32) and set (the
    bank's scorer: ops.keyframe_overlap, count / P in float64).  The points the mapper draws are recorded and held to the margin
    filter: the comparison runs under the first seed whose points have none within 0.01 px of a border in either spelling, so the
    two arithmetics must count alike."""
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.keyframes import KeyframeBank
    from dns_slam_amd.mapping import Mapper
    import slam_synth
    seq = slam_synth.SynthSequence(n=6)
    cam = seq.cam
    cfg = synthetic.default_cfg(n_pixels=96, n_samples_ray=16, n_surface_ray=9, hash_size=12, voxel_size=0.16, smooth_pts=8)
    dec = Decoder(cfg["model"], seq.bound, n_class=8).to(DEV)
    mapper = Mapper(cfg, dec, seq.bound, cam, device=DEV)
    bank = KeyframeBank(5, cam["H"], cam["W"], 8, DEV)
    for i in range(5):
        _, color, depth, label, c2w = seq[i]
        bank.add(i, color, depth, label, c2w, c2w)
    _, color, depth, _, c2w = seq[5]
    color, depth = color.to(DEV), depth.to(DEV)
    kfs = bank.as_list()
    seen = {}
    scorer = bank.overlap_scorer(cam)

    def recording(pts, keyframe_dict):
        seen["pts"] = pts.detach().cpu().numpy()
        return scorer(pts, keyframe_dict)

    # the input: the first seed whose drawn points ARE their own margin-filtered form (none within 0.01 px of a border in either
    # spelling of the rule -- a property of the points alone, judged by the two restatements, not by the code under test)
    P = 50 * 16
    cam6 = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    poses = bank.est_c2w.cpu().numpy()

    def select(fn, seed):
        mapper.overlap_scorer = fn
        torch.manual_seed(seed)
        np.random.seed(6)
        picked = mapper.keyframe_selection_overlap(color, depth, c2w, kfs, 3, pixels=50, th=0.05)
        return picked, np.asarray(mapper.last_overlap_percent, dtype=np.float64)

    for seed in range(21, 61):
        kernel_pick, kernel_percent = select(recording, seed)
        if kr.margin_filter(seen["pts"], poses, *cam6)[1] == 0:
            break
    else:
        raise AssertionError("40 seeds, each with a drawn point within 0.01 px of a border")
    print("seed", seed, "picked", kernel_pick, "counts", np.rint(kernel_percent * P).tolist())
    assert seen["pts"].shape == (P, 3)
    torch_pick, torch_percent = select(None, seed)
    assert np.array_equal(np.rint(torch_percent * P), np.rint(kernel_percent * P))
    assert kernel_pick == torch_pick and len(kernel_pick) >= 1
    assert np.array_equal(np.rint(kernel_percent * P).astype(np.int64), kr.overlap_counts(seen["pts"], poses, *cam6))
