"""CPU: the yardstick of the 2-D evaluation tests (tests/image_metrics_ref.py), the premises of the image pairs the GPU tests use,
and the host functions of dns_slam_amd.evaluation (semantic_metrics, evaluate_ate)."""
import numpy as np
import pytest
import torch

import image_metrics_ref as R


def test_library_window_is_the_fp32_window():
    """The eleven constants the kernels filter with are the bits of the fp32 evaluation of the window formula: on constant images
    a window whose sum differs by one fp32 ulp moves cs by 3e-5."""
    from dns_slam_amd import ops
    assert torch.equal(ops.ms_ssim_window(), R.window())


def test_ms_ssim_ref_identity_symmetry_transposition():
    for name in ("noise05", "affine"):
        p, g = R.case_pair(name, 161, 163)
        v, lv = R.ms_ssim_ref(p, g)
        assert abs(R.ms_ssim_ref(p, p)[0] - 1.0) < 1e-12
        v2, lv2 = R.ms_ssim_ref(g, p)
        assert abs(v - v2) < 1e-12 and float((lv - lv2).abs().max()) < 1e-12
        vt, lvt = R.ms_ssim_ref(p.transpose(0, 1), g.transpose(0, 1))
        assert abs(v - vt) < 1e-12 and float((lv - lvt).abs().max()) < 1e-12


def test_pooled_sizes():
    for chain in ((161, 81, 41, 21, 11), (163, 82, 41, 21, 11), (200, 100, 50, 25, 13), (245, 123, 62, 31, 16)):
        for a, b in zip(chain, chain[1:]):
            assert R.pooled_size(a) == b
            x = torch.zeros(1, 1, a, a)
            assert torch.nn.functional.avg_pool2d(x, 2, padding=a % 2).shape[-1] == b


@pytest.mark.parametrize("size", sorted(set(R.SIZES_CPU + R.SIZES_GPU)))
@pytest.mark.parametrize("name", R.CASES)
def test_case_premise(name, size):
    """Every level term of every pair the GPU tests compare is >= 0.05 in float64 (the clamped case: a term <= -0.05 in every
    channel, so the value is exactly 0), and the fp32 definition stays within 1.5e-5 of float64: the room the 5e-5 bound of the
    GPU tests leaves is for another summation order, not for the definition."""
    p, g = R.case_pair(name, *size)
    v, lv = R.ms_ssim_ref(p, g)
    assert R.premise_holds(name, lv), lv
    v32, lv32 = R.ms_ssim_ref(p, g, torch.float32)
    if name == "inverted":
        assert v == 0.0 and v32 == 0.0
    else:
        assert abs(v - v32) <= 1.5e-5
    assert float((lv - lv32).abs().max()) <= 1.5e-5


def test_uniform_noise_misses_the_premise():
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(161, 163, 3, generator=g), torch.rand(161, 163, 3, generator=g)
    assert not R.premise_holds("noise", R.ms_ssim_ref(a, b)[1])


def _label_cases():
    rng = np.random.default_rng(0)
    gt = rng.integers(0, 8, (37, 53))
    pred = np.where(rng.random((37, 53)) < 0.7, gt, rng.integers(0, 8, (37, 53)))
    yield "random", gt, pred, 8
    p2 = pred.copy()
    p2[p2 == 3] = 4
    yield "gt class never predicted", gt, p2, 8
    g3 = gt.copy()
    g3[g3 == 5] = 1
    yield "predicted class absent from gt", g3, pred, 8
    yield "single class", np.full((37, 53), 2), np.full((37, 53), 2), 8
    yield "single gt class, mixed pred", np.full((37, 53), 2), pred, 8


def test_semantic_metrics_matrix_route_equals_mask_route():
    from dns_slam_amd import evaluation as E
    for what, gt, pred, nc in _label_cases():
        conf, bad = R.confusion_ref(gt, pred, nc)
        assert bad == 0 and conf.sum() == gt.size
        got, want = E.semantic_metrics(conf, bad), R.semantic_metrics_ref(gt, pred)
        for k, v in want.items():
            assert abs(got[k] - v) <= 1e-12, (what, k, got[k], v)
    with pytest.raises(ValueError):
        E.semantic_metrics(conf, 3)
    with pytest.raises(ValueError):
        E.semantic_metrics(np.zeros((3, 4)))


def _trajectory(K=40, seed=0):
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 4, K)
    xyz = np.stack((np.cos(t) * 2, np.sin(1.3 * t), 0.3 * t), 1) + 0.01 * rng.standard_normal((K, 3))
    poses = np.tile(np.eye(4), (K, 1, 1))
    poses[:, :3, 3] = xyz
    return poses


def _motion(seed=1):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q, rng.standard_normal(3)


def test_evaluate_ate_recovers_a_rigid_motion_and_drops_nan_poses():
    from dns_slam_amd import evaluation as E
    gt = _trajectory()
    rot, trans = _motion()
    est = gt.copy()
    est[:, :3, 3] = (gt[:, :3, 3] - trans) @ rot                 # gt = rot est + trans
    r = E.evaluate_ate(torch.from_numpy(gt), torch.from_numpy(est))
    assert r["compared_pose_pairs"] == 40 and r["absolute_translational_error.rmse"] < 1e-12
    assert np.abs(r["rot"] - rot).max() < 1e-12 and np.abs(r["trans"] - trans).max() < 1e-12
    assert set(r) == {"compared_pose_pairs", "rot", "trans"} | {"absolute_translational_error." + k for k in
                                                                ("rmse", "mean", "median", "std", "min", "max")}
    bad = gt.copy()
    bad[7, 1, 2] = np.nan
    bad[11, 0, 3] = np.inf
    est2 = est.copy()
    est2[7, :3, 3] += 5.0                                        # would show in the error if the pair were kept
    r2 = E.evaluate_ate(bad, est2)
    assert r2["compared_pose_pairs"] == 38 and r2["absolute_translational_error.max"] < 1e-12
    r3 = E.evaluate_ate(gt, est, scale=2.0)                      # translations divided by scale: the same rotation, half the offset
    assert np.abs(r3["rot"] - rot).max() < 1e-12 and np.abs(r3["trans"] - trans / 2).max() < 1e-12
    with pytest.raises(ValueError):
        E.evaluate_ate(gt[:1], est[:1])


def test_evaluate_ate_against_ate_ref_and_reflection():
    from dns_slam_amd import evaluation as E
    gt = _trajectory()
    rot, trans = _motion(2)
    est = gt.copy()
    est[:, :3, 3] = (gt[:, :3, 3] - trans) @ rot + 0.05 * np.random.default_rng(3).standard_normal((40, 3))
    r = E.evaluate_ate(gt, est)
    rr, tr, err = R.ate_ref(gt[:, :3, 3], est[:, :3, 3])
    assert np.abs(r["rot"] - rr).max() < 1e-12 and np.abs(r["trans"] - tr).max() < 1e-12
    want = {"rmse": np.sqrt((err ** 2).mean()), "mean": err.mean(), "median": np.median(err), "std": err.std(), "min": err.min(),
            "max": err.max()}
    for k, v in want.items():
        assert abs(r["absolute_translational_error." + k] - v) < 1e-12, k
    mirrored = est.copy()
    mirrored[:, 0, 3] *= -1.0                                    # a reflected point set: the best ORTHOGONAL map is a reflection
    r = E.evaluate_ate(gt, mirrored)
    assert abs(np.linalg.det(r["rot"]) - 1.0) < 1e-12
    rr, _, err = R.ate_ref(gt[:, :3, 3], mirrored[:, :3, 3])
    assert np.abs(r["rot"] - rr).max() < 1e-9 and abs(r["absolute_translational_error.rmse"] - np.sqrt((err ** 2).mean())) < 1e-12
