"""CPU: the float64 restatement of ops.keyframe_overlap (tests/keyframe_overlap_ref.py) against the reference's rule in the
reference's own number formats (float32 inverse and camera coordinates), on points away from the image borders; its adjugate inverse
against numpy's; and wrong rules (non-strict comparison, missing x flip, missing eps) being noticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_overlap_ref as kr  # noqa: E402

CAM = kr.CAM
SEEDS = [0, 1, 2, 3, 4]


def _inputs(seed):
    """1600 points in a box around eight poses on a circle, border points (0.01 px, either spelling) removed: at most 1 %."""
    poses = kr.circle_poses(8)
    pts = kr.box_points(1600, seed)
    kept, removed = kr.margin_filter(pts, poses, **CAM)
    assert removed <= 16, f"seed {seed}: {removed} of 1600 points within 0.01 px of a border"
    return kept, poses


def test_adjugate_inverse_is_the_inverse():
    rng = np.random.default_rng(5)
    for m in list(kr.circle_poses(8)) + [rng.normal(size=(4, 4)).astype(np.float32) for _ in range(8)]:
        w, ok = kr.inverse_rows(m)
        assert ok
        inv = np.linalg.inv(m.astype(np.float64))
        assert np.allclose(w.reshape(3, 4), inv[:3], rtol=1e-9, atol=1e-9 * np.abs(inv).max())


def test_singular_and_non_finite_poses_are_refused():
    m = np.eye(4, dtype=np.float32)
    m[2] = m[1]
    assert not kr.inverse_rows(m)[1]
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = np.nan
    assert not kr.inverse_rows(m)[1]
    pts = kr.box_points(64, 0)
    assert kr.overlap_counts(pts, np.stack([m, np.eye(4, dtype=np.float32)]), **CAM)[0] == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_counts_equal_the_reference_rule(seed):
    pts, poses = _inputs(seed)
    want, _, _ = kr.reference_rule(pts, poses, **CAM)
    got = kr.overlap_counts(pts, poses, **CAM)
    print("counts", got.tolist())
    assert want.sum() > 100 and (want > 0).all(), "the test scene must put points into every view"
    assert np.array_equal(got, want)


def test_wrong_flip_is_noticed():
    pts, poses = _inputs(0)
    want, _, _ = kr.reference_rule(pts, poses, **CAM)
    assert not np.array_equal(kr.overlap_counts(pts, poses, flip=False, **CAM), want)


def test_non_strict_comparison_is_noticed():
    # identity pose, z = -1, eps = 0, fx = 64: u = 64 x + cx exactly; x = -21.5 / 64 puts u ON the left border u = edge = 10
    cam = dict(H=48, W=64, fx=64.0, fy=64.0, cx=31.5, cy=23.5)
    pose = np.eye(4, dtype=np.float32)[None]
    pts = np.array([[-21.5 / 64.0, 0.0, -1.0]], dtype=np.float32)
    u, v, ze, ok = kr.project(pts, pose[0], cam["fx"], cam["fy"], cam["cx"], cam["cy"], eps=0.0)
    assert ok and u[0] == 10.0 and v[0] == 23.5 and ze[0] == -1.0
    assert kr.overlap_counts(pts, pose, eps=0.0, **cam).tolist() == [0]
    assert kr.overlap_counts(pts, pose, eps=0.0, strict=False, **cam).tolist() == [1]
    # the reference's rule (its eps is 1e-5; a point exactly on the border after the fp32 rounding) agrees with the strict form
    inside = kr.overlap_counts(np.array([[0.0, 0.0, -1.0]], dtype=np.float32), pose, **cam)
    assert inside.tolist() == [1] == kr.reference_rule(np.array([[0.0, 0.0, -1.0]], dtype=np.float32), pose, **cam)[0].tolist()


def test_missing_eps_is_noticed():
    # zc = -5e-6: z = zc + 1e-5 > 0 is behind the camera by the rule, in front of it without the eps
    pose = np.eye(4, dtype=np.float32)[None]
    pts = np.array([[0.0, 0.0, -5e-6]], dtype=np.float32)
    want = kr.reference_rule(pts, pose, **CAM)[0]
    assert want.tolist() == [0]
    assert kr.overlap_counts(pts, pose, **CAM).tolist() == [0]
    assert kr.overlap_counts(pts, pose, use_eps=False, **CAM).tolist() == [1]


def test_empty_inputs():
    poses = kr.circle_poses(3)
    assert kr.overlap_counts(np.zeros((0, 3), np.float32), poses, **CAM).tolist() == [0, 0, 0]
    assert kr.overlap_counts(kr.box_points(5, 0), np.zeros((0, 4, 4), np.float32), **CAM).shape == (0,)
