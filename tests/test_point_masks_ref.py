"""CPU: the torch restatement of the reference's point_masks (tests/point_masks_ref.py) against cases worked out by hand, its
partition property, its dependence on the chunk length, and its float32 run against its float64 run."""
import functools

import pytest
import torch

import point_masks_ref as R


def test_hand_made_cases():
    pts, w2c, cam, H, W, depths, md, expected = R.hand_made()
    for dtype in (torch.float32, torch.float64):
        for mode, kw in R.hand_made_modes(depths, md).items():
            s, f, u, _ = R.point_masks_ref(pts, w2c, cam, H, W, dtype=dtype, **kw)
            assert R.classes(s, f).tolist() == expected[mode], (mode, dtype)
            assert u.tolist() == [c == 0 for c in expected[mode]]


def test_chunk_length_changes_the_forecast_mask():
    """torch.max(depth_sample) runs over the chunk: the point behind the wall is forecast only when its chunk also holds a point
    that samples the deep patch."""
    pts, w2c, cam, H, W, depths, md, _ = R.hand_made()
    s7, f7, _, _ = R.point_masks_ref(pts, w2c, cam, H, W, depths=depths, chunk=7)
    s3, f3, _, _ = R.point_masks_ref(pts, w2c, cam, H, W, depths=depths, chunk=3)
    assert (s7 == s3).all()                               # seen does not depend on the chunk
    assert bool(f7[2]) and not bool(f3[2]) and (f7 != f3).sum() == 1
    s9, f9, _, _ = R.point_masks_ref(pts, w2c, cam, H, W, depths=depths, chunk=9)     # a chunk longer than P is one chunk
    assert (f9 == f7).all() and (s9 == s7).all()


@functools.lru_cache(None)
def _scene():
    from dns_slam_amd import synthetic
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(6, cam=cam, seed=3)
    pts = R.scene_points(bound, 40000)
    w2c = torch.inverse(frames["est_c2w"]).float()
    dep = frames["gt_depth"].float()
    return pts, w2c, cam, dep, dep.reshape(6, -1).max(1).values


MODES = {"frustum": lambda dep, md: {}, "limit": lambda dep, md: {"max_depth": md},
         "test": lambda dep, md: {"depths": dep, "chunk": 8192}, "test_partial": lambda dep, md: {"depths": dep, "chunk": 7001}}


@pytest.mark.parametrize("mode", list(MODES))
def test_partition_and_fp32_against_fp64(mode):
    pts, w2c, cam, dep, md = _scene()
    kw = MODES[mode](dep, md)
    s, f, u, near = R.point_masks_ref(pts, w2c, cam, 60, 80, **kw)
    assert (s.int() + f.int() + u.int() == 1).all()       # disjoint, and they cover every point
    assert s.any() and f.any() and u.any()
    s64, f64, u64, _ = R.point_masks_ref(pts, w2c, cam, 60, 80, dtype=torch.float64, **kw)
    assert (s64.int() + f64.int() + u64.int() == 1).all()
    bad = (s != s64) | (f != f64)
    assert int((bad & ~near).sum()) == 0
    assert int(near.sum()) <= 1e-3 * pts.shape[0]          # the flag stays inside what a comparison may leave out


def test_depth_test_removes_some_seen_points():
    pts, w2c, cam, dep, md = _scene()
    sl = R.point_masks_ref(pts, w2c, cam, 60, 80, max_depth=md)[0]
    st = R.point_masks_ref(pts, w2c, cam, 60, 80, depths=dep, chunk=8192)[0]
    assert not (st & ~sl).any()                           # here the depth test only removes: ds + 0.1 <= max + 0.1 < 1.2 max
    assert 0 < int(st.sum()) < int(sl.sum())


def test_no_keyframes_and_no_points():
    pts, w2c, cam, dep, md = _scene()
    s, f, u, near = R.point_masks_ref(pts[:10], w2c[:0], cam, 60, 80)
    assert not s.any() and not f.any() and u.all() and not near.any()
    assert all(t.shape == (0,) for t in R.point_masks_ref(pts[:0], w2c, cam, 60, 80, depths=dep, chunk=5))
