"""CPU: the numpy restatement of the keyframe TSDF fusion (tests/tsdf_ref.py) -- the definition csrc/tsdf.hip is held to in
tests/test_gpu_bound.py -- against a hand-worked case and its own float64 evaluation."""
import functools

import numpy as np

import tsdf_ref as R

CAM = {"fx": 60.0, "fy": 60.0, "cx": 39.5, "cy": 29.5}
COARSE = (4.0 / 128.0, 0.16)


@functools.lru_cache(None)
def _scene():
    from dns_slam_amd import synthetic
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(6, cam=cam, seed=3)                 # tests/test_gpu_mesh.py::_scene
    return cam, {k: v.numpy() for k, v in frames.items() if hasattr(v, "numpy")}


@functools.lru_cache(None)
def _duplicate_case(dtype):
    cam, frames = _scene()
    c2w, depths = R.scene_keyframes(frames, (0, 1, 2))
    E, P, _ = R.poses(c2w)
    return R.fuse(depths, E, P, cam, *COARSE, dtype=np.dtype(dtype).type)


def test_plane_at_depth_one():
    """One frame with the identity pose (Open3D's convention: looking along +z) facing the plane z = 1."""
    H, W = 60, 80
    vl, tr = COARSE
    depths = np.ones((1, H, W), np.float32)
    E = np.eye(4)[None]
    r = R.fuse(depths, E, E, CAM, vl, tr)
    assert set(np.unique(r["weight"]).tolist()) <= {0.0, 1.0} and r["weight"].max() == 1.0
    # the units are exactly those within trunc of the sampled points
    L = 16 * vl
    want = set()
    for i in range(0, H, 4):
        for j in range(0, W, 4):
            p = np.array([(j - CAM["cx"]) * 1.0 / CAM["fx"], (i - CAM["cy"]) * 1.0 / CAM["fy"], 1.0])
            lo, hi = np.floor((p - tr) / L).astype(int), np.floor((p + tr) / L).astype(int)
            for ux in range(lo[0], hi[0] + 1):
                for uy in range(lo[1], hi[1] + 1):
                    for uz in range(lo[2], hi[2] + 1):
                        want.add((ux, uy, uz))
    assert set(map(tuple, r["units"].tolist())) == want
    assert np.array_equal(r["units"], np.array(sorted(want), np.int32))
    v = R.vertices(r["units"], r["tsdf"], r["weight"], vl)
    assert len(v) > 100
    assert np.abs(v[:, 2] - 1.0).max() < vl, np.abs(v[:, 2] - 1.0).max()
    assert len(np.unique(v, axis=0)) == len(v)


def test_duplicate_keyframe_averages():
    r = _duplicate_case("float32")
    assert r["weight"].max() == 2.0
    n_frames = np.unique(r["pairs"][:, :3], axis=0, return_counts=True)[1]
    share = float((n_frames > 1).mean())
    print(f"units {len(r['units'])}, pairs {len(r['pairs'])}, touched twice {share:.3f}")
    assert share >= 0.25
    # the running average: where both frames updated a voxel its value lies between -1 and 1 and the weight is 2
    both = r["weight"] == 2.0
    assert both.sum() > 1000 and np.abs(r["tsdf"][both]).max() <= 1.0


def test_no_vertex_from_an_incomplete_cube():
    r = _duplicate_case("float32")
    vl = COARSE[0]
    v, cube = R.vertices(r["units"], r["tsdf"], r["weight"], vl, with_cubes=True)
    assert len(v) > 50000
    # every vertex lies on a lattice edge; the four cubes around that edge are looked up again from the tiles, by position
    T = R.tiles(r["units"], r["tsdf"], r["weight"])
    index = {tuple(u): b for b, u in enumerate(r["units"].tolist())}
    g = (v - 0.5 * vl) / vl
    axis = np.argmax(np.abs(g - np.rint(g)) > 1e-9, axis=1)
    on_node = ~(np.abs(g - np.rint(g)) > 1e-9).any(1)                               # a zero exactly at voxel a: the axis is unknown
    rng = np.random.default_rng(0)
    for n in rng.choice(len(v), 2000, replace=False):
        if on_node[n]:
            continue
        e = axis[n]
        a = np.rint(g[n]).astype(int)
        a[e] = int(np.floor(g[n][e]))
        u, loc = a // 16, a % 16
        b = index[tuple(u)]
        ok = False
        others = [x for x in range(3) if x != e]
        for o1 in (0, 1):
            for o2 in (0, 1):
                q = loc + 1
                q[others[0]] -= o1
                q[others[1]] -= o2
                ok |= bool(~np.isnan(T[b, q[0]:q[0] + 2, q[1]:q[1] + 2, q[2]:q[2] + 2]).all())
        assert ok, (n, v[n])
        assert not np.isnan(T[b, loc[0] + 1, loc[1] + 1, loc[2] + 1])


def test_float32_equals_float64_away_from_near_voxels():
    r32, r64 = _duplicate_case("float32"), _duplicate_case("float64")
    assert np.array_equal(r32["units"], r64["units"]) and np.array_equal(r32["pairs"], r64["pairs"])
    near = r64["near"]
    share = near.sum() / r64["updates"]
    print(f"flagged {int(near.sum())} of {r64['updates']} updates ({share:.4f})")
    assert share < 0.02
    assert np.array_equal(r32["weight"][~near], r64["weight"][~near].astype(np.float32))
    # z_cam errs by a few ulp of ~4 m (4e-6), the multiplier is below 1.5, trunc is 0.16: 1e-4 of tsdf at the very most
    same = ~near & (r32["weight"] == r64["weight"])
    assert np.abs(r32["tsdf"][same] - r64["tsdf"][same]).max() < 1e-4
