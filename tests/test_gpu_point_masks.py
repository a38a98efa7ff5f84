"""GPU: point masks (csrc/mesh_masks.hip, ops.point_masks) against the torch restatement of the reference's point_masks
(tests/point_masks_ref.py, run on the device), and Mesher's forecast mesh and depth-tested cleaning built on them.

Criterion of the comparisons with the restatement (that of test_gpu_mesh.py::test_keyframe_project_matches_reference_loops): the
kernel projects with dev_project.hpp's expressions and samples the depth bilinearly at (u, v) itself, the restatement multiplies
matrices and goes through grid_sample's normalised coordinates, so the two may disagree where a keyframe puts a point within
rounding distance of a threshold -- the restatement's ``near`` flag -- and nowhere else; at most 1e-3 P points may disagree."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mc_ref
import point_masks_ref as R
import test_gpu_mesh as tgm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_SCENE = 300000


@functools.lru_cache(None)
def _scene():
    """test_gpu_mesh.py's scene and point recipe, and the restatement's answer per mode (computed once, never modified)."""
    bound, cam, frames = tgm._scene(6)
    pts = R.scene_points(bound, P_SCENE, seed=5).to(DEV)
    w2c = torch.inverse(frames["est_c2w"].to(DEV)).float()
    dep = frames["gt_depth"].to(DEV).float().contiguous()
    md = dep.reshape(6, -1).max(1).values
    return {"cam": cam, "H": cam["H"], "W": cam["W"], "pts": pts, "w2c": w2c, "dep": dep, "md": md, "frames": frames}


def _mode_kw(s, mode):
    if mode == "frustum":
        return {}
    if mode == "limit":
        return {"max_depth": s["md"]}
    return {"depths": s["dep"], "chunk": {"test_65536": 65536, "test_1000": 1000, "test_beyond_P": P_SCENE + 7}[mode]}


@functools.lru_cache(None)
def _ref(mode):
    s = _scene()
    seen, fore, unseen, near = R.point_masks_ref(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], **_mode_kw(s, mode))
    return R.classes(seen, fore), near


def _assert_matches(cls, ref, near, P):
    bad = cls != ref
    n_bad, n_far = int(bad.sum()), int((bad & ~near).sum())
    print(f"disagreements {n_bad} of {P} (cap {1e-3 * P:.0f}), of them not flagged near: {n_far}; flagged {int(near.sum())}")
    assert n_far == 0, n_far
    assert n_bad <= 1e-3 * P


@pytest.mark.parametrize("mode", ["frustum", "limit", "test_65536", "test_1000", "test_beyond_P"])
def test_point_masks_match_restatement(mode):
    from dns_slam_amd import ops
    s = _scene()
    ref, near = _ref(mode)
    cls = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], **_mode_kw(s, mode))
    assert cls.dtype == torch.uint8 and cls.shape == (P_SCENE,) and int(cls.max()) <= 2
    _assert_matches(cls, ref, near, P_SCENE)
    for c in (0, 1, 2):
        assert bool((cls == c).any()) and bool((ref == c).any())
    if mode == "test_65536":
        # the depth test removes some, not all, of the depth limit's seen points (on the restatement: 71 384 of 111 824)
        rl = _ref("limit")[0] == 1
        assert 0 < int(((ref == 1) & rl).sum()) < int(rl.sum())
        gl = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], max_depth=s["md"]) == 1
        assert 0 < int(((cls == 1) & gl).sum()) < int(gl.sum())


def test_chunk_lengths_differ():
    """The forecast limit is the chunk's maximum sample: other chunk lengths, another forecast mask; the seen mask is the same."""
    from dns_slam_amd import ops
    s = _scene()
    a = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], depths=s["dep"], chunk=1000)
    b = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], depths=s["dep"], chunk=65536)
    assert bool(((a == 1) == (b == 1)).all()) and bool((a != b).any())
    assert bool(((_ref("test_1000")[0] == 2) != (_ref("test_65536")[0] == 2)).any())


def test_hand_made_cases():
    from dns_slam_amd import ops
    pts, w2c, cam, H, W, depths, md, expected = R.hand_made()
    for mode, kw in R.hand_made_modes(depths.to(DEV), md.to(DEV)).items():
        cls = ops.point_masks(pts.to(DEV), w2c.to(DEV), cam, H, W, **kw)
        assert cls.tolist() == expected[mode], mode


def test_depth_limit_seen_is_keyframe_project():
    from dns_slam_amd import ops
    s = _scene()
    _, seen = ops.keyframe_project(s["pts"], s["w2c"], s["frames"]["gt_label"].to(DEV), s["md"], s["cam"])
    cls = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], max_depth=s["md"])
    assert torch.equal(cls == 1, seen)


def test_point_masks_many_keyframes():
    """600 keyframes (the recipe of test_keyframe_project_many_keyframes): three pose tiles, every mode."""
    from dns_slam_amd import ops
    bound, cam, frames = tgm._scene(3)
    n = 600
    idx = torch.arange(n) % 3
    c2w = frames["est_c2w"][idx].clone()
    c2w[:, :3, 3] += torch.randn(n, 3, generator=torch.Generator().manual_seed(1)) * 0.05
    depth = frames["gt_depth"][idx].to(DEV).float().contiguous()
    g = torch.Generator().manual_seed(2)
    b = bound.float()
    P = 20000
    pts = ((torch.rand(P, 3, generator=g)) * (b[:, 1] - b[:, 0]) + b[:, 0]).to(DEV)
    w2c = torch.inverse(c2w.to(DEV)).float()
    md = depth.reshape(n, -1).max(1).values
    H, W = cam["H"], cam["W"]
    _, kp_seen = ops.keyframe_project(pts, w2c, frames["gt_label"][idx].to(DEV), md, cam)
    for kw in ({}, {"max_depth": md}, {"depths": depth, "chunk": 8192}):
        seen, fore, _, near = R.point_masks_ref(pts, w2c, cam, H, W, **kw)
        cls = ops.point_masks(pts, w2c, cam, H, W, **kw)
        _assert_matches(cls, R.classes(seen, fore), near, P)
        if "max_depth" in kw:
            assert torch.equal(cls == 1, kp_seen)


def test_point_masks_edge_shapes():
    from dns_slam_amd import ops
    s = _scene()
    cam, H, W = s["cam"], s["H"], s["W"]
    pts = s["pts"][:1000]
    for kw in ({}, {"max_depth": s["md"]}, {"depths": s["dep"], "chunk": 256}):
        e = ops.point_masks(pts[:0], s["w2c"], cam, H, W, **kw)
        assert e.shape == (0,) and e.dtype == torch.uint8
    for kw in ({}, {"max_depth": s["md"][:0]}, {"depths": s["dep"][:0], "chunk": 256}):
        z = ops.point_masks(pts, s["w2c"][:0], cam, H, W, **kw)
        assert z.shape == (1000,) and not bool(z.any())
    for chunk in (255, 256, 257, 999, 1000, 1001):
        seen, fore, _, near = R.point_masks_ref(pts, s["w2c"], cam, H, W, depths=s["dep"], chunk=chunk)
        cls = ops.point_masks(pts, s["w2c"], cam, H, W, depths=s["dep"], chunk=chunk)
        assert not bool(near.any())                           # none of these 1000 points is near a threshold: exact equality
        assert torch.equal(cls, R.classes(seen, fore)), chunk


def test_point_masks_repeatable():
    from dns_slam_amd import ops
    s = _scene()
    for kw in ({"depths": s["dep"], "chunk": 1000}, {"max_depth": s["md"]}):
        a = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], **kw)
        b = ops.point_masks(s["pts"], s["w2c"], s["cam"], s["H"], s["W"], **kw)
        assert torch.equal(a, b)


def test_point_masks_refusals():
    from dns_slam_amd import _lib, ops
    s = _scene()
    cam, H, W, w2c, dep, md = s["cam"], s["H"], s["W"], s["w2c"], s["dep"], s["md"]
    pts = s["pts"][:64]
    huge = torch.zeros(1, 3, device=DEV).expand(1 << 31, 3)                 # 2^31 points without their memory
    for args, kw in (((huge, w2c), {}),                                       # P >= 2^31
                     ((pts, w2c), {"depths": dep}),                           # depths without chunk
                     ((pts, w2c), {"depths": dep, "chunk": 0}),               # chunk == 0
                     ((pts, w2c), {"max_depth": md, "depths": dep, "chunk": 8}),
                     ((pts, w2c), {"chunk": 8}),                              # chunk without depths
                     ((pts, w2c), {"max_depth": md[:5]}),                     # shapes
                     ((pts, w2c), {"depths": dep[:5], "chunk": 8}),
                     ((pts, w2c), {"depths": dep[:, :-1], "chunk": 8}),
                     ((pts[:, :2], w2c), {}),
                     ((pts, w2c[:, :3]), {}),
                     ((pts.cpu(), w2c), {})):
        with pytest.raises(ValueError):
            ops.point_masks(*args, cam, H, W, **kw)
    with pytest.raises(ValueError):
        ops.point_masks(pts, w2c, cam, 0, W)
    # the raw C symbol: -1 and a message, nothing launched
    L, p = _lib.lib, _lib.ptr
    intr = (C.c_float * 4)(cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    cls = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr()
    for a in ((p(pts), 1 << 31, p(w2c), 6, None, None, 0, H, W, intr, None, p(cls), st),
              (p(pts), 64, p(w2c), 6, p(md), p(dep), 8, H, W, intr, p(ws), p(cls), st),
              (p(pts), 64, p(w2c), 6, None, p(dep), 0, H, W, intr, p(ws), p(cls), st),
              (p(pts), 64, p(w2c), 6, None, None, 8, H, W, intr, p(ws), p(cls), st),
              (p(pts), 64, p(w2c), 6, None, None, 0, 0, W, intr, None, p(cls), st),
              (p(pts), 64, p(w2c), 6, None, p(dep), 8, H, W, intr, None, p(cls), st),
              (None, 64, p(w2c), 6, None, None, 0, H, W, intr, None, p(cls), st)):
        assert L.dns_point_masks(*a) == -1
        assert b"dns_point_masks" in L.dns_last_error()
    assert int(L.dns_point_masks_ws_bytes(1 << 31, 6, 8)) == 0
    assert int(L.dns_point_masks_ws_bytes(1000, 6, 256)) == 4 * 6 * 4 and int(L.dns_point_masks_ws_bytes(1000, 6, 5000)) == 6 * 4
    torch.cuda.synchronize()
    assert bool((cls == 7).all())


# ---- Mesher -----------------------------------------------------------------------------------------------------------------
B = 16384


@functools.lru_cache(None)
def _mesher():
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = tgm._mapper()
    cfg = copy.deepcopy(cfg)
    cfg["meshing"]["resolution"] = 48
    kfs = tgm._keyframes(frames)
    w2c = torch.inverse(torch.stack([k["est_c2w"] for k in kfs]).to(DEV)).float()
    labs = torch.stack([k["gt_label"] for k in kfs]).to(DEV)
    dep = torch.stack([k["gt_depth"] for k in kfs]).to(DEV).float()
    md = torch.stack([k["gt_depth"].max() for k in kfs]).to(DEV)
    return {"mesher": Mesher(cfg, mapper), "kfs": kfs, "cam": cam, "H": cam["H"], "W": cam["W"], "mapper": mapper, "w2c": w2c,
            "labs": labs, "dep": dep, "md": md, "frames": frames}


def _grid_points(grid):
    x, y, z = grid["xyz"]
    xx, yy, zz = np.meshgrid(x, y, z)
    return torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float).to(DEV).contiguous()


@pytest.mark.parametrize("depth_test", [False, True])
def test_grid_occupancy_forecast(depth_test):
    from dns_slam_amd import ops
    m = _mesher()
    mesher, mapper, cam = m["mesher"], m["mapper"], m["cam"]
    vol, grid = mesher.grid_occupancy(m["kfs"], forecast=True, depth_test=depth_test)
    gp = _grid_points(grid)
    nx, ny, nz = (len(a) for a in grid["xyz"])
    kw = {"depths": m["dep"], "chunk": B} if depth_test else {"max_depth": m["md"]}
    cls = ops.point_masks(gp, m["w2c"], cam, m["H"], m["W"], **kw)
    seen, fore, unseen = cls == 1, cls == 2, cls == 0
    assert bool(seen.any()) and bool(fore.any()) and bool(unseen.any())
    occ = torch.zeros(gp.shape[0], device=DEV)
    lab, _ = ops.keyframe_project(gp[seen], m["w2c"], m["labs"], m["md"], cam)
    occ[seen] = mapper.eval_occupancy(gp[seen], lab, stage="fine", rule_chunk=B)
    occ[fore] = mapper.eval_occupancy(gp[fore], None, stage="coarse", rule_chunk=B)
    occ[unseen] = -100
    ref = occ.reshape(ny, nx, nz).permute(1, 0, 2)
    assert torch.equal(vol, ref)
    assert bool((vol.permute(1, 0, 2).reshape(-1)[unseen] == -100).all())
    plain, _ = mesher.grid_occupancy(m["kfs"])
    assert plain.shape == vol.shape and bool((plain != vol).any())


def test_extract_forecast_colours_and_file(tmp_path):
    from dns_slam_amd import ops
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    v, f, c, l = mesher.extract(kfs, forecast=True, clean_mesh=False)
    assert f.shape[0] > 100
    fore = ops.point_masks(v * mesher.scale, m["w2c"], m["cam"], m["H"], m["W"], max_depth=m["md"]) == 2
    assert bool(fore.any()) and bool((~fore).any())
    assert bool((c[fore] == torch.tensor([0, 255, 255], dtype=torch.uint8, device=DEV)).all())
    c0, l0 = mesher.vertex_query(v * mesher.scale, mesher._keyframes(kfs))
    assert torch.equal(c[~fore], c0[~fore]) and torch.equal(l, l0)
    assert bool((c0[fore] != c[fore]).any())                  # the colours were the networks' before
    paths = mesher.get_mesh(str(tmp_path), kfs, 3, forecast=True, clean_mesh=False)
    assert [p.split("/")[-1] for p in paths] == ["mesh_3.ply"]
    pv, pf = mc_ref.read_ply(paths[0])
    assert (np.stack((pv["x"], pv["y"], pv["z"]), 1) == v.cpu().numpy()).all() and (pf == f.cpu().numpy()).all()
    assert (np.stack((pv["red"], pv["green"], pv["blue"]), 1) == c.cpu().numpy()).all()
    assert (pv["label"] == l.cpu().numpy()).all()


def _compacted(rv, rf, keep):
    fk = rf[keep]
    used = np.zeros(len(rv), bool)
    used[fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return rv[used], remap[fk].astype(np.int32)


def test_extract_forecast_bound_planes():
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    with pytest.raises(NotImplementedError, match="get_bound_from_frames"):
        mesher.extract(kfs, forecast=True)
    with pytest.raises(NotImplementedError, match="get_bound_from_frames"):
        mesher.get_mesh("/nonexistent", kfs, 0, forecast=True, clean_mesh=True)
    v0, f0, _, _ = mesher.extract(kfs, forecast=True, clean_mesh=False)
    rv, rf = v0.cpu().numpy(), f0.cpu().numpy()
    lo, hi = rv.astype(np.float64).min(0), rv.astype(np.float64).max(0)
    bmin, bmax = lo + 0.3 * (hi - lo), hi - 0.2 * (hi - lo)            # a box strictly inside the mesh's extent
    planes = np.zeros((6, 4))
    for a in range(3):
        planes[2 * a, a], planes[2 * a, 3] = 1.0, -bmax[a]              # x_a - max <= 0
        planes[2 * a + 1, a], planes[2 * a + 1, 3] = -1.0, bmin[a]      # min - x_a <= 0
    inside = ((rv.astype(np.float64) <= bmax) & (rv.astype(np.float64) >= bmin)).all(1)
    keep = inside[rf].any(1)
    assert 0 < keep.sum() < len(rf)
    v1, f1, c1, l1 = mesher.extract(kfs, forecast=True, clean_mesh=True, bound_planes=planes)
    ev, ef = _compacted(rv, rf, keep)
    assert (f1.cpu().numpy() == ef).all() and (v1.cpu().numpy() == ev).all()
    assert c1.shape == (len(ev), 3) and l1.shape == (len(ev),)


def test_extract_depth_test_cleaning():
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    v0, f0, _, _ = mesher.extract(kfs, clean_mesh=False)
    va, fa, _, _ = mesher.extract(kfs, clean_mesh=True)
    vb, fb, _, _ = mesher.extract(kfs, clean_mesh=True, depth_test=True)
    assert 0 < fb.shape[0] < fa.shape[0]
    # the torch composition: the restatement's depth-tested seen mask at the vertices, the faces with a seen vertex, compacted
    seen, _, _, _ = R.point_masks_ref(v0 * mesher.scale, m["w2c"], m["cam"], m["H"], m["W"], depths=m["dep"], chunk=B)
    rv, rf = v0.cpu().numpy(), f0.cpu().numpy()
    ev, ef = _compacted(rv, rf, seen.cpu().numpy()[rf].any(1))
    assert (fb.cpu().numpy() == ef).all() and (vb.cpu().numpy() == ev).all()


def test_all_frames_ignores_later_poses():
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    s = _scene()
    pts = s["pts"][:50000]
    est = m["frames"]["est_c2w"]
    a = mesher.point_masks(pts, kfs, est, 2, get_mask_use_all_frames=True)
    b = mesher.point_masks(pts, kfs, est[:3], 2, get_mask_use_all_frames=True)
    full = mesher.point_masks(pts, kfs, est, 5, get_mask_use_all_frames=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool((a[0] != full[0]).any())
    assert bool(((a[0].int() + a[1].int() + a[2].int()) == 1).all())
    w2c = torch.inverse(est[:3].to(DEV).double()).float()
    seen, fore, unseen, near = R.point_masks_ref(pts, w2c, m["cam"], m["H"], m["W"])
    _assert_matches(R.classes(a[0], a[1]), R.classes(seen, fore), near, pts.shape[0])
    with pytest.raises(ValueError):
        mesher.point_masks(pts, kfs, get_mask_use_all_frames=True)
    va, _ = mesher.grid_occupancy(kfs, forecast=True, all_frames=(est, 2))
    vb, _ = mesher.grid_occupancy(kfs, forecast=True, all_frames=(est[:3], 2))
    vf, _ = mesher.grid_occupancy(kfs, forecast=True, all_frames=(est, 5))
    assert torch.equal(va, vb) and bool((va != vf).any())


def test_mesher_point_masks_modes():
    """Mesher.point_masks is ops.point_masks in the keyframes' mode; ``depths`` replaces gt_depth in the depth test."""
    from dns_slam_amd import ops
    m = _mesher()
    mesher, kfs, cam = m["mesher"], m["kfs"], m["cam"]
    pts = _scene()["pts"][:50000]
    for depth_test, kw in ((False, {"max_depth": m["md"]}), (True, {"depths": m["dep"], "chunk": B})):
        seen, fore, unseen = mesher.point_masks(pts, kfs, depth_test=depth_test)
        cls = ops.point_masks(pts, m["w2c"], cam, m["H"], m["W"], **kw)
        assert torch.equal(seen, cls == 1) and torch.equal(fore, cls == 2) and torch.equal(unseen, cls == 0)
    other = m["dep"] * 0.5
    seen2, _, _ = mesher.point_masks(pts, kfs, depth_test=True, depths=other)
    assert torch.equal(seen2, ops.point_masks(pts, m["w2c"], cam, m["H"], m["W"], depths=other, chunk=B) == 1)
    assert bool((seen2 != seen).any())
