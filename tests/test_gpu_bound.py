"""GPU: the scene bound from keyframes -- TSDF fusion (csrc/tsdf.hip, ops.tsdf_fuse / ops.tsdf_vertices) against the float32
restatement tests/tsdf_ref.py bit for bit, the convex hull (csrc/hull.hip, ops.convex_hull) against scipy's under the acceptance of
tests/hull_ref.py, and Mesher.get_bound_from_frames / bound_planes="frames" built on them."""
import copy
import functools

import numpy as np
import pytest
import torch

import hull_ref as HR
import mc_ref
import test_gpu_mesh as tgm
import tsdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COARSE = (4.0 / 128.0, 0.16)
REFERENCE = (4.0 / 512.0, 0.04)


# ---- TSDF -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _frames():
    bound, cam, frames = tgm._scene(6)
    return cam, {k: v.numpy() for k, v in frames.items() if hasattr(v, "numpy")}


@functools.lru_cache(None)
def _case(name):
    """(cam, depths, extrinsic, pose, voxel_length, sdf_trunc) and the restatement's answer; computed once, never modified."""
    cam, frames = _frames()
    idx, (vl, tr) = {"coarse": ((0, 1, 2), COARSE), "reference": ((0, 1), REFERENCE), "odd": ((0, 1, 2), COARSE),
                     "zero_frame": ((0, 1, 2), COARSE)}[name]
    c2w, depths = R.scene_keyframes(frames, idx)
    if name == "odd":                                            # height and width no multiples of the stride
        depths = np.ascontiguousarray(depths[:, :57, :78])
    if name == "zero_frame":                                     # a frame that contributes nothing, between the others
        depths = depths.copy()
        depths[1] = 0.0
    E, P, _ = R.poses(c2w)
    ref = R.fuse(depths, E, P, cam, vl, tr)
    ref["verts"] = R.vertices(ref["units"], ref["tsdf"], ref["weight"], vl)
    return cam, depths, E, P, vl, tr, ref


def _fuse(name, **kw):
    from dns_slam_amd import ops
    cam, depths, E, P, vl, tr, ref = _case(name)
    out = ops.tsdf_fuse(torch.from_numpy(depths).to(DEV), torch.from_numpy(E).to(DEV), torch.from_numpy(P).to(DEV), cam, vl, tr, **kw)
    return out, ops.tsdf_vertices(*out, vl), ref


def _assert_bits(out, verts, ref):
    units, tsdf, weight = (t.cpu().numpy() for t in out)
    assert units.dtype == np.int32 and tsdf.dtype == np.float32 and weight.dtype == np.float32 and verts.dtype == torch.float64
    assert np.array_equal(units, ref["units"])
    assert np.array_equal(weight, ref["weight"])
    assert np.array_equal(tsdf.view(np.uint32), ref["tsdf"].view(np.uint32))
    v = verts.cpu().numpy()
    assert v.shape == ref["verts"].shape
    assert np.array_equal(v.view(np.uint64), ref["verts"].view(np.uint64))


@pytest.mark.parametrize("name", ["coarse", "reference", "odd", "zero_frame"])
def test_tsdf_matches_restatement_bit_for_bit(name):
    out, verts, ref = _fuse(name)
    print(f"{name}: units {len(ref['units'])}, pairs {len(ref['pairs'])}, vertices {len(ref['verts'])}, max weight {ref['weight'].max()}")
    assert ref["weight"].max() == 2.0 and len(ref["verts"]) > 10000           # the running average and the extraction are exercised
    _assert_bits(out, verts, ref)
    if name == "zero_frame":
        assert not (ref["pairs"][:, 3] == 1).any()


def test_tsdf_small_table_retries_to_the_same_bits():
    out, verts, ref = _fuse("coarse", table_slots=8)             # 893 keys: the table is doubled seven times
    _assert_bits(out, verts, ref)


def test_tsdf_repeatable():
    a, va, _ = _fuse("coarse")
    b, vb, _ = _fuse("coarse")
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(va, vb)


def test_tsdf_empty_and_refusals():
    from dns_slam_amd import ops
    cam, depths, E, P, vl, tr, _ = _case("coarse")
    d, e, p = torch.from_numpy(depths).to(DEV), torch.from_numpy(E).to(DEV), torch.from_numpy(P).to(DEV)
    units, tsdf, weight = ops.tsdf_fuse(d[:0], e[:0], p[:0], cam, vl, tr)                     # K = 0
    assert units.shape == (0, 3) and tsdf.shape == (0, 16, 16, 16) and weight.shape == (0, 16, 16, 16)
    assert ops.tsdf_vertices(units, tsdf, weight, vl).shape == (0, 3)
    units, tsdf, weight = ops.tsdf_fuse(torch.zeros_like(d), e, p, cam, vl, tr)               # nothing to fuse
    assert units.shape == (0, 3)
    big = torch.zeros(1, 1, 1, device=DEV).expand(65536, 1, 1)
    for args, match in (((d.double(), e, p), "depths"), ((d, e.float(), p), "extrinsic"), ((d, e, p.float()), "pose"),
                        ((d.cpu(), e, p), "depths"), ((d, e.cpu(), p), "extrinsic"), ((d[0], e, p), "depths"),
                        ((d, e[:2], p), "extrinsic"), ((d, e, p[:, :3]), "pose"),
                        ((big, e[:1].expand(65536, 4, 4), p[:1].expand(65536, 4, 4)), "depths")):
        with pytest.raises(ValueError, match=match):
            ops.tsdf_fuse(*args, cam, vl, tr)
    with pytest.raises(ValueError, match="sdf_trunc"):
        ops.tsdf_fuse(d, e, p, cam, vl, 8 * vl)                                              # 2 trunc >= 16 voxel_length
    with pytest.raises(ValueError, match="stride"):
        ops.tsdf_fuse(d, e, p, cam, vl, tr, stride=0)
    far = p.clone()
    far[:, :3, 3] += 40000.0 * 16 * vl                                                       # unit index outside 16 bits
    with pytest.raises(ValueError, match="16 bits"):
        ops.tsdf_fuse(d, e, far, cam, vl, tr)
    (units, tsdf, weight), _, _ = _fuse("coarse")
    for args, match in (((units.long(), tsdf, weight), "units"), ((units, tsdf.double(), weight), "tsdf"),
                        ((units, tsdf, weight[:-1]), "weight"), ((units.flip(0), tsdf, weight), "units"),
                        ((units.cpu(), tsdf, weight), "units")):
        with pytest.raises(ValueError, match=match):
            ops.tsdf_vertices(*args, vl)


# ---- convex hull --------------------------------------------------------------------------------------------------------------
def _hull(points, eps=0.0):
    from dns_slam_amd import ops
    vi, faces, planes, mo = ops.convex_hull(torch.as_tensor(points).to(DEV), eps)
    assert vi.dtype == torch.int64 and faces.dtype == torch.int64 and planes.dtype == torch.float64 and isinstance(mo, float)
    return vi.cpu().numpy(), faces.cpu().numpy(), planes.cpu().numpy(), mo


def _ball(n=2000, seed=0):
    g = np.random.default_rng(seed)
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * g.random((n, 1)) ** (1 / 3)


def _lattice(n=17):
    a = np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def _box(n=200000, seed=1):
    g = np.random.default_rng(seed)
    p = g.random((n, 3)) * np.array([6.0, 4.0, 3.0])
    face = g.integers(0, 6, n)
    ext = np.array([6.0, 4.0, 3.0])
    p[np.arange(n), face // 2] = (face % 2) * ext[face // 2]
    return p + g.uniform(-1e-3, 1e-3, (n, 3))


def test_hull_ball_matches_scipy_vertices():
    pts = _ball()
    hull = HR.scipy_hull(pts)
    vi, faces, planes, mo = _hull(pts)
    print(HR.accept(pts, 0.0, vi, faces, planes, mo, hull))
    assert np.array_equal(vi, np.sort(hull.vertices))            # general position: the vertex sets are equal
    assert faces.shape[0] == 2 * vi.size - 4


@pytest.mark.parametrize("eps", [0.0, 1e-3])
def test_hull_lattice(eps):
    pts = _lattice()
    vi, faces, planes, mo = _hull(pts, eps)
    print(HR.accept(pts, eps, vi, faces, planes, mo))
    corners = [i for i, p in enumerate(pts) if all(c in (0.0, 16.0) for c in p)]
    assert len(corners) == 8 and set(corners) <= set(vi.tolist())


def test_hull_box_with_noise():
    """Room-like: 200 000 points on the six faces of a box; the live list is compacted on the way."""
    from dns_slam_amd import ops
    pts = _box()
    t = torch.from_numpy(pts).to(DEV)
    faces, planes, info = ops.convex_hull_launch(t)
    print(info)
    vi = torch.unique(faces.reshape(-1))
    print(HR.accept(pts, 0.0, vi.cpu().numpy(), faces.cpu().numpy(), planes.cpu().numpy(), info["max_outside"]))
    assert info["rounds"] >= vi.numel() - 4 > 100             # an inserted point may be swallowed later
    small = ops.convex_hull_launch(t, face_cap=64)               # too few face slots: quadrupled until the hull fits, same hull
    assert small[2]["face_cap"] > 64 and torch.equal(small[0], faces) and torch.equal(small[1], planes)


def test_hull_small_and_degenerate_inputs():
    from dns_slam_amd import ops
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.2, 0.3, 1.0]])
    vi, faces, planes, mo = _hull(tet)                                       # N = 4
    HR.accept(tet, 0.0, vi, faces, planes, mo)
    assert vi.tolist() == [0, 1, 2, 3] and faces.shape == (4, 3)
    pts = np.concatenate((_ball(300, 3), _ball(300, 3)))                     # all points duplicated
    vi, faces, planes, mo = _hull(pts)
    HR.accept(pts, 0.0, vi, faces, planes, mo)
    assert vi.max() < 300                                                    # ties go to the smallest index: never a second copy
    assert np.array_equal(vi, np.sort(HR.scipy_hull(pts[:300]).vertices))
    g = np.random.default_rng(4)
    flat = g.random((500, 3))
    flat[:, 2] = 2.0 * flat[:, 0] - flat[:, 1] + 1.0
    for bad in (flat, tet[:3], np.zeros((10, 3))):                           # coplanar, N = 3, one point ten times
        with pytest.raises(ValueError, match="points"):
            ops.convex_hull(torch.from_numpy(bad).to(DEV))
    for bad, match in ((torch.from_numpy(tet), "GPU"), (torch.from_numpy(tet).to(DEV).long(), "float"),
                       (torch.from_numpy(tet).to(DEV)[:, :2], r"\[N,3\]")):
        with pytest.raises(ValueError, match=match):
            ops.convex_hull(bad)
    with pytest.raises(ValueError, match="eps"):
        ops.convex_hull(torch.from_numpy(tet).to(DEV), eps=-1.0)
    nan = torch.from_numpy(_ball(50, 5)).to(DEV)
    nan[7, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        ops.convex_hull(nan)


def test_hull_float32_is_widened_and_calls_repeat():
    from dns_slam_amd import ops
    p32 = torch.from_numpy(_ball(1000, 6).astype(np.float32)).to(DEV)
    a = ops.convex_hull(p32)
    b = ops.convex_hull(p32.double())
    c = ops.convex_hull(p32)
    for x, y in ((a, b), (a, c)):
        assert all(torch.equal(s, t) for s, t in zip(x[:3], y[:3])) and x[3] == y[3]
    HR.accept(p32.double().cpu().numpy(), 0.0, *(t.cpu().numpy() for t in a[:3]), a[3])


# ---- Mesher -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _mesher():
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = tgm._mapper()
    cfg = copy.deepcopy(cfg)
    cfg["meshing"]["resolution"] = 48
    kfs = tgm._keyframes(frames)
    return {"mesher": Mesher(cfg, mapper), "kfs": kfs, "cam": cam, "cfg": cfg, "mapper": mapper}


def _grid_points(grid):
    x, y, z = grid["xyz"]
    xx, yy, zz = np.meshgrid(x, y, z)
    return torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float).to(DEV).contiguous()


def _snapshot(kfs):
    return [{k: v.clone() for k, v in kf.items()} for kf in kfs]


def _unchanged(kfs, snap):
    return all(torch.equal(kf[k], s[k]) for kf, s in zip(kfs, snap) for k in s)


def test_get_bound_from_frames_matches_restatement_and_scipy():
    """Coarse voxels keep the numpy restatement at a second; the default hull tolerance is 0, so eps = 0 below."""
    from dns_slam_amd.meshing import Bound, inside_planes
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    snap = _snapshot(kfs)
    vl, tr = COARSE
    b = mesher.get_bound_from_frames(kfs, voxel_length=vl, sdf_trunc=tr)
    assert isinstance(b, Bound) and b.verts.dtype == torch.float64 and b.planes.shape == (b.faces.shape[0], 4)
    assert _unchanged(kfs, snap)                                  # the reference's in-place negation is not copied
    c2w = np.stack([k["est_c2w"].numpy() for k in kfs])
    depths = np.stack([k["gt_depth"].numpy() for k in kfs]).astype(np.float32)
    E, P, centres = R.poses(c2w)
    ref = R.fuse(depths, E, P, m["cam"], vl, tr)
    pts = np.concatenate((centres, R.vertices(ref["units"], ref["tsdf"], ref["weight"], vl)))
    ref_planes, c = HR.scaled_planes(pts, mesher.clean_mesh_bound_scale)
    probes = _grid_points(mesher.get_grid_uniform())
    got = inside_planes(probes, b.planes).cpu().numpy()
    pr = probes.double().cpu().numpy()
    val = HR.max_over_faces(ref_planes, pr)
    want = val <= 0
    eps, r = 0.0, 1e-9 * float(np.abs(pts).max())
    near = np.zeros(len(pr), bool)
    for s in range(0, len(ref_planes), 64):
        near |= (np.abs(HR.plane_values(ref_planes[s:s + 64], pr)) <= 2 * eps + r).any(1)
    print(f"probes {len(pr)}: inside {int(want.sum())}, outside {int((~want).sum())}, near {int(near.sum())}, differ {int((got != want).sum())}, "
          f"hull faces {b.faces.shape[0]} (scipy {len(ref_planes)})")
    assert want.any() and (~want).any()
    assert near.sum() <= 0.005 * len(pr)
    assert not ((got != want) & ~near).any()
    # the scaled hull's own vertices lie on its planes and its faces index them
    vals = HR.plane_values(b.planes.cpu().numpy(), b.verts.cpu().numpy())
    assert vals.max() <= 1e-9 * float(np.abs(pts).max()) and int(b.faces.max()) == b.verts.shape[0] - 1 and int(b.faces.min()) == 0


def test_extract_and_get_mesh_with_the_frames_bound(tmp_path):
    m = _mesher()
    mesher, kfs = m["mesher"], m["kfs"]
    snap = _snapshot(kfs)
    planes = mesher.get_bound_from_frames(kfs).planes
    a = mesher.extract(kfs, forecast=True, bound_planes="frames")
    b = mesher.extract(kfs, forecast=True, bound_planes=planes)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[1].shape[0] > 100
    raw = mesher.extract(kfs, forecast=True, clean_mesh=False)
    assert 0 < a[1].shape[0] < raw[1].shape[0]                    # the bound removes some faces, not all
    pa = mesher.get_mesh(str(tmp_path / "a"), kfs, 1, forecast=True, bound_planes="frames")
    pb = mesher.get_mesh(str(tmp_path / "b"), kfs, 1, forecast=True, bound_planes=planes)
    assert open(pa[0], "rb").read() == open(pb[0], "rb").read()
    pv, pf = mc_ref.read_ply(pa[0])
    assert (pf == a[1].cpu().numpy()).all() and (np.stack((pv["x"], pv["y"], pv["z"]), 1) == a[0].cpu().numpy()).all()
    vol_a, _ = mesher.grid_occupancy(kfs, forecast=True, bound_planes="frames")
    vol_b, _ = mesher.grid_occupancy(kfs, forecast=True)
    assert torch.equal(vol_a, vol_b)
    for call in (lambda: mesher.extract(kfs, forecast=True, bound_planes="other"),
                 lambda: mesher.get_mesh(str(tmp_path / "c"), kfs, 1, forecast=True, bound_planes="other"),
                 lambda: mesher.grid_occupancy(kfs, forecast=True, bound_planes="other")):
        with pytest.raises(ValueError, match="bound_planes"):
            call()
    with pytest.raises(NotImplementedError, match='bound_planes="frames"'):
        mesher.extract(kfs, forecast=True)
    assert _unchanged(kfs, snap)


def test_clean_mesh_bound_scale_is_honoured():
    from dns_slam_amd.meshing import Mesher
    m = _mesher()
    kfs = m["kfs"]
    n_faces, planes = {}, {}
    for s in (1.02, 1.5):
        cfg = copy.deepcopy(m["cfg"])
        cfg["meshing"]["clean_mesh_bound_scale"] = s
        mesher = Mesher(cfg, m["mapper"])
        assert mesher.clean_mesh_bound_scale == s
        planes[s] = mesher.get_bound_from_frames(kfs).planes
        n_faces[s] = mesher.extract(kfs, forecast=True, bound_planes="frames")[1].shape[0]
    assert m["mesher"].clean_mesh_bound_scale == 1.02            # the default
    assert torch.equal(planes[1.02][:, :3], planes[1.5][:, :3]) and bool((planes[1.5][:, 3] < planes[1.02][:, 3]).all())
    print(n_faces)
    assert n_faces[1.5] >= n_faces[1.02] > 0
