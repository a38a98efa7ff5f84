"""GPU: the mesh component pass (csrc/mesh_cc.hip, ops.mesh_components) against the host reference of tests/mesh_cc_ref.py, and
its users in dns_slam_amd.meshing (filter_components, extract / get_mesh with components=, get_part_meshes).

Tolerance of comp_area: both sides sum the same float64 face areas (bit for bit: -ffp-contract=off) in different orders; a
float64 sum of F positive terms moves by at most a relative F 2^-53 with its order, so two orders differ by at most F 2^-52."""
import copy
import functools

import numpy as np
import pytest
import torch

import mc_ref
import mesh_cc_ref as cc
from test_gpu_mesh import _keyframes, _mapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = dict(cc.HAND_BUILT, five_spheres=cc.five_spheres, random_field=cc.random_surface, open_surface=cc.open_surface,
             closed_strip=lambda: cc.strip(5000, closed=True))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, reference comp, comp_area, n_comp), computed once and shared; nobody writes into them."""
    v, f = CASES[name]()
    out = (v, f) + cc.components(v, f)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # a copy: the shared cases are read-only


def _gpu(v, f):
    from dns_slam_amd import ops
    comp, area, n = ops.mesh_components(_t(v), _t(f))
    assert comp.dtype == torch.int32 and area.dtype == torch.float64 and comp.shape == area.shape == (len(f),)
    return comp.cpu().numpy(), area.cpu().numpy(), n


def _assert_same(got, ref, F):
    (gc, ga, gn), (rc, ra, rn) = got, ref
    print(f"F {F}: components {gn} (reference {rn}), worst relative area difference "
          f"{np.abs(ga / ra - 1).max() if F and (ra > 0).all() else 0.0:.3e}, bound {F * 2.0 ** -52:.3e}")
    assert gn == rn
    assert (gc == rc).all()
    assert (np.abs(ga - ra) <= F * 2.0 ** -52 * ra).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_components_equal_host_reference(name):
    v, f, rc, ra, rn = _case(name)
    _assert_same(_gpu(v, f), (rc, ra, rn), len(f))


def test_known_answers():
    assert _case("two_octahedra")[4] == 2 and _case("touching_tetrahedra")[4] == 2 and _case("fan")[4] == 3
    assert _case("open_strip")[4] == 1 and _case("doubled_face")[4] == 1 and _case("closed_strip")[4] == 1
    assert _case("five_spheres")[4] == 5 and _case("random_field")[4] == 3 and _case("open_surface")[4] == 1
    gc, ga, gn = _gpu(*_case("two_octahedra")[:2])
    assert (gc == np.repeat([0, 8], 8)).all()
    exact = 4 * np.sqrt(3.0) * np.repeat([1.0, 4.0], 8)
    assert (np.abs(ga - exact) <= 8 * 2.0 ** -52 * exact).all()


def _canonical(comp):
    """Relabel a partition by the smallest member of each part."""
    _, inv = np.unique(comp, return_inverse=True)
    small = np.full(inv.max() + 1, len(comp), np.int64)
    np.minimum.at(small, inv, np.arange(len(comp)))
    return small[inv]


@pytest.mark.parametrize("name", ["five_spheres", "closed_strip"])
@pytest.mark.parametrize("spread", [False, True])
def test_order_independence(name, spread):
    """Faces permuted and vertices relabelled at random (neighbouring faces land in different workgroups and hash slots, the
    unions form long chains); with ``spread`` the vertex ids reach up to 2^30 through unused vertices (2^24 if the device has
    no room for 12 GiB of positions)."""
    from dns_slam_amd import ops
    v, f, rc, ra, rn = _case(name)
    F, V = len(f), len(v)
    rng = np.random.default_rng(11 + spread)
    perm = rng.permutation(F)
    if spread:
        big = 1 << 30 if torch.cuda.mem_get_info()[0] >= (32 << 30) else 1 << 24
        step = big // V
        ids = rng.permutation(V).astype(np.int64) * step + rng.integers(0, step, V)
        assert ids.max() >= big // 2
    else:
        big, ids = V, rng.permutation(V).astype(np.int64)
    fp = ids[f[perm]].astype(np.int32)
    vp = torch.zeros(big, 3, device=DEV)
    vp[_t(ids)] = _t(v)
    comp, area, n = ops.mesh_components(vp, _t(fp))
    del vp
    comp, area = comp.cpu().numpy(), area.cpu().numpy()
    assert n == rn
    assert (comp == _canonical(comp)).all()                    # canonical ids in the permuted order, too
    back_c, back_a = np.empty_like(comp), np.empty_like(area)
    back_c[perm], back_a[perm] = comp, area
    assert (_canonical(back_c) == rc).all()
    assert (np.abs(back_a - ra) <= F * 2.0 ** -52 * ra).all()
    assert (comp == cc.components(v, f[perm])[0]).all()       # the ids do not depend on the vertex labels


def test_edge_cases():
    from dns_slam_amd import ops
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0]], device=DEV)
    comp, area, n = ops.mesh_components(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert comp.shape == (0,) and comp.dtype == torch.int32 and area.shape == (0,) and area.dtype == torch.float64 and n == 0
    gc, ga, gn = _gpu(v.cpu().numpy(), np.array([[0, 1, 2]], np.int32))
    assert gn == 1 and gc[0] == 0 and ga[0] == 0.5
    # zero-area faces: collinear points (0, 1, 3) next to a proper face, and a face that repeats a vertex, whose doubled edge
    # key (1, 2) then has three holders and joins nothing
    for faces in ([[0, 1, 2], [1, 0, 3]], [[0, 1, 2], [1, 2, 2]], [[1, 1, 1]], [[2, 1, 4], [1, 2, 2], [0, 1, 2]]):
        f = np.array(faces, np.int32)
        _assert_same(_gpu(v.cpu().numpy(), f), cc.components(v.cpu().numpy(), f), len(f))
    assert _gpu(v.cpu().numpy(), np.array([[0, 1, 2], [1, 0, 3]], np.int32))[1].tolist() == [0.5, 0.5]
    with pytest.raises(ValueError):
        ops.mesh_components(v.cpu(), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.mesh_components(v, torch.zeros(1, 3, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("bad", [5, -1, 2 ** 31 - 1, -2 ** 31])
def test_index_out_of_range_is_refused(bad):
    """V = 5: the index is flagged on the device and never dereferenced; the next call is unaffected."""
    from dns_slam_amd import ops
    v, f, rc, ra, rn = _case("two_octahedra")
    vt = _t(v[:5])
    faces = torch.tensor([[0, 1, 2], [1, 0, 3], [2, 1, bad], [0, 2, 4]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        ops.mesh_components(vt, faces)
    _assert_same(_gpu(v, f), (rc, ra, rn), len(f))


# ---- Mesher ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """The small mapper of test_gpu_mesh.py, its cleaned (unfiltered) mesh in the units extract works in, and the host
    reference's components of that mesh."""
    from dns_slam_amd import ops
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = _mapper()
    kfs = _keyframes(frames)
    mesher = Mesher(cfg, mapper)
    kf = mesher._keyframes(kfs)
    vol, grid = mesher.grid_occupancy(kfs, kf=kf)
    x, y, z = grid["xyz"]
    v0, f0 = ops.marching_cubes(vol, mesher.level_set, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
    vc, fc = mesher.clean(v0, f0, kf)
    comp, area, n = cc.components(vc.cpu().numpy(), fc.cpu().numpy())
    return {"cfg": cfg, "mapper": mapper, "kfs": kfs, "kf": kf, "mesher": mesher, "raw": (v0, f0), "clean": (vc, fc),
            "ref": (comp, area, n)}


def _expect_kept(v, f, keep):
    """numpy restatement of the compaction: the kept faces and the vertices they use, in their original order."""
    fk = f[keep]
    used = np.zeros(len(v), bool)
    used[fk.reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[fk].astype(np.int32)


def _assert_mesh(gv, gf, rv, rf):
    assert gf.dtype == torch.int32 and tuple(gv.shape) == rv.shape and tuple(gf.shape) == rf.shape
    assert (gv.cpu().numpy() == rv).all() and (gf.cpu().numpy() == rf).all()


def test_filter_components_five_spheres(scene):
    mesher = scene["mesher"]
    v, f, rc, ra, rn = _case("five_spheres")
    vt, ft = _t(v), _t(f)
    keep = ra > 0.2
    assert len(np.unique(rc[keep])) == 3 and len(np.unique(rc[~keep])) == 2
    gv, gf = mesher.filter_components(vt, ft, min_area=0.2)
    _assert_mesh(gv, gf, *_expect_kept(v, f, keep))
    assert (gv.cpu().numpy()[gf.cpu().numpy()] == v[f[keep]]).all()          # the same corner positions through the new indices
    gv, gf = mesher.filter_components(vt, ft, largest=True)
    big = ra == ra.max()
    assert abs(ra.max() - 2.0002) < 5e-5 and 0 < big.sum() < len(f)
    _assert_mesh(gv, gf, *_expect_kept(v, f, big))
    gv, gf = mesher.filter_components(vt, ft, min_area=10)
    assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3) and gf.dtype == torch.int32
    gv, gf = mesher.filter_components(vt, ft[:0], min_area=0.2)
    assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3)
    # strict comparison: a threshold equal to a component's area drops that component (the octahedra's 8 equal terms sum
    # exactly in any order, so the figure is the same in every run)
    v8, f8 = _case("two_octahedra")[:2]
    small = float(_gpu(v8, f8)[1][0])
    assert small == 8 * (0.5 * np.sqrt(3.0))
    assert mesher.filter_components(_t(v8), _t(f8), min_area=small)[1].shape[0] == 8
    assert mesher.filter_components(_t(v8), _t(f8), min_area=float(np.nextafter(small, 0.0)))[1].shape[0] == 16
    # ties of largest=True go to the smallest component id
    v2, f2 = cc.two_octahedra()
    v2[6:] = v2[:6] + np.float32(8.0)                                          # two equal octahedra
    gv, gf = mesher.filter_components(_t(v2), _t(f2), largest=True)
    _assert_mesh(gv, gf, v2[:6], f2[:8])
    with pytest.raises(ValueError):
        mesher.filter_components(vt, ft)
    with pytest.raises(ValueError):
        mesher.filter_components(vt, ft, min_area=0.2, largest=True)


def _threshold(area_per_comp):
    """Midway between two distinct component areas (the middle pair), or None when there is only one."""
    a = np.unique(area_per_comp)
    if len(a) < 2:
        return None
    k = len(a) // 2
    return float(0.5 * (a[k - 1] + a[k]))


def test_extract_components_step_by_step(scene):
    from dns_slam_amd.meshing import Mesher
    mesher, kfs, kf, cfg, mapper = scene["mesher"], scene["kfs"], scene["kf"], scene["cfg"], scene["mapper"]
    vc, fc = scene["clean"]
    rc, ra, rn = scene["ref"]
    vcn, fcn = vc.cpu().numpy(), fc.cpu().numpy()
    assert len(fcn) > 100
    _assert_same(_gpu(vcn, fcn), (rc, ra, rn), len(fcn))
    # components=None: the parent's extraction (marching cubes -> clean -> vertex query), unchanged
    v1, f1, c1, l1 = mesher.extract(kfs)
    _assert_mesh(v1 * mesher.scale, f1, vcn, fcn)
    cq, lq = mesher.vertex_query(vc, kf)
    assert (c1 == cq).all() and (l1 == lq).all()
    v0, f0, _, _ = mesher.extract(kfs, clean_mesh=False)
    _assert_mesh(v0 * mesher.scale, f0, scene["raw"][0].cpu().numpy(), scene["raw"][1].cpu().numpy())
    # largest
    big = rc == rc[ra == ra.max()].min()
    v3, f3, c3, l3 = mesher.extract(kfs, components="largest")
    _assert_mesh(v3 * mesher.scale, f3, *_expect_kept(vcn, fcn, big))
    sv, sf = mesher.filter_components(vc, fc, largest=True)
    assert (v3 * mesher.scale == sv).all() and (f3 == sf).all()
    cq, lq = mesher.vertex_query(sv, kf)
    assert (c3 == cq).all() and (l3 == lq).all()
    # small, with the threshold between two component areas of the host reference
    thr = _threshold(ra[np.unique(rc)])
    print(f"cleaned mesh: {len(fcn)} faces, {rn} components, threshold {thr}")
    if thr is None:
        print("the random mapper's cleaned mesh is ONE component: components='small' is covered by 'largest' above only")
    else:
        keep = ra > thr
        assert 0 < keep.sum() < len(fcn)
        v2, f2, c2, l2 = mesher.extract(kfs, components="small", min_area=thr)
        _assert_mesh(v2 * mesher.scale, f2, *_expect_kept(vcn, fcn, keep))
        sv, sf = mesher.filter_components(vc, fc, min_area=thr)
        assert (v2 * mesher.scale == sv).all() and (f2 == sf).all()
        cq, lq = mesher.vertex_query(sv, kf)
        assert (c2 == cq).all() and (l2 == lq).all()
        # the config key, times scale^2; an explicit min_area overrides it
        c = copy.deepcopy(cfg)
        c["meshing"]["remove_small_geometry_threshold"] = thr
        m2 = Mesher(c, mapper)
        assert all((a == b).all() for a, b in zip(m2.extract(kfs, components="small"), (v2, f2, c2, l2)))
        c["meshing"]["remove_small_geometry_threshold"] = 1e9
        m3 = Mesher(c, mapper)
        assert m3.extract(kfs, components="small")[1].shape[0] == 0
        assert all((a == b).all() for a, b in zip(m3.extract(kfs, components="small", min_area=thr), (v2, f2, c2, l2)))
    # refusals
    with pytest.raises(ValueError, match="remove_small_geometry_threshold"):
        mesher.extract(kfs, components="small")
    for comp in ("small", "largest"):
        with pytest.raises(ValueError, match="clean_mesh"):
            mesher.extract(kfs, clean_mesh=False, components=comp, min_area=0.1)
    with pytest.raises(ValueError):
        mesher.extract(kfs, components="biggest")


def _read(path):
    pv, pf = mc_ref.read_ply(path)
    return np.stack((pv["x"], pv["y"], pv["z"]), 1), pf, np.stack((pv["red"], pv["green"], pv["blue"]), 1), pv["label"]


def test_get_mesh_components_and_part_meshes(scene, tmp_path):
    mesher, kfs = scene["mesher"], scene["kfs"]
    rc, ra, rn = scene["ref"]
    thr = _threshold(ra[np.unique(rc)])
    kw = {"components": "largest"} if thr is None else {"components": "small", "min_area": thr}
    v, f, c, l = (t.cpu().numpy() for t in mesher.extract(kfs, **kw))
    assert 0 < len(f) < scene["clean"][1].shape[0] or rn == 1
    paths = mesher.get_mesh(str(tmp_path), kfs, 3, **kw)
    assert [p.split("/")[-1] for p in paths] == ["mesh_3.ply"]
    pv, pf, pc, pl = _read(paths[0])
    assert (pv == v).all() and (pf == f).all() and (pc == c).all() and (pl == l).all()
    # the per-class meshes of the same extraction
    parts = mesher.get_part_meshes(str(tmp_path), kfs, 3, **kw)
    ids = np.unique(l)
    assert [p.split("/")[-1] for p in parts] == [f"mesh_3_part_{int(e)}.ply" for e in ids]
    covered = np.zeros(len(f), bool)
    for e, path in zip(ids, parts):
        qv, qf, qc, ql = _read(path)
        keep = (l == e)[f].any(1)
        rv, rf = _expect_kept(v, f, keep)
        assert len(qf) > 0 and (qv == rv).all() and (qf == rf).all()
        assert ((ql == e)[qf]).any(1).all()                                    # every face has a vertex of this part's label
        used = np.zeros(len(v), bool)
        used[f[keep].reshape(-1)] = True
        assert (qc == c[used]).all() and (ql == l[used]).all()                 # the full mesh's colours and labels
        covered |= keep
    assert covered.all()
    # without colours the part files still carry the labels
    parts_nc = mesher.get_part_meshes(str(tmp_path / "nc"), kfs, 4, color=False, **kw)
    qv, qf = mc_ref.read_ply(parts_nc[0])
    assert "red" not in qv.dtype.names and (qv["label"] == _read(parts[0])[3]).all()
