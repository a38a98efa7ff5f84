"""GPU: csrc/mesh_eval.hip (ops.nearest_points, ops.frustum_seen) and dns_slam_amd/evaluation.py against the host reference
tests/mesh_eval_ref.py."""
import functools

import numpy as np
import pytest
import torch

import mesh_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    ref, q = R.CLOUDS[name]()
    d, i = R.nearest(ref, q)
    for a in (ref, q, d, i):
        a.setflags(write=False)
    return ref, q, d, i


def _check_nearest(ref, q, d_ref, dist, idx, what):
    """|dist - ref| <= 2^-20 ref; the float64 distance to ref[idx] within the same bound of the reference distance."""
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    assert dist.shape == d_ref.shape and idx.shape == d_ref.shape
    assert (idx >= 0).all() and (idx < len(ref)).all(), what
    err = np.abs(dist - d_ref)
    worst = (err / np.maximum(d_ref, 1e-300)).max() if len(d_ref) else 0.0
    print(f"{what}: worst |dist - ref| / ref = {worst / 2.0 ** -24:.2f} units of 2^-24")
    assert (err <= R.DIST_RTOL * d_ref).all(), f"{what}: {worst / 2.0 ** -24:.2f} units of 2^-24"
    d_idx = np.linalg.norm(ref.astype(np.float64)[idx] - q.astype(np.float64), axis=1)
    assert (np.abs(d_idx - d_ref) <= R.DIST_RTOL * d_ref).all(), f"{what}: idx does not point at a nearest point"


@pytest.mark.parametrize("name", sorted(R.CLOUDS))
def test_nearest_points_clouds(name):
    from dns_slam_amd import ops
    ref, q, d_ref, _ = _cloud(name)
    r, qq = _dev(ref), _dev(q)
    dist, idx, stats = ops.nearest_points(r, qq, return_stats=True)
    print(f"{name}: M {len(ref)}, N {len(q)}, {stats}")
    _check_nearest(ref, q, d_ref, dist, idx, name)
    dist2, idx2 = ops.nearest_points(r, qq)
    assert torch.equal(dist.view(torch.int32), dist2.view(torch.int32)), "dist differs between two calls"
    assert torch.equal(idx, idx2)
    if name == "lattice":
        assert stats["cells"] == 32 ** 3                     # the premise: lattice points on cell boundaries
    if name in ("lattice", "copies"):
        n0 = 17 ** 3 if name == "lattice" else len(q)
        assert (dist[:n0] == 0).all()
    if name == "clusters":
        assert 0 < stats["brute_queries"] < len(q)           # the far queries took the all-pairs pass, the inner ones did not
    if name in ("single", "identical"):
        assert stats["cells"] == 1


@pytest.mark.parametrize("name", ["uniform", "clusters", "lattice", "coplanar"])
def test_nearest_points_paths_agree(name):
    """The grid, the grid cut off after its first cell (every other query finished by the all-pairs pass) and the all-pairs
    kernel alone return the same distances and indices, bit for bit."""
    from dns_slam_amd import ops
    ref, q, d_ref, _ = _cloud(name)
    r, qq = _dev(ref), _dev(q)
    dist, idx = ops.nearest_points(r, qq)
    d0, i0, s0 = ops.nearest_points(r, qq, max_rings=0, return_stats=True)
    db, ib, sb = ops.nearest_points(r, qq, method="brute", return_stats=True)
    assert sb["brute_queries"] == len(q) and 0 < s0["brute_queries"] <= len(q)
    _check_nearest(ref, q, d_ref, db, ib, name + " (brute)")
    for d, i in ((d0, i0), (db, ib)):
        assert torch.equal(dist.view(torch.int32), d.view(torch.int32)) and torch.equal(idx, i)


def test_nearest_points_sizes():
    from dns_slam_amd import ops
    rng = np.random.default_rng(7)
    for M in R.SIZES_M:
        for N in R.SIZES_N:
            ref, q = rng.normal(size=(M, 3)).astype(np.float32), rng.normal(size=(N, 3)).astype(np.float32)
            dist, idx = ops.nearest_points(_dev(ref), _dev(q))
            _check_nearest(ref, q, R.nearest(ref, q)[0], dist, idx, f"M {M} N {N}")


def test_nearest_points_arguments():
    from dns_slam_amd import ops
    ref = torch.rand(10, 3, device=DEV)
    dist, idx = ops.nearest_points(ref, torch.zeros(0, 3, device=DEV))
    assert dist.shape == (0,) and dist.dtype == torch.float32 and idx.shape == (0,) and idx.dtype == torch.int32
    with pytest.raises(ValueError):
        ops.nearest_points(torch.zeros(0, 3, device=DEV), ref)
    for where in ("ref", "query"):
        for bad in (float("nan"), float("inf")):
            a, b = torch.rand(100, 3, device=DEV), torch.rand(70, 3, device=DEV)
            (a if where == "ref" else b)[33, 1] = bad
            with pytest.raises(ValueError, match=where):
                ops.nearest_points(a, b)
    with pytest.raises(ValueError):
        ops.nearest_points(torch.rand(10, 3), torch.rand(10, 3))
    with pytest.raises(ValueError):
        ops.nearest_points(ref, torch.rand(10, 2, device=DEV))


# ---- sampling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SAMPLING_CASES))
def test_sample_surface(name):
    from dns_slam_amd import evaluation as E
    v, f, u = R.sampling_case(name)
    p_ref, f_ref, cdf, pick = R.sample_surface(v, f, u)
    pts, face = E.sample_surface(_dev(v), _dev(f), len(u), u=_dev(u))
    assert pts.dtype == torch.float32 and pts.shape == (len(u), 3) and face.dtype == torch.int64 and face.shape == (len(u),)
    pts, face = pts.cpu().numpy(), face.cpu().numpy()
    out = R.sample_ambiguous(cdf, pick)
    assert out.mean() <= 1e-4
    ok = ~out
    assert np.array_equal(face[ok], f_ref[ok])
    p32 = p_ref.astype(np.float32)
    assert (np.abs(pts[ok].astype(np.float64) - p32[ok]) <= np.spacing(np.abs(p32[ok]))).all()
    assert (R.face_areas(v, f)[face] > 0).all()
    assert R.barycentric_min(v, f, pts, face).min() >= -1e-6


def test_sample_surface_generator_and_refusals():
    from dns_slam_amd import evaluation as E
    v, f = (_dev(a) for a in R.plane(4, 0.5))
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    a, fa = E.sample_surface(v, f, 1000, generator=g)
    g.manual_seed(5)
    b, fb = E.sample_surface(v, f, 1000, generator=g)
    assert torch.equal(a, b) and torch.equal(fa, fb)
    assert (a[:, 2] == 0.5).all() and a[:, :2].min() >= 0 and a[:, :2].max() <= 1
    assert torch.unique(fa).numel() == f.shape[0]            # 1000 draws over 32 equal faces
    with pytest.raises(ValueError):
        E.sample_surface(v, f[:0], 10)
    with pytest.raises(ValueError):
        E.sample_surface(v, torch.zeros(3, 3, dtype=torch.int32, device=DEV), 10)      # total area 0


# ---- frustum / cull ----------------------------------------------------------------------------------------------------
def test_frustum_seen_and_cull_mesh():
    from dns_slam_amd import evaluation as E, ops
    v, f = R.sphere(0.6, 32)
    c2w = R.frustum_poses()
    cam = R.FRUSTUM_CAM
    w2c = R.world_to_camera(c2w)
    seen_ref, near = R.check_proj(v, w2c, **cam)
    assert near.mean() <= 0.01
    vd, fd = _dev(v), _dev(f)
    seen = ops.frustum_seen(vd, _dev(w2c), cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    assert seen.dtype == torch.bool and seen.shape == (len(v),)
    s = seen.cpu().numpy()
    assert np.array_equal(s[~near], seen_ref[~near])
    # each pose alone
    for k in range(len(w2c)):
        sk = ops.frustum_seen(vd, _dev(w2c[k:k + 1]), cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]).cpu().numpy()
        rk, nk = R.check_proj(v, w2c[k:k + 1], **cam)
        assert np.array_equal(sk[~nk], rk[~nk])
    # K = 0 sees nothing
    assert not ops.frustum_seen(vd, torch.zeros(0, 4, 4, device=DEV), 68, 120, 60.0, 60.0, 59.5, 33.5).any()
    # the face rule and compact=True, exactly, given the vertex mask
    v1, f1 = E.cull_mesh(vd, fd, c2w, **cam)
    keep = s[f].any(1)
    assert torch.equal(v1, vd) and np.array_equal(f1.cpu().numpy(), f[keep]) and 0 < keep.sum() < len(f)
    v2, f2 = E.cull_mesh(vd, fd, torch.as_tensor(c2w), compact=True, **cam)
    used = np.zeros(len(v), bool)
    used[f[keep].ravel()] = True
    assert np.array_equal(v2.cpu().numpy(), v[used])
    assert f2.dtype == torch.int32 and np.array_equal(v2.cpu().numpy()[f2.cpu().numpy()], v[f[keep]])
    v3, f3 = E.cull_mesh(vd, fd, np.zeros((0, 4, 4)), **cam)
    assert f3.shape == (0, 3) and torch.equal(v3, vd)
    # flip_yz=False with the columns negated beforehand is the same cull
    flipped = c2w.copy()
    flipped[:, :3, 1:3] *= -1.0
    assert torch.equal(E.cull_mesh(vd, fd, flipped, flip_yz=False, **cam)[1], f1)


def test_frustum_seen_many_poses():
    """More poses than one LDS tile holds (128), the only seeing pose last: the tiles are walked to the end."""
    from dns_slam_amd import ops
    v, _ = R.sphere(0.6, 32)
    cam = R.FRUSTUM_CAM
    c2w = R.frustum_poses(1)
    away = np.tile(np.eye(4), (300, 1, 1))
    away[:, :3, 3] = [50.0, 0.0, 0.0]
    away[:, :3, :3] = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])     # far outside, looking along +x, away from the sphere
    w2c = R.world_to_camera(np.concatenate((away, c2w)))
    ref_all, near = R.check_proj(v, w2c, **cam)
    ref_last, _ = R.check_proj(v, w2c[-1:], **cam)
    assert np.array_equal(ref_all, ref_last) and ref_all.any()
    s = ops.frustum_seen(_dev(v), _dev(w2c), cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]).cpu().numpy()
    assert np.array_equal(s[~near], ref_all[~near])


# ---- metrics -----------------------------------------------------------------------------------------------------------
def test_metrics_3d_two_spheres():
    """metrics_3d equals the host reference on the same samples: the means to the distance bound, the ratio up to the samples
    whose reference distance lies within the bound of the threshold."""
    from dns_slam_amd import evaluation as E
    (vr, fr), (vg, fg) = R.sphere(0.57, 32), R.sphere(0.6, 32)
    n, th = 6000, 0.032
    rng = np.random.default_rng(9)
    u_rec, u_gt = rng.random((n, 3)), rng.random((n, 3))
    dv = [_dev(a) for a in (vr, fr, vg, fg)]
    m = E.metrics_3d(*dv, n_samples=n, dist_th=th, u_rec=_dev(u_rec), u_gt=_dev(u_gt))
    rec = E.sample_surface(dv[0], dv[1], n, u=_dev(u_rec))[0]
    gt = E.sample_surface(dv[2], dv[3], n, u=_dev(u_gt))[0]
    rec_h, gt_h = rec.cpu().numpy(), gt.cpu().numpy()
    acc, comp = R.accuracy(gt_h, rec_h) * 100, R.completion(gt_h, rec_h) * 100
    d = R.nearest(rec_h, gt_h)[0]
    ratio = (d < th).mean() * 100
    unsure = (np.abs(d - th) <= R.DIST_RTOL * d).sum()
    print(f"device {m}; host accuracy {acc:.6f} cm, completion {comp:.6f} cm, ratio {ratio:.4f} % ({unsure} at the threshold)")
    assert abs(m["accuracy_cm"] - acc) <= R.DIST_RTOL * acc
    assert abs(m["completion_cm"] - comp) <= R.DIST_RTOL * comp
    assert abs(m["completion_ratio_pct"] - ratio) <= unsure / n * 100 + 1e-9
    assert 1.0 < ratio < 99.0 and 2.9 < acc < 3.6
    # the three metrics one by one, argument order as in the reference
    assert abs(float(E.accuracy(gt, rec)) * 100 - acc) <= R.DIST_RTOL * acc
    assert abs(float(E.completion(gt, rec)) * 100 - comp) <= R.DIST_RTOL * comp
    assert abs(float(E.completion_ratio(gt, rec, th)) * 100 - ratio) <= unsure / n * 100 + 1e-9
    assert E.accuracy(gt, rec).dtype == torch.float64
    # seeded draws: the same seed gives the same figures
    a, b = E.metrics_3d(*dv, n_samples=2000, seed=3), E.metrics_3d(*dv, n_samples=2000, seed=3)
    assert a == b and set(a) == {"accuracy_cm", "completion_cm", "completion_ratio_pct"}
    with pytest.raises(NotImplementedError):
        E.metrics_3d(*dv, n_samples=100, align=True)


@pytest.mark.parametrize("seed", [0, 1])
def test_metrics_3d_two_planes(seed):
    from dns_slam_amd import evaluation as E
    (v0, f0), (v1, f1) = R.plane(16, 0.0), R.plane(12, 0.03)
    m = E.metrics_3d(_dev(v0), _dev(f0), _dev(v1), _dev(f1), n_samples=20000, seed=seed)
    print(m)
    assert 3.0 <= m["accuracy_cm"] <= 3.1 and 3.0 <= m["completion_cm"] <= 3.1
    assert m["completion_ratio_pct"] == 100.0
