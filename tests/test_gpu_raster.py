"""GPU: csrc/mesh_raster.hip (ops.rasterize_depth, ops.depth_l1, ops.views_see_any) and the Depth L1 functions of
dns_slam_amd/evaluation.py against the host reference tests/raster_ref.py."""
import functools

import numpy as np
import pytest
import torch

import mesh_eval_ref as M
import raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METHODS = ("auto", "simple")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _cam(cam):
    return cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]


@functools.lru_cache(maxsize=None)
def _gpu(name, method="auto"):
    """The kernel's images of a scene (numpy [V,H,W] fp32) and the stats, computed once."""
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    d, st = ops.rasterize_depth(_dev(v), _dev(f), _dev(w2c), *_cam(cam), method=method, return_stats=True)
    return d.cpu().numpy(), st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", R.SCENES)
def test_against_reference(name, method):
    r = R.render(name)
    d, _ = _gpu(name, method)
    assert d.shape == r["D"].shape and (d >= 0).all()
    x = np.where(d == 0, np.inf, d.astype(np.float64))                        # 0 reads as +inf
    rt = R.DEPTH_RTOL
    lo, hi = r["D_grown"] * (1 - rt), r["D_shrunk"] * (1 + rt)
    bad = ~((x >= lo) & (x <= hi))
    print(f"{name}/{method}: {bad.sum()} pixels outside the sandwich")
    assert not bad.any(), np.argwhere(bad)[:5]
    un, hit = r["unambiguous"], np.isfinite(r["D"])
    m = un & hit
    if m.any():
        rel = np.abs(x[m] - r["D"][m]) / r["D"][m]
        print(f"{name}/{method}: worst relative error on unambiguous pixels {rel.max():.3e} (bound {rt:.3e})")
        assert (rel <= rt).all()
    assert (d[un & ~hit] == 0).all() and (_bits(d[un & ~hit]) == 0).all()    # the background is exactly +0


def test_lattice_has_no_hole():
    L = R.LATTICE
    for method in METHODS:
        d = _gpu("lattice", method)[0][0]
        inside = np.zeros(d.shape, bool)
        inside[L["i0"]:L["i0"] + L["ny"] + 1, L["j0"]:L["j0"] + L["nx"] + 1] = True
        assert (d[inside] == 2.0).all() and (d[~inside] == 0).all()


@pytest.mark.parametrize("name", R.SCENES)
def test_methods_calls_stacks_and_list_cap_agree_bit_for_bit(name):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    vd, fd, wd = _dev(v), _dev(f), _dev(w2c)
    a = _gpu(name, "auto")[0]
    assert np.array_equal(_bits(a), _bits(_gpu(name, "simple")[0]))
    again = ops.rasterize_depth(vd, fd, wd, *_cam(cam)).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(again))
    for k in range(len(w2c)):
        one = ops.rasterize_depth(vd, fd, wd[k:k + 1], *_cam(cam)).cpu().numpy()
        assert np.array_equal(_bits(a[k:k + 1]), _bits(one))
    # a small list: the (triangle, view) pairs cut into many launches, by triangle range and by view
    for cap in (700, max(len(f), 1)):
        d, st = ops.rasterize_depth_launch(vd, fd, wd, *_cam(cam), list_cap=cap)
        assert np.array_equal(_bits(a), _bits(d.cpu().numpy())) and int(st[0]) == 0
        assert int(st[1]) == _gpu(name, "auto")[1]["large"]


def test_stats_show_the_path():
    room, sphere = _gpu("room")[1], _gpu("sphere")[1]
    assert room["large"] > 0 and room["small"] == 0 and not room["nonfinite"]
    assert sphere["small"] > 1000 and sphere["large"] == 0
    simple = _gpu("room", "simple")[1]
    assert simple["large"] == 0 and simple["small"] == room["large"]
    soup = _gpu("soup")[1]
    assert soup["large"] > 0 and soup["small"] > 0
    assert _gpu("empty")[1] == {"nonfinite": False, "large": 0, "small": 0}


@pytest.mark.parametrize("method", METHODS)
def test_nan_vertex_is_flagged_and_skipped(method):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene("soup")
    k = int(f[17, 1])
    v2 = v.copy()
    v2[k, 1] = np.nan
    d, st = ops.rasterize_depth(_dev(v2), _dev(f), _dev(w2c), *_cam(cam), method=method, return_stats=True)
    assert st["nonfinite"]
    keep = ~(f == k).any(1)
    assert 0 < (~keep).sum() < 5
    want, st2 = ops.rasterize_depth(_dev(v), _dev(f[keep]), _dev(w2c), *_cam(cam), method=method, return_stats=True)
    assert not st2["nonfinite"]
    assert torch.equal(d.view(torch.int32), want.view(torch.int32))
    v3 = v.copy()
    v3[k, 0] = np.inf
    assert ops.rasterize_depth(_dev(v3), _dev(f), _dev(w2c), *_cam(cam), method=method, return_stats=True)[1]["nonfinite"]


def test_refused_arguments():
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene("room")
    for bad in (8, -1):
        f2 = f.copy()
        f2[5, 2] = bad
        with pytest.raises(ValueError):
            ops.rasterize_depth(_dev(v), _dev(f2), _dev(w2c), *_cam(cam))
    with pytest.raises(ValueError):
        ops.rasterize_depth(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(w2c), *_cam(cam))
    with pytest.raises(ValueError):
        ops.rasterize_depth(_dev(v), _dev(f), _dev(w2c), *_cam(cam), method="fast")
    with pytest.raises(ValueError):
        ops.rasterize_depth(_dev(v), _dev(f), _dev(w2c), *_cam(cam), z_near=0.0)
    with pytest.raises(ValueError):
        ops.depth_l1(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        ops.views_see_any(torch.zeros(5, 3), torch.zeros(2, 4, 4), 68, 120, 60.0, 60.0, 59.5, 33.5)
    # the kernel's own guard: the launch form skips the face and flags it
    f2 = f.copy()
    f2[5, 2] = 8
    d, st = ops.rasterize_depth_launch(_dev(v), _dev(f2), _dev(w2c), *_cam(cam))
    assert int(st[0]) & 2
    assert ops.rasterize_depth(_dev(v), _dev(f), torch.zeros(0, 4, 4, device=DEV), *_cam(cam)).shape == (0, cam["H"], cam["W"])


# ---- depth L1 ------------------------------------------------------------------------------------------------------------------
def test_depth_l1():
    from dns_slam_amd import ops
    a = torch.from_numpy(_gpu("soup")[0]).to(DEV)
    v, f, w2c, cam = R.scene("soup")
    b = ops.rasterize_depth(_dev(v * np.float32(1.03)), _dev(f), _dev(w2c), *_cam(cam))
    e = ops.depth_l1(a, b)
    assert e.dtype == torch.float64 and e.shape == (len(w2c),)
    want = np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64)).mean(axis=(1, 2))
    assert (want > 0).all()
    assert np.abs(e.cpu().numpy() - want).max() <= 1e-12 * want.max()
    assert torch.equal(e.view(torch.int64), ops.depth_l1(a, b).view(torch.int64))
    assert (ops.depth_l1(a, a) == 0).all()
    assert ops.depth_l1(a[:0], b[:0]).shape == (0,)
    # the lattice moved from z = 2 to z = 2.5 (vertices scaled by 1.25: the same pixels): |2.5 - 2| on 25 x 17 of 96 x 80 pixels
    lv, lf = R.lattice_mesh()
    _, _, lw, lcam = R.scene("lattice")
    near = ops.rasterize_depth(_dev(lv), _dev(lf), _dev(lw[:1]), *_cam(lcam))
    far = ops.rasterize_depth(_dev(lv * np.float32(1.25)), _dev(lf), _dev(lw[:1]), *_cam(lcam))
    assert float(ops.depth_l1(near, far)[0]) == 0.5 * 25 * 17 / (96 * 80)
    odd = torch.rand(3, 37, 50, device=DEV), torch.rand(3, 37, 50, device=DEV)        # a pixel count that is no multiple of 256
    want = (odd[0].double() - odd[1].double()).abs().mean(dim=(1, 2))
    assert ((ops.depth_l1(*odd) - want).abs() <= 1e-12 * want).all()


# ---- the view sampler ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (40, 0, 129))
def test_views_see_any_against_frustum_seen(K):
    from dns_slam_amd import evaluation as E, ops
    cam = M.FRUSTUM_CAM
    rng = np.random.default_rng(5)
    pts = _dev((rng.normal(size=(700, 3)) * 0.3 + np.array([0.0, 0.0, 1.5])).astype(np.float32))
    c2w = M.frustum_poses(K, seed=3) if K else np.zeros((0, 4, 4))
    if K:
        c2w[:, :3, 3] *= 8.0                                      # centres within 1.6 of the origin: some poses see nothing
    w2c = _dev(E.world_to_camera(c2w)) if K else torch.zeros(0, 4, 4, device=DEV)
    args = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    sees = ops.views_see_any(pts, w2c, *args)
    assert sees.shape == (K,) and sees.dtype == torch.bool
    want = [bool(ops.frustum_seen(pts, w2c[k:k + 1], *args).any()) for k in range(K)]
    assert sees.cpu().tolist() == want
    if K:
        assert 0 < sum(want) < K
        assert not ops.views_see_any(pts[:0], w2c, *args).any()


def test_sample_views_rejects_views_of_the_unseen_cloud():
    from dns_slam_amd import evaluation as E
    rng = np.random.default_rng(9)
    unseen = (rng.normal(size=(400, 3)) * 0.2 + np.array([3.0, 0.0, 0.0])).astype(np.float32)       # a blob beside the box
    extents, transform = np.array([1.0, 1.0, 1.0]), np.eye(4)
    cam = dict(H=68, W=120, fx=60.0, fy=60.0, cx=59.5, cy=33.5)
    a = E.sample_views(extents, transform, 50, unseen_pts=_dev(unseen), cam=cam, seed=2, batch=32)
    assert a.shape == (50, 4, 4)
    assert np.array_equal(a, E.sample_views(extents, transform, 50, unseen_pts=_dev(unseen), cam=cam, seed=2, batch=32))
    for m in a:
        seen, near = M.check_proj(unseen, M.world_to_camera(m[None]), cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        assert not (seen & ~near).any()
    plain = E.sample_views(extents, transform, 50, seed=2)
    assert not np.array_equal(a, plain)                           # something was rejected
    assert (np.abs(a[:, :3, 3]) <= 0.5).all()


# ---- the metric ----------------------------------------------------------------------------------------------------------------
def test_calc_2d_metric_against_the_reference_images():
    """A coarse sphere (the reference is brute force: 16 images of it cost what one of the 5000-triangle sphere does) against a
    copy scaled by 1.02 about its centre, 8 views of 64 x 64.  The kernel's image lies in [D_grown (1 - rtol), D_shrunk (1 + rtol)]
    per pixel (a pixel only D_grown covers may also be background), so each |d_gt - d_rec| lies between the distance of the two
    intervals and their farthest ends; the means of those bound the metric."""
    from dns_slam_amd import evaluation as E
    c = np.array([0.2, -0.1, 0.3])
    gv, gf = R.uv_sphere(0.5, c, 16, 20)
    rv = ((gv.astype(np.float64) - c) * 1.02 + c).astype(np.float32)
    box = (np.array([0.4, 0.4, 0.4]), np.array([[1, 0, 0, c[0]], [0, 1, 0, c[1]], [0, 0, 1, c[2]], [0, 0, 0, 1.0]]))    # inside it
    kw = dict(n_imgs=8, seed=1, box=box, H=64, W=64, focal=40.0)
    out = E.calc_2d_metric(_dev(rv), _dev(gf), _dev(gv), _dev(gf), align=False, **kw)
    assert out["per_view"].shape == (8,) and out["depth_l1_cm"] == pytest.approx(out["per_view"].mean() * 100.0, rel=1e-14)
    assert np.array_equal(out["c2w"], E.sample_views(*box, 8, seed=1))
    w2c = R.w2c_f32(out["c2w"])
    rt, zf = R.DEPTH_RTOL, 20.0

    def interval(verts, m):
        r = R.render_view(verts, gf, m, 64, 64, 40.0, 40.0, 31.5, 31.5)
        lo = np.where(np.isinf(r["D_shrunk"]), 0.0, r["D_grown"] * (1 - rt))          # may be background: 0
        hi = np.where(np.isinf(r["D_grown"]), 0.0, np.where(np.isinf(r["D_shrunk"]), zf, r["D_shrunk"] * (1 + rt)))
        return lo, hi

    n_hit = 0
    for k in range(8):
        (alo, ahi), (blo, bhi) = interval(gv, w2c[k]), interval(rv, w2c[k])
        least = np.maximum(np.maximum(alo - bhi, blo - ahi), 0.0).mean()
        most = np.maximum(ahi - blo, bhi - alo).mean()
        print(f"view {k}: {least:.9f} <= {out['per_view'][k]:.9f} <= {most:.9f}")
        assert least <= out["per_view"][k] <= most
        n_hit += int((ahi > 0).sum())
    assert n_hit == 8 * 64 * 64                                   # seen from inside: every pixel is hit
    aligned = E.calc_2d_metric(_dev(rv), _dev(gf), _dev(gv), _dev(gf), align=True, **kw)
    assert np.isfinite(aligned["depth_l1_cm"]) and aligned["transformation"].shape == (4, 4)
