"""CPU: the host reference of the depth rasteriser (tests/raster_ref.py) against closed forms and its own conditions, and the
host-side functions of the Depth L1 metric (evaluation.view_box / look_at / sample_views)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_ref as R                                       # noqa: E402


def test_lattice_is_exactly_two_with_no_hole():
    r = R.render("lattice")
    L = R.LATTICE
    inside = np.zeros(r["D"].shape[1:], bool)
    inside[L["i0"]:L["i0"] + L["ny"] + 1, L["j0"]:L["j0"] + L["nx"] + 1] = True
    assert (r["D"][0][inside] == 2.0).all()                  # every pixel centre inside lies on an edge or a vertex
    assert np.isinf(r["D"][0][~inside]).all()
    assert (R.render_f32("lattice")[0][inside] == 2.0).all()
    assert np.isfinite(r["D"][1]).sum() > 300                # the shifted view sees the grid's interior


def test_room_equals_the_ray_box_distance():
    v, f, w2c, cam = R.scene("room")
    assert len(f) == 12
    D = R.render("room")["D"]
    for k in range(len(w2c)):
        a = R.room_depth_analytic(w2c[k], cam)
        assert np.isfinite(D[k]).all()
        assert np.abs(D[k] - a).max() <= 1e-6 * a.max()      # the fp32 rounding of the camera-space vertices
    # every triangle is larger than the image, several reach behind the camera
    z = np.stack([R.camera_vertices_f32(v, m)[:, 2][f] for m in w2c])
    assert ((z.min(2) < 0) & (z.max(2) > 0)).sum() >= 6


@pytest.mark.parametrize("name", R.SCENES)
def test_reference_conditions(name):
    r = R.render(name)
    assert (r["D_grown"] <= r["D"]).all() and (r["D"] <= r["D_shrunk"]).all()
    amb = 1.0 - r["unambiguous"].mean()
    print(f"{name}: ambiguous pixels {amb:.4%}")
    assert amb <= 0.05
    if name in ("behind", "empty"):
        assert np.isinf(r["D_grown"]).all()


def test_depth_rtol_is_four_times_the_measured_error():
    """The fp32 restatement against D on the unambiguous pixels of all scenes; and it meets the sandwich the GPU test asks of
    the kernel on EVERY pixel (a condition on the reference: a scene where fp32 arithmetic itself cannot meet it would test
    nothing about the kernel)."""
    worst = 0.0
    for name in R.SCENES:
        r, d = R.render(name), R.render_f32(name).astype(np.float64)
        m = r["unambiguous"] & np.isfinite(r["D"])
        if m.any():
            worst = max(worst, float((np.abs(d[m] - r["D"][m]) / r["D"][m]).max()))
        assert np.isinf(d[r["unambiguous"] & np.isinf(r["D"])]).all()
        assert ((d >= r["D_grown"] * (1 - R.DEPTH_RTOL)) & (d <= r["D_shrunk"] * (1 + R.DEPTH_RTOL))).all(), name
    print(f"worst relative difference of the fp32 restatement: {worst:.4e}")
    assert 0.5 * R.DEPTH_ERR_MEASURED <= worst <= R.DEPTH_ERR_MEASURED
    assert R.DEPTH_RTOL == 4.0 * R.DEPTH_ERR_MEASURED


def test_scene_contents():
    v, f, w2c, cam = R.scene("soup")
    assert len(f) == 2000
    z = R.camera_vertices_f32(v, w2c[0])[:, 2][f]
    assert ((z.min(1) < 0.01) & (z.max(1) > 0.01)).sum() > 50 and (z.min(1) > 20.0).sum() > 5
    assert (f[:, 0] == f[:, 2]).sum() == 50
    assert len(np.unique(np.sort(f, 1), axis=0)) <= len(f) - 50 + 5
    assert 4500 <= len(R.scene("sphere")[1]) <= 5500
    for name in R.SCENES:
        _, f, w2c, cam = R.scene(name)
        assert 2 <= len(w2c) <= 4 and cam["H"] <= 80 and cam["W"] <= 96 and len(f) <= 5500


# ---- evaluation: the host side of the view sampler -------------------------------------------------------------------------
def test_view_box_on_a_hand_checked_box():
    from dns_slam_amd import evaluation as E
    v = np.array([[-1.0, 0.0, 2.0], [3.0, 2.0, 2.5], [0.0, 1.0, 4.0]])
    extents, transform = E.view_box(v)
    assert np.allclose(extents, [4.0 * 0.3, 2.0 * 0.7, 2.0 * 0.7], rtol=0, atol=1e-15)
    want = np.eye(4)
    want[:3, 3] = [1.0, 1.0, 3.0 + 0.4]
    assert np.allclose(transform, want, rtol=0, atol=1e-15)


def test_look_at_is_the_reference_viewmatrix():
    from dns_slam_amd import evaluation as E
    o, tgt = np.array([1.0, 2.0, 0.5]), np.array([4.0, 6.0, 0.5])
    m = E.look_at(o, tgt)
    assert np.allclose(m[:3, 2], [0.6, 0.8, 0.0]) and np.allclose(m[:3, 3], o) and np.allclose(m[3], [0, 0, 0, 1])
    # x = normalize(up x z) with up = (0, 0, -1); y = z x x: world down (0, 0, -1) for a level camera
    assert np.allclose(m[:3, 0], [0.8, -0.6, 0.0]) and np.allclose(m[:3, 1], [0.0, 0.0, -1.0])
    assert np.allclose(m[:3, :3].T @ m[:3, :3], np.eye(3), atol=1e-14) and np.linalg.det(m[:3, :3]) > 0
    z = tgt - o                                                   # viewmatrix(z, up, pos) written out
    v2 = z / np.linalg.norm(z)
    v0 = np.cross([0, 0, -1.0], v2)
    v0 /= np.linalg.norm(v0)
    v1 = np.cross(v2, v0)
    v1 /= np.linalg.norm(v1)
    assert np.array_equal(m[:3], np.stack([v0, v1, v2, o], 1))


def test_sample_views_without_rejection():
    from dns_slam_amd import evaluation as E
    extents = np.array([1.2, 1.4, 0.7])
    transform = np.eye(4)
    transform[:3, :3] = R._rot((0, 0, 1), 30.0)
    transform[:3, 3] = [1.0, -2.0, 0.4]
    a = E.sample_views(extents, transform, 40, seed=3)
    b = E.sample_views(extents, transform, 40, seed=3)
    c = E.sample_views(extents, transform, 40, seed=4)
    assert a.shape == (40, 4, 4) and a.dtype == np.float64
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    local = (a[:, :3, 3] - transform[:3, 3]) @ transform[:3, :3]          # back into the box frame
    assert (np.abs(local) <= 0.5 * extents + 1e-12).all()
    assert local.std(0).min() > 0.1 * extents.min()
    # the first view from the generator's stream, by hand
    rs = np.random.RandomState(3)
    origin = transform[:3, :3] @ ((rs.rand(3) - 0.5) * extents) + transform[:3, 3]
    target = np.round(rs.uniform(-10000.0, 10000.0, 3), 2)
    assert np.array_equal(a[0], E.look_at(origin, target))
    assert np.allclose(np.einsum("nij,nik->njk", a[:, :3, :3], a[:, :3, :3]), np.eye(3), atol=1e-12)
    assert E.sample_views(extents, transform, 0).shape == (0, 4, 4)
