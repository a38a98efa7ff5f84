"""GPU: csrc/mesh_render.hip (ops.render_mesh), dns_slam_amd/visualize.py and tools/visualize.py against the host reference
tests/mesh_render_ref.py, on the shared scenes of tests/raster_ref.py."""
import functools
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import mesh_render_ref as M
import raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METHODS = ("auto", "simple")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _cam(cam):
    return cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32))
               for k in ("color", "depth", "index"))


@functools.lru_cache(maxsize=None)
def _gpu(name, cull=None, method="auto", shade=None):
    """The kernel's images of all views of a scene, computed once (numpy)."""
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    return _np(ops.render_mesh(_dev(v), _dev(f), _dev(M.scene_colors(name)), _dev(w2c), *_cam(cam), cull=cull, shade=shade,
                               method=method, stats=True))


# ---- 1. reference parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shade", M.SHADES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("cull", M.CULLS)
@pytest.mark.parametrize("name,views", M.PARITY)
def test_against_reference(name, views, cull, method, shade):
    out = _gpu(name, cull, method, shade)
    assert out["color"].dtype == np.float32 and out["depth"].dtype == np.float32 and out["index"].dtype == np.int32
    assert int(out["status"][0]) == 0
    for view in views:
        ref = M.render(name, view)[cull]
        r = M.compare(ref, out["index"][view], out["depth"][view], out["color"][view], shade)
        print(f"{name}/{view}/{cull}/{method}/{shade}: {r}")
        assert r["bad_index"] == 0, "the index differs from the reference's triangle at an unambiguous pixel"
        assert r["bad_color"] == 0, "a colour outside the derived bound"
        assert r["bad_depth"] == 0, "a depth outside raster_ref.DEPTH_RTOL"
        if r["covered"]:
            assert r["compared"] >= M.MIN_COMPARED * r["covered"]
        bg = out["index"][view] == -1
        assert (out["color"][view][bg] == 1.0).all() and (out["depth"][view][bg].view(np.uint32) == 0).all()


# ---- 2. the depth image is rasterize_depth's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", R.SCENES)
def test_depth_is_rasterize_depth_bit_for_bit(name, method):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    out = _gpu(name, None, method)
    d, st = ops.rasterize_depth(_dev(v), _dev(f), _dev(w2c), *_cam(cam), method=method, return_stats=True)
    assert np.array_equal(out["depth"].view(np.uint32), d.cpu().numpy().view(np.uint32))
    assert np.array_equal(out["index"] == -1, out["depth"] == 0)
    assert (out["index"] >= -1).all() and (out["index"] < max(len(f), 1)).all()
    assert [int(x) for x in out["status"][:3]] == [0, st["large"], st["small"]]


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cull,shade", [("room", None, "headlight"), ("sphere", "back", None), ("lattice", "front", "headlight"),
                                             ("soup", None, None), ("behind", None, None), ("empty", None, "headlight")])
def test_calls_methods_stacks_and_list_cap_agree_bit_for_bit(name, cull, shade):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    p, pc = M.actor_cloud(M.ACTOR_FRONT)
    kw = dict(cull=cull, shade=shade, points=_dev(p), point_colors=_dev(pc), point_size=3)
    args = (_dev(v), _dev(f), _dev(M.scene_colors(name)))
    a = _np(ops.render_mesh(*args, _dev(w2c), *_cam(cam), **kw))
    assert _same_bits(a, _np(ops.render_mesh(*args, _dev(w2c), *_cam(cam), **kw)))
    assert _same_bits(a, _np(ops.render_mesh(*args, _dev(w2c), *_cam(cam), method="simple", **kw)))
    for k in range(len(w2c)):
        one = _np(ops.render_mesh(*args, _dev(w2c[k:k + 1]), *_cam(cam), **kw))
        assert _same_bits({q: a[q][k:k + 1] for q in a}, one)
    for cap in (700, max(len(f), 1)):                             # the pairs cut into many launches, by triangle range and by view
        b = _np(ops.render_mesh(*args, _dev(w2c), *_cam(cam), list_cap=cap, **kw))
        assert _same_bits(a, b) and np.array_equal(a["status"], b["status"])


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ("sphere", "room", "soup"))
def test_of_two_copies_of_a_face_the_lower_index_wins(name, method):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene(name)
    col = _dev(M.scene_colors(name))
    single = _gpu(name, None, method)
    for order in (np.concatenate((f, f)), np.concatenate((f[::-1], f[::-1]))):
        two = _np(ops.render_mesh(_dev(v), _dev(order), col, _dev(w2c), *_cam(cam), method=method))
        assert (two["index"] < len(f)).all()                      # never the upper copy
        assert np.array_equal(two["depth"].view(np.uint32), single["depth"].view(np.uint32))
    two = _np(ops.render_mesh(_dev(v), _dev(np.concatenate((f, f))), col, _dev(w2c), *_cam(cam), method=method))
    assert np.array_equal(two["index"], single["index"])
    assert np.array_equal(two["color"].view(np.uint32), single["color"].view(np.uint32))


def test_point_at_a_triangles_depth_loses_to_it():
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene("lattice")                          # view 0: the wall's depth is exactly 2 at every pixel
    pts = np.array([[0.25, 0.0, 2.0], [0.25, -0.25, np.nextafter(np.float32(2.0), np.float32(0.0))]], np.float32)
    pc = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    out = _np(ops.render_mesh(_dev(v), _dev(f), _dev(M.scene_colors("lattice")), _dev(w2c[:1]), *_cam(cam), points=_dev(pts),
                              point_colors=_dev(pc), point_size=4))
    assert (out["depth"][0][25:42, 30:55] > 0).all()
    assert not (out["index"] == -2).any()                         # in the plane: hidden
    assert (out["index"] == -3).sum() == 16                       # one ulp nearer: drawn
    assert (out["color"][out["index"] == -3] == [0, 1, 0]).all()


# ---- 5. points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (1, 4))
@pytest.mark.parametrize("where", ("front", "behind", "border"))
def test_camera_actor_about_a_wall(where, size):
    from dns_slam_amd import ops
    at = {"front": M.ACTOR_FRONT, "behind": M.ACTOR_BEHIND, "border": M.ACTOR_BORDER}[where]
    ref = M.render_actor(at, size)[None]
    v, f, w2c, cam = R.scene("lattice")
    p, c = M.actor_cloud(at)
    out = _np(ops.render_mesh(_dev(v), _dev(f), _dev(M.scene_colors("lattice")), _dev(w2c[1:2]), *_cam(cam), points=_dev(p),
                              point_colors=_dev(c), point_size=size))
    r = M.compare(ref, out["index"][0], out["depth"][0], out["color"][0], None)
    print(f"{where}/{size}: {r}")
    assert r["bad_index"] == 0 and r["bad_depth"] == 0 and r["bad_color"] == 0
    assert r["compared"] >= M.MIN_COMPARED * r["covered"]
    pts, wall = out["index"][0] <= -2, ref["face_index"] >= 0
    if where == "front":
        assert (pts & wall).sum() > 50 * size                     # drawn over the wall
    if where == "behind":
        assert not (pts & wall & ref["unambiguous"]).any() and pts.any()
    if where == "border":
        assert pts[:, 0].any() and not pts[:, -1].any()           # clipped by the left border
    assert int(out["status"][0]) == 0


# ---- 6. bad inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_nan_vertex_and_nan_point_are_flagged_and_skipped(method):
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene("soup")
    col = M.scene_colors("soup")
    p, pc = M.actor_cloud(M.ACTOR_FRONT)
    k = int(f[17, 1])
    v2 = v.copy()
    v2[k, 1] = np.nan
    keep = ~(f == k).any(1)
    kw = dict(points=_dev(p), point_colors=_dev(pc), method=method, shade="headlight")
    got = _np(ops.render_mesh(_dev(v2), _dev(f), _dev(col), _dev(w2c), *_cam(cam), **kw))
    want = _np(ops.render_mesh(_dev(v), _dev(f[keep]), _dev(col), _dev(w2c), *_cam(cam), **kw))
    assert int(got["status"][0]) == 1 and int(want["status"][0]) == 0
    old = np.nonzero(keep)[0]
    want["index"] = np.where(want["index"] >= 0, old[np.maximum(want["index"], 0)], want["index"]).astype(np.int32)
    assert _same_bits(got, want)
    p2, pc2 = np.concatenate((p, [[np.nan, 0, 1]], [[0, np.inf, 1]])).astype(np.float32), np.concatenate((pc, pc[:2]))
    got = _np(ops.render_mesh(_dev(v), _dev(f), _dev(col), _dev(w2c), *_cam(cam), **dict(kw, points=_dev(p2), point_colors=_dev(pc2))))
    want = _np(ops.render_mesh(_dev(v), _dev(f), _dev(col), _dev(w2c), *_cam(cam), **kw))
    assert int(got["status"][0]) == 4 and _same_bits(got, want)


def test_refused_arguments():
    from dns_slam_amd import ops
    v, f, w2c, cam = R.scene("room")
    col = M.scene_colors("room")
    good = (_dev(v), _dev(f), _dev(col), _dev(w2c), *_cam(cam))
    assert ops.render_mesh(*good)["color"].shape == (3, cam["H"], cam["W"], 3)
    for bad in (8, -1):
        f2 = f.copy()
        f2[5, 2] = bad
        with pytest.raises(ValueError):
            ops.render_mesh(_dev(v), _dev(f2), _dev(col), _dev(w2c), *_cam(cam))
    f2 = f.copy()
    f2[5, 2] = 8                                                  # the kernel's own guard: skipped and flagged
    out = ops.render_mesh_launch(_dev(v), _dev(f2), _dev(col), _dev(w2c), *_cam(cam))
    assert int(out["status"][0]) & 2 and not (out["index"] == 5).any()
    with pytest.raises(ValueError):
        ops.render_mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col), torch.from_numpy(w2c), *_cam(cam))
    p = _dev(np.zeros((5, 3), np.float32))
    for kw in (dict(method="fast"), dict(z_near=0.0), dict(z_far=float("inf")), dict(cull="both"), dict(cull="Back"), dict(shade="phong"),
               dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=float("nan")), dict(point_size=0), dict(point_size=17),
               dict(point_size=2.5), dict(points=p), dict(point_colors=p), dict(points=p, point_colors=p[:4]),
               dict(points=p, point_colors=p.double()), dict(points=p[:, :2], point_colors=p), dict(background=(1, 1)),
               dict(points=p.cpu(), point_colors=p)):
        with pytest.raises(ValueError):
            ops.render_mesh(*good, **kw)
    for c in (_dev(col[:-1]), _dev(col).double(), _dev(col)[:, :2], _dev((col * 255).astype(np.uint8)), _dev(col).cpu(), col):
        with pytest.raises(ValueError):
            ops.render_mesh(_dev(v), _dev(f), c, _dev(w2c), *_cam(cam))
    none = ops.render_mesh(_dev(v), _dev(f), _dev(col), torch.zeros(0, 4, 4, device=DEV), *_cam(cam))
    assert none["color"].shape == (0, cam["H"], cam["W"], 3) and none["index"].shape == (0, cam["H"], cam["W"])
    # no mesh at all: the background and the points
    e = ops.render_mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), torch.zeros(0, 3, device=DEV),
                        _dev(w2c[:1]), *_cam(cam), background=(0.25, 0.5, 0.75), points=_dev(np.array([[0, 0, 1.0]], np.float32)),
                        point_colors=_dev(np.array([[1, 0, 0]], np.float32)), point_size=16)
    assert (e["index"] == -2).sum() == 256 and (e["index"] == -1).sum() == cam["H"] * cam["W"] - 256
    assert (e["color"][e["index"] == -1] == torch.tensor([0.25, 0.5, 0.75], device=DEV)).all()


# ---- 7. the frontend and the tool ----------------------------------------------------------------------------------------------
def _gl(c2w_cv):
    """An OpenCV camera-to-world pose as the OpenGL-style pose the SLAM system stores (columns 1 and 2 negated)."""
    m = np.array(c2w_cv, np.float64)
    m[:3, 1] *= -1
    m[:3, 2] *= -1
    return m


def _trajectory(n):
    est = np.stack([_gl(R.pose((0.3, 1.0, 0.2), 75.0 + 2.0 * k, (0.4 + 0.03 * k, -0.2, 0.6 + 0.02 * k))) for k in range(n)])
    gt = est.copy()
    gt[:, :3, 3] += np.array([0.02, 0.05, -0.03])
    return est, gt


def test_frontend_is_the_composition_of_render_mesh_calls():
    from dns_slam_amd import evaluation as E, ops, visualize
    v, f, _, _ = R.scene("room")
    f = f[:, ::-1].copy()                                         # seen from inside, the room's stored winding faces the viewer
    col = M.scene_colors("room")
    est, gt = _trajectory(12)
    view = _gl(R.pose((0.3, 1.0, 0.2), 60.0, (-0.6, -0.1, -0.4)))
    keep = view.copy()
    fe = visualize.Frontend("unused", view, cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, H=48, W=64)
    assert np.array_equal(view, keep)
    blank = fe.render()
    assert blank.shape == (48, 64, 3) and blank.dtype == np.uint8 and (blank == 255).all()
    fe.update_mesh(v, f, col)
    fe.update_pose(1, est[11], gt=False)
    fe.update_pose(1, torch.from_numpy(gt[11]), gt=True)
    fe.update_pose(1, est[11], gt=False)                          # moving an actor replaces it
    fe.update_cam_trajectory(11, gt=False)
    fe.update_cam_trajectory(11, gt=True)
    img = fe.render()
    # the same frame composed here
    cloud, colour = [], []
    for pose, is_gt in ((est[11], False), (gt[11], True)):
        m = pose.copy()
        m[:3, 2] *= -1
        a = visualize.camera_actor(0.3, is_gt)[0]                 # held to the reference's construction on the CPU
        cloud.append(a @ m[:3, :3].T + m[:3, 3])
        colour.append(np.tile([0.0, 0.0, 0.0] if is_gt else [1.0, 0.0, 0.0], (len(a), 1)))
    for lst, c in ((est, [1.0, 0.0, 0.0]), (gt, [0.0, 0.0, 0.0])):
        cloud.append(lst[1:11, :3, 3])
        colour.append(np.tile(c, (10, 1)))
    fy = 24.0 / np.tan(np.radians(30.0))
    w2c = _dev(E.world_to_camera(view[None], flip_yz=True))
    out = ops.render_mesh(_dev(v), _dev(f), _dev(col), w2c, 48, 64, fy, fy, 31.5, 23.5, z_near=0.01, z_far=1000.0, cull="front",
                          shade="headlight", ambient=0.3, background=(1, 1, 1), points=_dev(np.concatenate(cloud).astype(np.float32)),
                          point_colors=_dev(np.concatenate(colour).astype(np.float32)), point_size=4)
    want = (out["color"][0].clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy()
    assert np.array_equal(img, want)
    idx = out["index"][0].cpu().numpy()
    assert (idx >= 0).sum() > 1000 and (idx <= -2).sum() > 50
    assert (img[idx <= -2] == [255, 0, 0]).all(-1).any() and (img[idx <= -2] == [0, 0, 0]).all(-1).any()
    # the stored winding (the room seen from inside is front-facing) is hidden, as the reference hides it
    fe.update_mesh(v, f[:, ::-1].copy(), col)
    assert not (_np(ops.render_mesh(_dev(v), _dev(f[:, ::-1].copy()), _dev(col), w2c, 48, 64, fy, fy, 31.5, 23.5, z_far=1000.0,
                                    cull="front"))["index"] >= 0).any()
    fe.reset()
    assert len(fe.scene_points()[0]) == 20                        # the actors are gone, the trajectories stay
    with pytest.raises(ValueError):
        visualize.Frontend("unused", view, H=48, W=64).update_cam_trajectory(3, gt=False)


def _png_size(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    W, H = struct.unpack(">II", data[16:24])
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT" and len(zlib.decompress(data[41:41 + n])) == H * (1 + 3 * W)
    return H, W


def test_tool_writes_the_frames(tmp_path):
    from dns_slam_amd import meshing
    spec = importlib.util.spec_from_file_location("tools_visualize", os.path.join(ROOT, "tools", "visualize.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f, _, _ = R.scene("room")
    f = f[:, ::-1].copy()
    est, gt = _trajectory(12)
    scale = 2.0
    ck_est, ck_gt = est.copy(), gt.copy()
    ck_est[:, :3, 3] *= scale
    ck_gt[:, :3, 3] *= scale
    torch.save({"estimate_c2w_list": torch.from_numpy(ck_est).float(), "gt_c2w_list": torch.from_numpy(ck_gt).float(), "idx": 11},
               str(tmp_path / "00011.pt"))
    os.makedirs(tmp_path / "mesh")
    labels = (np.arange(len(v)) % 3).astype(np.int32)
    colours = (M.scene_colors("room") * 255).astype(np.uint8)
    meshing.write_ply(str(tmp_path / "mesh" / "00000_mesh.ply"), v, f[:6], colours, labels)
    meshing.write_ply(str(tmp_path / "mesh" / "00010_mesh.ply"), v, f, colours, labels)
    for extra in ((), ("--labels",), ("--no_gt_traj", "--every", "5")):
        tool.main([str(tmp_path), "--scale", str(scale), "--H", "48", "--W", "64", "--cam_scale", "0.3", *extra])
        names = sorted(os.listdir(tmp_path / "tmp_rendering"))
        n = 3 if "--every" in extra else 12
        assert names == [f"{k:06d}.png" for k in range(1, n + 1)]
        assert all(_png_size(str(tmp_path / "tmp_rendering" / x)) == (48, 64) for x in names)
