"""CPU: the host reference of the colour rasteriser (tests/mesh_render_ref.py) against raster_ref, against the kernel's arithmetic
restated in numpy float32 -- which its bounds must accept -- and against deliberately wrong renderers, which they must reject;
the PNG writer and the camera actor of dns_slam_amd/visualize.py."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_render_ref as M                                     # noqa: E402
import raster_ref as R                                          # noqa: E402


def _f32(name, view, cull=None, shade=None, wrong=None):
    v, f, w2c, cam = R.scene(name)
    return M.render_view_f32(v, f, M.scene_colors(name), w2c[view], *R._cam_args(cam), cull=cull, shade=shade, wrong=wrong)


@pytest.mark.parametrize("name,view", [("room", 1), ("soup", 2), ("lattice", 1), ("sphere", 1)])
def test_agrees_with_raster_ref_without_culling(name, view):
    r, m = R.render(name), M.render(name, view)[None]
    assert np.array_equal(m["index"], r["tri"][view])
    assert np.array_equal(m["D"], r["D"][view])
    assert not (m["unambiguous"] & ~r["unambiguous"][view]).any()           # only ever stricter
    # culling partitions the faces: every face pixel of "back" and "front" is a face of that facing, and together they cover
    # what the unculled image covers
    back, front = M.render(name, view)["back"], M.render(name, view)["front"]
    assert np.array_equal(back["covered"] | front["covered"], m["covered"])
    both = back["covered"] & front["covered"]
    assert (np.minimum(back["D"], front["D"])[m["covered"]] == m["D"][m["covered"]]).all()
    assert not (back["index"][both] == front["index"][both]).any()


@pytest.mark.parametrize("cull", M.CULLS)
@pytest.mark.parametrize("name,view", [("room", 1), ("soup", 1), ("sphere", 1), ("lattice", 1)])
def test_fp32_restatement_is_inside_the_bounds(name, view, cull):
    ref = M.render(name, view)[cull]
    for shade in M.SHADES:
        r = M.compare(ref, *_f32(name, view, cull, shade), shade)
        print(f"{name}/{view}/{cull}/{shade}: {r}")
        assert r["bad_index"] == 0 and r["bad_depth"] == 0 and r["bad_color"] == 0
        if r["covered"]:
            assert r["compared"] >= M.MIN_COMPARED * r["covered"]


def test_compared_pixels_of_every_parity_case():
    """The share of the reference's covered pixels that is compared, per (scene, view, cull): at least MIN_COMPARED."""
    worst = 1.0
    for name, views in M.PARITY:
        for view in views:
            for cull in M.CULLS:
                ref = M.render(name, view)[cull]
                n = int(ref["covered"].sum())
                if n:
                    share = int((ref["covered"] & ref["unambiguous"]).sum()) / n
                    print(f"{name}/{view}/{cull}: {share:.4f} of {n}")
                    worst = min(worst, share)
                    assert share >= M.MIN_COMPARED
    assert worst < 1.0                                            # and the rules do leave pixels out


@pytest.mark.parametrize("wrong,name,view,cull,shade", [
    ("affine", "room", 1, None, None), ("affine", "soup", 1, None, "headlight"),
    ("rotate", "room", 1, None, None), ("rotate", "sphere", 1, "back", None),
    ("cull", "soup", 1, "back", None), ("cull", "sphere", 1, "front", None),
    ("noabs", "soup", 1, None, "headlight"), ("noabs", "room", 1, None, "headlight"),
])
def test_bounds_reject_wrong_renderers(wrong, name, view, cull, shade):
    ref = M.render(name, view)[cull]
    good = M.compare(ref, *_f32(name, view, cull, shade), shade)
    bad = M.compare(ref, *_f32(name, view, cull, shade, wrong=wrong), shade)
    print(f"{wrong} on {name}/{view}/{cull}/{shade}: {bad}")
    assert good["bad_index"] == 0 and good["bad_color"] == 0
    if wrong == "cull":
        assert bad["bad_index"] > 0.5 * good["compared"]
    else:
        assert bad["bad_index"] == 0 and bad["bad_color"] > 0.5 * good["compared"] and bad["worst"] > 10.0


@pytest.mark.parametrize("size", (1, 4))
@pytest.mark.parametrize("where", ("front", "behind", "border"))
def test_point_squares(where, size):
    at = {"front": M.ACTOR_FRONT, "behind": M.ACTOR_BEHIND, "border": M.ACTOR_BORDER}[where]
    ref = M.render_actor(at, size)[None]
    v, f, w2c, cam = R.scene("lattice")
    p, c = M.actor_cloud(at)
    args = (v, f, M.scene_colors("lattice"), w2c[1], *R._cam_args(cam))
    good = M.compare(ref, *M.render_view_f32(*args, points=p, point_colors=c, point_size=size), None)
    bad = M.compare(ref, *M.render_view_f32(*args, points=p, point_colors=c, point_size=size, wrong="shift"), None)
    print(f"{where}/{size}: {good}; shifted {bad}")
    assert good["bad_index"] == 0 and good["bad_depth"] == 0 and good["bad_color"] == 0
    assert good["compared"] >= M.MIN_COMPARED * good["covered"]
    assert bad["bad_index"] > 0
    pts = ref["index"] <= -2
    wall = ref["face_index"] >= 0
    if where == "front":
        assert (pts & wall).sum() > 50 * size
    if where == "behind":
        assert not (pts & wall).any() and pts.any()               # seen only beside the wall
    if where == "border":
        assert pts[:, 0].any() and not pts[:, -1].any()           # cut by the left border


def test_point_rules():
    """The square of one point: pixel centres in [u - s/2, u + s/2); a face at the same depth wins; the lower point wins."""
    cam = R.SCENE_CAMS["lattice"]
    v, f = R.lattice_mesh()
    w2c = R.w2c_f32(R.pose()[None])[0]
    col = M.scene_colors("lattice")
    # u = 32 * 0.25 / 2 + 47.5 = 51.5, w = 39.5: size 4 -> columns 50..53 (50 - 51.5 = -1.5 >= -2), rows 38..41
    pts = np.array([[0.25, 0.0, 2.0], [0.25, 0.0, 1.0], [0.5, 0.0, 1.0]], np.float32)
    pc = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    out = M.render_view(v, f, col, w2c, *R._cam_args(cam), culls=(None,), points=pts, point_colors=pc, point_size=4)[None]
    idx = out["index"]
    assert (idx >= 0).sum() == 25 * 17 - 0 - ((idx <= -2) & (out["face_index"] >= 0)).sum()
    assert not (idx == -2).any()                                  # point 0 lies exactly in the wall's plane: the faces win
    # point 1 at z = 1: u = 32 * 0.25 + 47.5 = 55.5 -> columns 54..57; point 2: u = 63.5 -> columns 62..65
    assert np.array_equal(np.argwhere(idx == -3), [[i, j] for i in range(38, 42) for j in range(54, 58)])
    assert np.array_equal(np.argwhere(idx == -4), [[i, j] for i in range(38, 42) for j in range(62, 66)])
    assert out["unambiguous"][38:42, 54:58].all() and out["unambiguous"][38:42, 62:66].all()      # u - 2 is a half-integer
    i32, d32, c32 = M.render_view_f32(v, f, col, w2c, *R._cam_args(cam), points=pts, point_colors=pc, point_size=4)
    assert np.array_equal(i32, idx) and (d32[idx == -3] == 1.0).all() and (c32[idx == -4] == [0, 0, 1]).all()
    # size 1: u - 1/2 = 55 and w - 1/2 = 39 are integers, the square may start on either side: 2 x 2 ambiguous pixels
    one = M.render_view(v, f, col, w2c, *R._cam_args(cam), culls=(None,), points=pts[1:2], point_colors=pc[1:2], point_size=1)[None]
    assert np.array_equal(np.argwhere(one["index"] == -2), [[39, 55]])
    assert not one["unambiguous"][39:41, 55:57].any() and one["unambiguous"][38:42, 55:59].sum() == 12
    # two points on one pixel at one depth: the lower index
    two = np.array([[0.5, 0.0, 1.0], [0.5, 0.0, 1.0]], np.float32)
    out2 = M.render_view(v, f, col, w2c, *R._cam_args(cam), culls=(None,), points=two, point_colors=pc[:2], point_size=2)[None]
    assert (out2["index"] == -2).sum() == 4 and not (out2["index"] == -3).any()


def test_uncertain_facing_faces_are_left_out():
    """A triangle in a plane through the camera centre (here the plane of pixel row 12: y / z = 1 / 60) has num = 0 up to
    rounding: uncertain-facing.  Under a culling mode the pixels it may cover are ambiguous, the rest of a certain triangle
    behind it is compared."""
    cam = R.SCENE_CAMS["behind"]                                  # cy = 11.5, fy = 30
    v = np.array([[-0.5, 1 / 60, 1.0], [0.5, 2 / 60, 2.0], [0.0, 3 / 60, 3.0], [-1, -1, 4.0], [1, -1, 4.0], [0, 1, 4.0]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    w2c = R.w2c_f32(R.pose()[None])[0]
    fd = M._face_data(v, f, w2c)
    assert M.keep_mask(fd, "back")[1].tolist() == [True, False] and fd["num"][1] > 0        # face 1 is back-facing
    out = M.render_view(v, f, np.ones((6, 3), np.float32), w2c, *R._cam_args(cam))
    big = out["front"]["face_index"] == 1
    assert big[12, 12:20].all() and big.sum() > 100
    assert not out["front"]["unambiguous"][12, 12:20].any()
    rest = big.copy()
    rest[12] = False
    assert np.array_equal(out["front"]["unambiguous"][rest], out["front"]["plain"][rest]) and out["front"]["unambiguous"][rest].sum() > 80
    assert out["front"]["plain"][12, 13:19].all()                 # raster_ref's own rules would have compared them
    assert not (out["back"]["face_index"] == 1).any()


# ---- dns_slam_amd/visualize.py: what needs no GPU ----------------------------------------------------------------------------
def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(H, 1 + W * ch)
    assert (raw[:, 0] == 0).all()                                 # filter type 0 on every row
    return raw[:, 1:].reshape((H, W, 3) if ch == 3 else (H, W))


@pytest.mark.parametrize("shape", ((5, 7, 3), (1, 1, 3), (33, 20), (48, 64, 3)))
def test_png_round_trip(tmp_path, shape):
    from dns_slam_amd import visualize
    img = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    path = tmp_path / "a.png"
    visualize.write_png(str(path), img)
    assert np.array_equal(_decode_png(str(path)), img)
    with pytest.raises(ValueError):
        visualize.write_png(str(path), img.astype(np.float32))
    with pytest.raises(ValueError):
        visualize.write_png(str(path), np.zeros((4, 4, 4), np.uint8))


@pytest.mark.parametrize("scale,is_gt", ((0.005, False), (0.1, True), (1.0, False)))
def test_camera_actor_is_the_references_construction(scale, is_gt):
    from dns_slam_amd import visualize
    pts, colour = visualize.camera_actor(scale, is_gt)
    assert pts.shape == (1200, 3) and pts.dtype == np.float64
    want = M.camera_actor_ref(scale)
    assert np.abs(pts - want).max() <= 4 * np.finfo(np.float64).eps * 1.5 * scale
    assert tuple(colour) == ((0.0, 0.0, 0.0) if is_gt else (1.0, 0.0, 0.0))
    assert np.array_equal(pts[0], scale * np.array([-1, -1, 1.5])) and np.array_equal(pts[99], scale * np.array([1, -1, 1.5]))
    assert np.array_equal(pts[600], scale * np.array([-1, -1, 1.5])) and np.array_equal(pts[699], [0, 0, 0])       # line (1, 0)
