"""CPU: the host restatement of the frame preparation (tests/frame_prep_ref.py) against F.interpolate, its bound against wrong
preparers, the class numbering from first-seen order against the literal set walk, and the dataset classes (dns_slam_amd.datasets) on
device="cpu" with method="torch" on tiny Replica and ScanNet trees."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_prep_ref as fr  # noqa: E402

SIZE_PAIRS = [(480, 484), (640, 648), (968, 480), (7, 5), (5, 7), (7, 9), (9, 11), (1, 4), (6, 1), (8, 8), (65, 65)]


# ---- the crop_size stages against F.interpolate --------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_torch_nearest_rule_is_f_interpolate(src, dst):
    x = torch.arange(src, dtype=torch.float32)
    along_w = F.interpolate(x.reshape(1, 1, 1, src), (1, dst), mode="nearest").reshape(-1).long().numpy()
    along_h = F.interpolate(x.reshape(1, 1, src, 1), (dst, 1), mode="nearest").reshape(-1).long().numpy()
    t = fr.torch_nearest_table(src, dst)
    assert np.array_equal(t, along_w) and np.array_equal(t, along_h)


@pytest.mark.parametrize("hw,out", [((7, 9), (9, 11)), ((11, 13), (9, 11)), ((5, 6), (11, 13)), ((8, 65), (8, 65)), ((4, 1), (6, 3)),
                                    ((48, 64), (49, 66))])
def test_torch_bilinear_rule_within_bound(hw, out):
    g = np.random.default_rng(hw[0] * 100 + out[1])
    img = g.integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)
    c32 = torch.from_numpy(img.astype(np.float32) / np.float32(255))
    got = F.interpolate(c32.permute(2, 0, 1)[None], out, mode="bilinear", align_corners=True)[0].permute(1, 2, 0).numpy().astype(np.float64)
    ref = fr.resize_linear64(img.astype(np.float64) / 255.0, fr.torch_linear_table(hw[1], out[1]), fr.torch_linear_table(hw[0], out[0]))
    b = fr.bound([(hw, out)]) if hw != out else fr.bound([])
    err = np.abs(got - ref).max()
    print(f"bilinear {hw} -> {out}: max |F.interpolate - restatement| {err:.3e}, bound {b:.3e}")
    assert err <= b


def test_bound_counts_operations():
    u = fr.U
    assert fr.bound([]) == u                                    # the division alone
    one, two = fr.bound([((2, 2), (3, 3))]), fr.bound([((2, 2), (3, 3)), ((3, 3), (4, 4))])
    assert 5 * u <= one <= 5 * u * (1 + 1e-5) and 9 * u <= two <= 9 * u * (1 + 1e-5)   # 1 + 2 per pass, two passes per resize


# ---- the bound rejects wrong preparers -----------------------------------------------------------------------------------------------
def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def test_bound_rejects_wrong_colour_preparers():
    img = _noise((13, 17, 3), 1)
    depth_hw, crop_size, edge = (7, 9), (9, 11), 1
    ref = fr.prepare_color(img, depth_hw, crop_size, edge)
    b = fr.bound(fr.stage_list(img.shape[:2], depth_hw, crop_size))
    rounded = ref.astype(np.float32).astype(np.float64)          # a correct fp32 preparer at its best passes
    assert np.abs(rounded - ref).max() <= b
    wrong = {
        "swapped channels": fr.prepare_color(img, depth_hw, crop_size, edge, bgr=True),
        "align_corners=False in the second stage": fr.prepare_color(
            img, depth_hw, crop_size, edge, torch_table=lambda s, d: fr.torch_linear_table(s, d, align_corners=False)),
    }
    # the crop taken before the resize: crop the depth-sized image by edge, then resize to the cropped crop_size
    c = fr.resize_linear64(img.astype(np.float64) / 255.0, fr.cv_linear_table(17, 9), fr.cv_linear_table(13, 7))
    c = fr.crop(c, edge)
    wrong["crop before the resize"] = fr.resize_linear64(c, fr.torch_linear_table(7, 9), fr.torch_linear_table(5, 7))
    for name, w in wrong.items():
        assert w.shape == ref.shape, name
        err = np.abs(w - ref).max()
        print(f"{name}: {err:.3e} against the bound {b:.3e}")
        assert err > b, name


def test_bound_rejects_exact_cv_coordinates():
    """Rounding the cv2 coordinate to fp32 moves a weight by up to 2^-14 at ScanNet's width: a preparer with exact weights is a
    different image, far outside the rounding bound."""
    img = _noise((2, 1296, 3), 2)
    depth_hw = (2, 640)
    ref = fr.prepare_color(img, depth_hw, None, 0)
    wrong = fr.prepare_color(img, depth_hw, None, 0, cv_table=fr.cv_linear_table_exact)
    b = fr.bound(fr.stage_list((2, 1296), depth_hw, None))
    w_rule, w_exact = fr.cv_linear_table(1296, 640)[1], fr.cv_linear_table_exact(1296, 640)[1]
    assert 2.0 ** -17 < np.abs(w_rule.astype(np.float64) - w_exact).max() <= 2.0 ** -14
    assert np.abs(wrong - ref).max() > b


def test_nearest_rules_reject_round_to_nearest():
    lab = np.random.default_rng(3).integers(0, 200, size=(13, 17), dtype=np.uint16)
    dep = np.random.default_rng(4).integers(0, 65536, size=(7, 9), dtype=np.uint16)
    ident = lambda v: int(v)
    ref_l = fr.prepare_label(lab, (7, 9), (9, 11), 1, ident)
    ref_d = fr.prepare_depth(dep, 6553.5, 1.0, (9, 11), 1)
    near = lambda table: (lambda s, d: table(s, d, rounding=np.rint))
    assert not np.array_equal(fr.prepare_label(lab, (7, 9), (9, 11), 1, ident, cv_near=near(fr.cv_nearest_table)), ref_l)
    assert not np.array_equal(fr.prepare_label(lab, (7, 9), (9, 11), 1, ident, torch_near=near(fr.torch_nearest_table)), ref_l)
    assert not np.array_equal(fr.prepare_depth(dep, 6553.5, 1.0, (9, 11), 1, nearest=near(fr.torch_nearest_table)), ref_d)


# ---- class numbering ---------------------------------------------------------------------------------------------------------------------
def test_class_numbering_from_first_seen_order():
    ascending_wrong = 0
    cases = [(np.uint8, n) for n in (1, 2, 7, 40, 120)] + [(np.uint16, n) for n in (1, 2, 7, 40, 120)]
    for k, (dtype, n) in enumerate(cases * 3):
        imgs = fr.label_images(100 + k, dtype, n)
        literal = fr.class_numbering(imgs)
        seen = fr.numbering_from_order([fr.first_seen_order(i) for i in imgs], np.dtype(dtype))
        assert seen == literal, (dtype, n)
        assert [type(x) for x in seen[0]] == [type(x) for x in literal[0]]
        ascending_wrong += fr.numbering_from_order([np.unique(i) for i in imgs], np.dtype(dtype)) != literal
    assert ascending_wrong >= 1                                   # np.unique alone is not enough
    id_map = {v: v % 41 for v in range(1, 3001, 2)}               # ScanNet: through id_map first, absent ids -> 0
    imgs = fr.label_images(7, np.uint16, 60)
    assert fr.numbering_from_order([fr.first_seen_order(i) for i in imgs], np.dtype(np.uint16), id_map) == fr.class_numbering(imgs, id_map)


def test_label_first_seen_torch_method():
    from dns_slam_amd import ops
    for dtype in (np.uint8, np.uint16):
        img = np.stack(fr.label_images(11, dtype, 30, shape=(9, 13)))
        got = ops.label_first_seen(torch.from_numpy(img), method="torch")
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), fr.first_seen(img))
    with pytest.raises(ValueError):
        ops.label_first_seen(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.label_first_seen(torch.zeros(4, dtype=torch.uint8), method="kernel")      # the kernel takes device tensors only


# ---- ops.prepare_frames(method="torch") and the dataset classes on the CPU --------------------------------------------------------------
def test_camera_from_cfg():
    from dns_slam_amd.datasets import camera_from_cfg
    assert camera_from_cfg(fr.REPLICA_CFG) == {"H": 8, "W": 13, "fx": 6.0, "fy": 6.0, "cx": 6.0, "cy": 3.5}
    # crop_size [9, 11] of 7 x 9: sx = 11 / 9, sy = 9 / 7; then crop_edge 1 takes 2 off H, W and 1 off cx, cy
    cam = camera_from_cfg(fr.SCANNET_CFG)
    assert cam == {"H": 7, "W": 9, "fx": 11 / 9 * 5.5, "fy": 9 / 7 * 5.25, "cx": 11 / 9 * 4.0 - 1, "cy": 9 / 7 * 3.0 - 1}
    assert fr.SCANNET_CFG["cam"]["H"] == 7 and fr.SCANNET_CFG["cam"]["crop_size"] == [9, 11]            # the config is not written to


def _check_frame(ds, store, i, item, depth_hw, crop_size, edge, pds, scale, bgr):
    idx, color, depth, label, pose = item
    cp, dp, lp = ds.frame_paths(i)
    assert idx == i and color.dtype == torch.float32 and depth.dtype == torch.float32 and label.dtype == torch.int64
    ref_c = fr.prepare_color(store[cp], depth_hw, crop_size, edge, bgr=bgr)
    b = fr.bound(fr.stage_list(store[cp].shape[:2], depth_hw, crop_size))
    assert tuple(color.shape) == ref_c.shape and np.abs(color.numpy().astype(np.float64) - ref_c).max() <= b
    assert np.array_equal(depth.numpy(), fr.prepare_depth(store[dp], pds, scale, crop_size, edge))
    assert np.array_equal(label.numpy(), fr.prepare_label(store[lp], depth_hw, crop_size, edge, ds.map_function))
    return pose


def test_replica_on_cpu(tmp_path):
    from dns_slam_amd import datasets
    store = {}
    rep, rep_poses, _, _ = fr.write_trees(tmp_path, store)
    ds = datasets.get_dataset(fr.REPLICA_CFG, rep, 2.0, device="cpu", reader=fr.reader(store), method="torch")
    assert isinstance(ds, datasets.Replica) and len(ds) == ds.n_img == 7
    assert (ds.H, ds.W, ds.cx, ds.cy) == (8, 13, 6.0, 3.5) and ds.fx == ds.fy == 13 / 2.0 / math.tan(math.radians(45.0))
    l2c, c2l = fr.class_numbering([store[ds.label_path(i)] for i in (0, 5)])
    assert ds.label2class_dict == l2c and ds.class2label_dict == c2l and ds.n_class == len(l2c)
    assert [type(k) for k in ds.label2class_dict] == [type(k) for k in l2c]
    for i in (0, 3, 6):
        pose = _check_frame(ds, store, i, ds[i], (8, 13), None, 0, 6553.5, 2.0, False)
        want = rep_poses[i].reshape(4, 4).copy()
        want[:3, 1] *= -1
        want[:3, 2] *= -1
        want = want.astype(np.float32)
        assert np.array_equal(ds.poses[i].numpy(), want)                       # a read leaves the stored pose alone ...
        want[:3, 3] *= np.float32(2.0)
        assert np.array_equal(pose.numpy(), want)                              # ... and returns the scaled copy
    # Replica's colour is the identity case: fl32(u8) / 255 bit for bit
    assert np.array_equal(ds[2][1].numpy(), store[ds.frame_paths(2)[0]].astype(np.float32) / np.float32(255))
    idx, c, d, l, p = ds.frames([4, 1])
    assert idx == [4, 1] and torch.equal(c[1], ds[1][1]) and torch.equal(d[0], ds[4][2]) and torch.equal(l[1], ds[1][3]) and torch.equal(p[0], ds[4][4])
    # the reader declares the channel order
    ds_bgr = datasets.Replica(fr.REPLICA_CFG, rep, 2.0, device="cpu", reader=fr.reader(store, "BGR"), method="torch")
    assert torch.equal(ds_bgr[0][1], ds[0][1].flip(-1))


def test_scannet_on_cpu(tmp_path):
    from dns_slam_amd import datasets
    store = {}
    _, _, scan, scan_poses = fr.write_trees(tmp_path, store)
    ds = datasets.get_dataset(fr.SCANNET_CFG, scan, 1.0, device="cpu", reader=fr.reader(store), method="torch")
    assert isinstance(ds, datasets.ScanNet) and ds.n_img == 6 and (ds.H, ds.W, ds.fx, ds.fy, ds.cx, ds.cy) == (7, 9, 5.5, 5.25, 4.0, 3.0)
    assert ds.id_map[1] == 7 and ds.id_map[4] == 28 and ds.id_map[7] == 8 and 2 not in ds.id_map and len(ds.id_map) == 133
    l2c, c2l = fr.class_numbering([store[ds.label_path(i)] for i in (0, 5)], ds.id_map)
    assert ds.label2class_dict == l2c and ds.class2label_dict == c2l and ds.n_class == len(l2c) and ds.n_class > 1
    for i in (0, 4):
        pose = _check_frame(ds, store, i, ds[i], (7, 9), (9, 11), 1, 1000.0, 1.0, False)
        assert tuple(ds[i][1].shape) == (7, 9, 3)
        want = scan_poses[i].copy()
        want[:3, 1] *= -1
        want[:3, 2] *= -1
        assert np.array_equal(pose.numpy(), want.astype(np.float32))


def test_distortion_is_refused(tmp_path):
    from dns_slam_amd import datasets
    cfg = {"dataset": "replica", "cam": dict(fr.REPLICA_CFG["cam"], distortion=[0.1, 0.0, 0.0, 0.0, 0.0])}
    with pytest.raises(NotImplementedError, match="distortion"):
        datasets.get_dataset(cfg, str(tmp_path), 1.0, device="cpu")


def test_prepare_frames_argument_errors_on_cpu():
    from dns_slam_amd import ops
    t = ops.frame_prep_tables((5, 6), (5, 6), (5, 6), None, 0, device="cpu")
    c, d = torch.zeros(5, 6, 3, dtype=torch.uint8), torch.zeros(5, 6, dtype=torch.uint16)
    l, lut = torch.zeros(5, 6, dtype=torch.uint8), torch.arange(65536, dtype=torch.int32)
    assert ops.prepare_frames(c, d, l, lut, t, 1000.0)[2].shape == (5, 6)
    for bad in (lambda: ops.prepare_frames(c.float(), d, l, lut, t, 1000.0), lambda: ops.prepare_frames(c, d.to(torch.int32), l, lut, t, 1000.0),
                lambda: ops.prepare_frames(c, d, l.to(torch.int64), lut, t, 1000.0), lambda: ops.prepare_frames(c, d, l, lut.long(), t, 1000.0),
                lambda: ops.prepare_frames(c[:4], d, l, lut, t, 1000.0), lambda: ops.prepare_frames(c, d, None, None, t, 1000.0),
                lambda: ops.prepare_frames(c, d, l, lut, t, 0.0), lambda: ops.prepare_frames(c, d, l, lut, t, 1000.0, method="kernel"),
                lambda: ops.prepare_frames(c, d, l, lut, t, 1000.0, method="cv2"),
                lambda: ops.frame_prep_tables((5, 6), (5, 6), None, None, 3, device="cpu"), lambda: ops.frame_prep_tables((0, 6), (5, 6))):
        with pytest.raises(ValueError):
            bad()


def test_default_reader_decodes_png_files(tmp_path):
    """The Pillow reader: 16-bit grey PNGs come back uint16, 8-bit grey uint8, colour uint8 RGB -- and a Replica tree of real files
    reads through it."""
    Image = pytest.importorskip("PIL.Image")
    from dns_slam_amd import datasets
    g = np.random.default_rng(9)
    d16 = g.integers(0, 65536, size=(8, 13)).astype(np.uint16)
    d16[0, :2] = [0, 65535]
    l8 = fr.label_images(1, np.uint8, 5, (8, 13), 1)[0]
    rgb = g.integers(0, 256, size=(8, 13, 3), dtype=np.uint8)
    rep = tmp_path / "rep"
    for sub in ("rgb", "depth", "semantic_class"):
        (rep / sub).mkdir(parents=True)
    Image.fromarray(d16).save(rep / "depth" / "depth_0.png")
    Image.fromarray(l8).save(rep / "semantic_class" / "semantic_class_0.png")
    Image.fromarray(rgb).save(rep / "rgb" / "rgb_0.png")
    (rep / "traj_w_c.txt").write_text(" ".join(str(float(v)) for v in np.eye(4).reshape(-1)) + "\n")
    for path, want in ((rep / "depth" / "depth_0.png", d16), (rep / "semantic_class" / "semantic_class_0.png", l8), (rep / "rgb" / "rgb_0.png", rgb)):
        got = datasets.pil_reader(str(path))
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert datasets.pil_reader.color_order == "RGB"
    ds = datasets.Replica(fr.REPLICA_CFG, str(rep), 1.0, device="cpu", method="torch")
    _, color, depth, label, _ = ds[0]
    assert np.array_equal(color.numpy(), rgb.astype(np.float32) / np.float32(255))
    assert np.array_equal(depth.numpy(), fr.prepare_depth(d16, 6553.5, 1.0, None, 0))
    assert np.array_equal(label.numpy(), fr.prepare_label(l8, (8, 13), None, 0, ds.map_function))
