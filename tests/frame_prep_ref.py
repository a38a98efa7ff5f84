"""Host restatement of the frame preparation (include/dns_hip.h, "frame preparation"; BaseDataset.__getitem__ and cal_class_n of
datas/slam_datasets.py), written in numpy from the libraries' published resampling rules, independently of
csrc/frame_prep_plan.hpp:

  * the four tables (cv2 linear / nearest, torch bilinear align_corners=True / nearest), one function each;
  * colour evaluated in float64 from the fp32 weights: u8 / 255 exactly, each pass a w0 + b w1 without rounding, so what is left
    between it and an fp32 implementation is that implementation's rounding, which ``bound`` bounds;
  * depth in the reference's fp32 operations (numpy's fp32 division and product are IEEE, so these are THE bits);
  * labels and the class numbering done literally: ``np.vectorize`` over dict look-ups, ``set(label_data.flatten())``.
"""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32


# ---- tables: destination coordinate -> source index (, fp32 weights of index and index + 1) ---------------------------------------
def cv_linear_table(src, dst):
    """cv2.resize INTER_LINEAR on float32: the coordinate is rounded to fp32 before the floor."""
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.stack([np.float32(1) - f, f], -1).astype(np.float32)


def cv_linear_table_exact(src, dst):
    """The same rule with the coordinate kept in float64 (a WRONG preparer: tests show the bound tells it from the rule)."""
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    f = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
    s = np.floor(f).astype(np.int64)
    f = f - s
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, 0.0, f)
    return s, np.stack([1.0 - f, f], -1).astype(np.float32)


def cv_nearest_table(src, dst, rounding=np.floor):
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    return np.minimum(rounding(np.arange(dst, dtype=np.float64) * scale).astype(np.int64), src - 1)


def torch_nearest_table(src, dst, rounding=np.floor):
    scale = np.float32(src) / np.float32(dst)
    return np.minimum(rounding(np.arange(dst, dtype=np.float32) * scale).astype(np.int64), src - 1)


def torch_linear_table(src, dst, align_corners=True):
    d = np.arange(dst, dtype=np.float32)
    if align_corners:
        scale = np.float32(src - 1) / np.float32(dst - 1) if dst > 1 else np.float32(0)
        real = (scale * d).astype(np.float32)
    else:
        scale = np.float32(src) / np.float32(dst)
        real = np.maximum((scale * (d + np.float32(0.5)) - np.float32(0.5)).astype(np.float32), np.float32(0))
    s = np.minimum(np.floor(real).astype(np.int64), src - 1)
    lam = np.clip((real - s.astype(np.float32)).astype(np.float32), np.float32(0), np.float32(1))
    return s, np.stack([np.float32(1) - lam, lam], -1).astype(np.float32)


# ---- stages -----------------------------------------------------------------------------------------------------------------------
def resize_linear64(img, x_table, y_table):
    """img float64 [H,W,C] -> [len(y_table), len(x_table), C]: the horizontal pass, then the vertical pass, in float64 from the fp32
    weights."""
    (ix, wx), (iy, wy) = x_table, y_table
    H, W = img.shape[:2]
    wx, wy = wx.astype(np.float64), wy.astype(np.float64)
    h = img[:, ix] * wx[None, :, 0, None] + img[:, np.minimum(ix + 1, W - 1)] * wx[None, :, 1, None]
    return h[iy] * wy[:, 0, None, None] + h[np.minimum(iy + 1, H - 1)] * wy[:, 1, None, None]


def crop(img, edge):
    return img[edge:-edge, edge:-edge] if edge > 0 else img


def stage_list(color_hw, depth_hw, crop_size):
    """The resizes of the colour path that are not the identity, as (src, dst) size pairs."""
    out = []
    if tuple(color_hw) != tuple(depth_hw):
        out.append((tuple(color_hw), tuple(depth_hw)))
    if crop_size is not None and tuple(crop_size) != tuple(depth_hw):
        out.append((tuple(depth_hw), tuple(crop_size)))
    return out


def bound(stages):
    """Bound of |fp32 colour - float64 restatement| for values in [0, 1], from the operation count.  u = 2^-24.
    The tap: one correctly rounded division of a value <= 1: e <= u, magnitude M <= 1.
    Each pass (two per resize; an identity stage has none) computes fl(fl(a w0) + fl(b w1)) with w0 + w1 = S <= 1 + 2u (the pair
    sums to 1 within one ulp): the inherited error is scaled by at most S, each product adds u times its magnitude (together
    <= u M S), the sum adds u times the result's magnitude M S (1 + u); the magnitude becomes M S (1 + u)^2."""
    e, M = U, 1.0
    S = 1.0 + 2.0 * U
    for _ in stages:
        for _pass in range(2):
            e = S * e + U * M * S + U * M * S * (1.0 + U)
            M = M * S * (1.0 + U) ** 2
    return e


def prepare_color(color_u8, depth_hw, crop_size, edge, bgr=False, cv_table=cv_linear_table, torch_table=torch_linear_table):
    """color uint8 [Hc,Wc,3] -> float64 [H,W,3]."""
    c = color_u8.astype(np.float64) / 255.0
    if bgr:
        c = c[..., ::-1]
    Hc, Wc = c.shape[:2]
    Hd, Wd = depth_hw
    if (Hc, Wc) != (Hd, Wd):
        c = resize_linear64(c, cv_table(Wc, Wd), cv_table(Hc, Hd))
    if crop_size is not None and tuple(crop_size) != (Hd, Wd):
        c = resize_linear64(c, torch_table(Wd, crop_size[1]), torch_table(Hd, crop_size[0]))
    return crop(c, edge)


def prepare_depth(depth_u16, png_depth_scale, scale, crop_size, edge, nearest=torch_nearest_table):
    d = depth_u16.astype(np.float32) / np.float32(png_depth_scale)
    d = (d * np.float32(scale)).astype(np.float32)
    if crop_size is not None:
        d = d[nearest(d.shape[0], crop_size[0])][:, nearest(d.shape[1], crop_size[1])]
    return crop(d, edge)


def prepare_label(label, depth_hw, crop_size, edge, map_function, cv_near=cv_nearest_table, torch_near=torch_nearest_table):
    """label uint8/uint16 [Hl,Wl] -> int64 [H,W]; map_function(value) -> class as the dataset's (dict look-ups), through np.vectorize
    as the reference."""
    Hd, Wd = depth_hw
    lab = label.astype(np.float32)
    lab = lab[cv_near(lab.shape[0], Hd)][:, cv_near(lab.shape[1], Wd)]
    lab = np.vectorize(map_function, otypes=[np.int64])(lab)
    if crop_size is not None:
        lab = lab[torch_near(Hd, crop_size[0])][:, torch_near(Wd, crop_size[1])]
    return crop(lab, edge)


# ---- class numbering (cal_class_n) ------------------------------------------------------------------------------------------------
def class_numbering(label_images, id_map=None):
    """cal_class_n over the given (every fifth) label images, literally: set(label_data.flatten()), numbered in iteration order;
    id_map (ScanNet) first where given -> (label2class, class2label)."""
    l2c, c2l, n = {}, {}, 0
    for img in label_images:
        for label in set(img.flatten()):
            key = id_map.get(label, 0) if id_map is not None else label
            if key not in l2c:
                l2c[key] = n
                c2l[n] = key
                n += 1
    return l2c, c2l


def numbering_from_order(orders, dtype, id_map=None):
    """The same numbering from, per image, the distinct values in some order (first-seen, ascending, ...): the values go into a set
    as numpy scalars of the image's dtype in that order, and the set is iterated."""
    l2c, c2l, n = {}, {}, 0
    for order in orders:
        s = set()
        for v in order:
            s.add(dtype.type(v))
        for label in s:
            key = id_map.get(label, 0) if id_map is not None else label
            if key not in l2c:
                l2c[key] = n
                c2l[n] = key
                n += 1
    return l2c, c2l


def first_seen(label):
    """int64 [65536]: smallest flat index of every value, -1 where absent."""
    vals, idx = np.unique(label.reshape(-1), return_index=True)
    out = np.full(65536, -1, dtype=np.int64)
    out[vals.astype(np.int64)] = idx
    return out


def first_seen_order(label):
    vals, idx = np.unique(label.reshape(-1), return_index=True)
    return vals[np.argsort(idx, kind="stable")]


# ---- test data: label images of a chosen number of distinct values; tiny dataset trees ----------------------------------------------
def label_images(seed, dtype, n_distinct, shape=(12, 15), n_images=2):
    g = np.random.default_rng(seed)
    top = 256 if dtype == np.uint8 else 3001
    out = []
    for _ in range(n_images):
        values = g.choice(top, size=min(n_distinct, top), replace=False)
        out.append(values[g.integers(0, len(values), size=shape)].astype(dtype))
    return out


def write_trees(tmp_path, store):
    """A tiny Replica tree and a tiny ScanNet tree: the image 'files' hold nothing; their arrays live in `store`, keyed by path, and
    the reader returns them (decoding is host work behind reader=)."""
    g = np.random.default_rng(5)
    rep, scan = tmp_path / "replica", tmp_path / "scannet"
    n_rep, n_scan = 7, 6
    for sub in ("rgb", "depth", "semantic_class"):
        (rep / sub).mkdir(parents=True)
    rep_poses = g.normal(size=(n_rep, 16))
    (rep / "traj_w_c.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in rep_poses) + "\n")
    for i in range(n_rep):
        for path, arr in ((rep / "rgb" / f"rgb_{i}.png", g.integers(0, 256, size=(8, 13, 3), dtype=np.uint8)),
                          (rep / "depth" / f"depth_{i}.png", g.integers(0, 65536, size=(8, 13)).astype(np.uint16)),
                          (rep / "semantic_class" / f"semantic_class_{i}.png", label_images(20 + i, np.uint8, 9, (8, 13), 1)[0])):
            path.write_bytes(b"")
            store[str(path)] = arr
    for sub in ("color", "depth", "label-filt", "pose"):
        (scan / sub).mkdir(parents=True)
    scan_poses = g.normal(size=(n_scan, 4, 4))
    rows = ["id\traw_category\tcategory\tcount\tnyu40id\tmore"] + [f"{v}\tx\tx\t1\t{(v * 7) % 41}\tx" for v in range(1, 400, 3)]
    (scan / "scannetv2-labels.combined.tsv").write_text("\n".join(rows) + "\n")
    for i in range(n_scan):
        (scan / "pose" / f"{i}.txt").write_text("\n".join(" ".join(repr(float(v)) for v in r) for r in scan_poses[i]) + "\n")
        for path, arr in ((scan / "color" / f"{i}.jpg", g.integers(0, 256, size=(13, 17, 3), dtype=np.uint8)),
                          (scan / "depth" / f"{i}.png", g.integers(0, 65536, size=(7, 9)).astype(np.uint16)),
                          (scan / "label-filt" / f"{i}.png", label_images(40 + i, np.uint16, 12, (13, 17), 1)[0] % 400)):
            path.write_bytes(b"")
            store[str(path)] = arr.astype(arr.dtype)
    return str(rep), rep_poses, str(scan), scan_poses


def reader(store, order="RGB"):
    def read(path):
        return store[str(path)]
    read.color_order = order
    return read


REPLICA_CFG = {"dataset": "replica", "cam": {"H": 8, "W": 13, "fx": 6.0, "fy": 6.0, "cx": 6.0, "cy": 3.5, "png_depth_scale": 6553.5,
                                             "crop_edge": 0}}
SCANNET_CFG = {"dataset": "scannet", "cam": {"H": 7, "W": 9, "fx": 5.5, "fy": 5.25, "cx": 4.0, "cy": 3.0, "png_depth_scale": 1000.0,
                                             "crop_edge": 1, "crop_size": [9, 11]}}
