"""3-D reconstruction metrics: the reference's ``cull_mesh.py`` and ``eval_3d.py`` (calc_3d_metric) on the device.

``read_ply`` / ``load_poses`` read what the tools take from disk; ``cull_mesh`` drops the faces no camera of a trajectory sees
(``ops.frustum_seen``); ``sample_surface`` is trimesh's area-weighted surface sampler; ``accuracy`` / ``completion`` /
``completion_ratio`` are the nearest-neighbour metrics (``ops.nearest_points`` in place of the host KD-tree) and ``metrics_3d``
the three of them for two meshes.  ``align_transformation`` is the reference's ICP alignment (open3d's point-to-point
``registration_icp``, restated by ``ops.icp_point_to_point``) and ``calc_3d_metric`` the reference's function under its own name:
the alignment, then ``metrics_3d``.

2-D evaluation and trajectory error: the reference's ``eval_2d.py`` and ``eval_ate.py``.  ``psnr`` / ``ms_ssim`` score rendered
images (``ops.ms_ssim``: MS-SSIM and the masked MSE in one launch sequence), ``semantic_metrics`` turns a confusion matrix
(``ops.label_confusion``) into mIoU / fwIoU / accuracies, ``render_metrics`` is the loop of eval_2d.py:398-411 over a frame list
with one host read at the end, and ``evaluate_ate`` the absolute trajectory error after the closed-form rigid alignment.

LPIPS (eval_2d.py:81-82,304): ``lpips`` is ``ops.lpips``, the AlexNet tower and the distance head on the device, and
``render_metrics(..., lpips=weights)`` queues it behind each frame's MS-SSIM.  The network weights are an input:
``load_lpips_weights`` reads torchvision's AlexNet state dict and lpips v0.1's ``alex.pth`` from files the caller has; none is part
of this repository and none is fetched.  Limit: neither the lpips package, torchvision nor a pretrained file was available where
this was written, so the arithmetic is held to a float64 restatement of the published definition (include/dns_hip.h,
tests/lpips_ref.py) with weights drawn from a seed, not to values the lpips package wrote.

Depth L1: the reference's ``eval_3d.calc_2d_metric``.  ``view_box`` / ``look_at`` / ``sample_views`` draw the virtual cameras
(``ops.views_see_any`` rejects those that see the unseen cloud), ``render_depth`` turns a mesh into depth images
(``ops.rasterize_depth`` in place of open3d's visualiser), ``depth_l1`` is the per-view mean absolute difference of two meshes'
images (``ops.depth_l1``) with one host read at the end, and ``calc_2d_metric`` the reference's function under its own name.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .meshing import compact_mesh

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path) -> dict:
    """Binary little-endian PLY 1.0 -> {"verts": fp32 [V,3], "faces": int32 [F,3]} plus "colors" uint8 [V,3] (properties red,
    green, blue) and "labels" int32 [V] (property label) when the file has them: what ``meshing.write_ply`` writes, and more
    generally any scalar vertex properties of the standard PLY types in any order and a face list with a ``uchar`` count and
    ``int`` / ``uint`` indices.  ASCII and big-endian files, faces that are not triangles and anything else this reader cannot
    lay out raise ValueError naming the cause."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"read_ply: {path}: not a PLY file (no 'ply' ... 'end_header' header)")
    lines = [l.strip() for l in data[:end].decode("ascii", "replace").splitlines()]
    fmt = None
    elements = []                                   # [name, count, [property, ...]]
    for line in lines[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1:]
        elif tok[0] == "element" and len(tok) == 3:
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property" and elements:
            if tok[1] == "list" and len(tok) == 5:
                elements[-1][2].append(("list", tok[4], tok[2], tok[3]))
            elif len(tok) == 3:
                elements[-1][2].append(("scalar", tok[2], tok[1]))
            else:
                raise ValueError(f"read_ply: {path}: cannot parse header line {line!r}")
        else:
            raise ValueError(f"read_ply: {path}: cannot parse header line {line!r}")
    if not fmt or fmt[0] != "binary_little_endian":
        raise ValueError(f"read_ply: {path}: format {' '.join(fmt or ['(none)'])} is not supported (binary_little_endian only; "
                         f"ASCII and big-endian files are refused)")
    off = nl + 1
    vert = None
    faces = np.zeros((0, 3), np.int32)
    for name, count, props in elements:
        if count < 0:
            raise ValueError(f"read_ply: {path}: element {name} has count {count}")
        lists = [p for p in props if p[0] == "list"]
        for p in props:
            for t in p[2:]:
                if t not in _PLY_TYPES:
                    raise ValueError(f"read_ply: {path}: unknown property type {t!r} in element {name}")
        if name == "face":
            if len(props) != 1 or not lists:
                raise ValueError(f"read_ply: {path}: the face element must hold exactly one list property")
            _, _, ct, it = props[0]
            if _PLY_TYPES[ct] != "u1" or _PLY_TYPES[it] not in ("i4", "u4"):
                raise ValueError(f"read_ply: {path}: face list '{ct} {it}' is not supported (uchar count, int / uint indices)")
            rec = np.dtype([("n", "u1"), ("i", "<" + _PLY_TYPES[it], (3,))])
            if count:
                n0 = data[off] if off < len(data) else 3
                if n0 != 3:
                    raise ValueError(f"read_ply: {path}: a face has {n0} vertices; only triangles are supported")
            if off + count * rec.itemsize > len(data):
                raise ValueError(f"read_ply: {path}: truncated face data (or faces that are not triangles)")
            fd = np.frombuffer(data, rec, count, off)
            if count and not (fd["n"] == 3).all():
                raise ValueError(f"read_ply: {path}: only triangles are supported (a face with another vertex count found)")
            if count and _PLY_TYPES[it] == "u4" and fd["i"].max() >= 2 ** 31:
                raise ValueError(f"read_ply: {path}: vertex index >= 2^31")
            faces = fd["i"].astype(np.int32).reshape(-1, 3)
            off += count * rec.itemsize
        else:
            if lists:
                raise ValueError(f"read_ply: {path}: list property in element {name} is not supported")
            rec = np.dtype([(p[1], "<" + _PLY_TYPES[p[2]]) for p in props])
            if off + count * rec.itemsize > len(data):
                raise ValueError(f"read_ply: {path}: truncated data in element {name}")
            if name == "vertex":
                vert = np.frombuffer(data, rec, count, off)
            off += count * rec.itemsize
    if vert is None:
        raise ValueError(f"read_ply: {path}: no vertex element")
    have = vert.dtype.names or ()
    if not all(a in have for a in "xyz"):
        raise ValueError(f"read_ply: {path}: vertex properties x, y, z are missing")
    out = {"verts": np.stack([vert[a].astype(np.float32) for a in "xyz"], 1).reshape(-1, 3), "faces": faces}
    if all(c in have for c in ("red", "green", "blue")):
        out["colors"] = np.stack([vert[c].astype(np.uint8) for c in ("red", "green", "blue")], 1).reshape(-1, 3)
    if "label" in have:
        out["labels"] = vert["label"].astype(np.int32)
    return out


def load_poses(path) -> np.ndarray:
    """Trajectory text file, 16 floats per line (a row-major camera-to-world matrix) -> float64 [K,4,4], as stored: the
    reference's load_poses also negates columns 1 and 2, which ``cull_mesh(flip_yz=True)`` does here."""
    poses = []
    with open(path, "r") as f:
        for n, line in enumerate(f):
            tok = line.split()
            if not tok:
                continue
            if len(tok) != 16:
                raise ValueError(f"load_poses: {path}: line {n + 1} holds {len(tok)} numbers, not 16")
            poses.append(np.array([float(t) for t in tok], np.float64).reshape(4, 4))
    return np.stack(poses) if poses else np.zeros((0, 4, 4), np.float64)


def world_to_camera(c2w, flip_yz=True) -> np.ndarray:
    """c2w [K,4,4] -> fp32 [K,4,4] world-to-camera: columns 1 and 2 negated with ``flip_yz`` (cull_mesh.py:15-16,
    eval_3d.py:68-69), inverted in float64 (np.linalg.inv, as the reference) and rounded to fp32."""
    c = torch.as_tensor(c2w).detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
    c = np.array(c, dtype=np.float64).reshape(-1, 4, 4)
    if flip_yz:
        c[:, :3, 1] *= -1.0
        c[:, :3, 2] *= -1.0
    return np.linalg.inv(c).astype(np.float32) if len(c) else np.zeros((0, 4, 4), np.float32)


def cull_mesh(verts, faces, c2w, H, W, fx, fy, cx, cy, flip_yz=True, compact=False):
    """cull_mesh.py: keep the faces with at least one vertex some pose of ``c2w`` [K,4,4] sees (``ops.frustum_seen``).
    verts [V,3] fp32 and faces [F,3] int32 on the device -> (verts, faces): the vertices as they are (trimesh's update_faces),
    or with ``compact`` only the used ones, the faces re-indexed (``meshing.compact_mesh``)."""
    w2c = torch.from_numpy(world_to_camera(c2w, flip_yz)).to(verts.device)
    seen = ops.frustum_seen(verts, w2c, H, W, fx, fy, cx, cy)
    keep = seen[faces.long()].any(1) if faces.shape[0] else torch.zeros(0, dtype=torch.bool, device=verts.device)
    if compact:
        return compact_mesh(verts, faces, keep)[:2]
    return verts, faces[keep]


def _face_areas(verts, faces):
    v = verts.detach().double()[faces.long()]
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return v, 0.5 * torch.sqrt(nx * nx + ny * ny + nz * nz)


def _sample(verts, faces, n, generator, u):
    """sample_surface without its host read: (points, face_idx, total area as a device scalar)."""
    if faces.dim() != 2 or faces.shape[1] != 3 or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"sample_surface: verts [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    F = int(faces.shape[0])
    if F == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    dev = verts.device
    if u is None:
        u = torch.rand(int(n), 3, dtype=torch.float64, device=dev, generator=generator)
    else:
        u = torch.as_tensor(u, dtype=torch.float64).to(dev)
        if u.shape != (int(n), 3):
            raise ValueError(f"sample_surface: u must be [{int(n)}, 3], got {tuple(u.shape)}")
    v, area = _face_areas(verts, faces)
    cum = torch.cumsum(area, 0)
    total = cum[-1]
    face = torch.searchsorted(cum, (u[:, 0] * total).contiguous(), right=False).clamp_(max=F - 1)
    # a zero-area face is never chosen: only u0 = 0 ahead of the first face with an area could land on one; move on to that face
    pos = torch.where(area > 0, torch.arange(F, device=dev), torch.full((F,), F - 1, device=dev))
    face = torch.flip(torch.cummin(torch.flip(pos, (0,)), 0).values, (0,))[face]
    r = u[:, 1:3]
    r = torch.where((r.sum(1) > 1.0)[:, None], r - 1.0, r).abs()
    t = v[face]
    pts = t[:, 0] + r[:, 0:1] * (t[:, 1] - t[:, 0]) + r[:, 1:2] * (t[:, 2] - t[:, 0])
    return pts.float(), face, total


def sample_surface(verts, faces, n, generator=None, u=None):
    """trimesh.sample.sample_surface (eval_3d.py:103-106): n points on the mesh, faces drawn by area.  verts [V,3] fp32, faces
    [F,3] int32 on the device -> (points [n,3] fp32, face_idx [n] int64).  Face areas and the points are float64 (the points
    rounded to fp32 at the end): face of sample i = searchsorted(cumsum(area), u[i,0] * total, 'left'); r = u[i,1:3], where
    r0 + r1 > 1 r -= 1, r = |r|; point = v0 + r0 (v1 - v0) + r1 (v2 - v0).  ``u`` [n,3] float64 uniforms in [0, 1) is drawn
    from ``generator`` on the device unless given.  Zero-area faces are never chosen; a mesh without faces or of total area 0
    raises ValueError (one host read)."""
    pts, face, total = _sample(verts, faces, n, generator, u)
    if not float(total) > 0.0:
        raise ValueError("sample_surface: the mesh has total area 0 (or a non-finite area)")
    return pts, face


def accuracy(gt_pts, rec_pts):
    """eval_3d.py:31-35: mean distance from the reconstructed points to their nearest ground-truth point (float64 device
    scalar, in the unit of the points)."""
    return ops.nearest_points(gt_pts, rec_pts)[0].double().mean()


def completion(gt_pts, rec_pts):
    """eval_3d.py:38-42: mean distance from the ground-truth points to their nearest reconstructed point."""
    return ops.nearest_points(rec_pts, gt_pts)[0].double().mean()


def completion_ratio(gt_pts, rec_pts, dist_th=0.05):
    """eval_3d.py:24-28: the share of ground-truth points closer than ``dist_th`` to a reconstructed point."""
    return (ops.nearest_points(rec_pts, gt_pts)[0] < dist_th).double().mean()


def metrics_3d(rec_verts, rec_faces, gt_verts, gt_faces, n_samples=200000, dist_th=0.05, seed=0, align=False, u_rec=None,
               u_gt=None):
    """calc_3d_metric (eval_3d.py:91-117) -> {"accuracy_cm", "completion_cm", "completion_ratio_pct"}: ``n_samples`` points on
    each mesh (the reconstruction first, from one device generator seeded with ``seed``; or the uniforms ``u_rec`` / ``u_gt``),
    two nearest-point passes, the means in float64 on the device.  One host read at the end carries the three figures and every
    error flag.  ``align=True`` is refused: ``calc_3d_metric`` aligns (the reference's default) and then calls this."""
    if align:
        raise NotImplementedError("metrics_3d: align=True is not implemented here; calc_3d_metric aligns the meshes "
                                  "(align_transformation, the reference's point-to-point ICP) and then measures")
    dev = rec_verts.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    rec_pts, _, rec_area = _sample(rec_verts, rec_faces, n_samples, gen, u_rec)
    gt_pts, _, gt_area = _sample(gt_verts, gt_faces, n_samples, gen, u_gt)
    d_acc, _, st_acc = ops.nearest_points_launch(gt_pts, rec_pts)
    d_comp, _, st_comp = ops.nearest_points_launch(rec_pts, gt_pts)
    out = torch.stack((d_acc.double().mean() * 100.0, d_comp.double().mean() * 100.0,
                       (d_comp < dist_th).double().mean() * 100.0, rec_area, gt_area, st_acc[0].double(),
                       st_comp[0].double())).cpu().tolist()
    if not (out[3] > 0.0 and out[4] > 0.0):
        raise ValueError("metrics_3d: a mesh has total area 0 (or a non-finite area)")
    if out[5] or out[6]:
        raise ValueError("metrics_3d: non-finite coordinate in a mesh")
    return {"accuracy_cm": out[0], "completion_cm": out[1], "completion_ratio_pct": out[2]}


def align_transformation(rec_verts, gt_verts, threshold=0.1, return_info=False):
    """get_align_transformation (eval_3d.py:45-59): the rigid motion that registers the reconstruction's vertices rec_verts
    [V,3] to the ground truth's gt_verts [W,3] by point-to-point ICP from the identity, correspondence distance ``threshold``,
    open3d's default criteria (30 iterations, relative fitness and rmse 1e-6) -> float64 [4,4] on the device; with
    ``return_info`` also the dict of ``ops.icp_point_to_point``."""
    info = ops.icp_point_to_point(rec_verts, gt_verts, max_dist=threshold)
    return (info["transformation"], info) if return_info else info["transformation"]


def apply_transform(verts, T):
    """mesh.apply_transform(T) for the vertices: verts [V,3] -> fp32 [V,3] = R v + t, computed in float64 and rounded once."""
    T = torch.as_tensor(T, dtype=torch.float64).to(verts.device)
    if T.shape != (4, 4):
        raise ValueError(f"apply_transform: T must be [4,4], got {tuple(T.shape)}")
    return (verts.detach().double() @ T[:3, :3].T + T[:3, 3]).float()


def calc_3d_metric(rec_verts, rec_faces, gt_verts, gt_faces, align=True, threshold=0.1, n_samples=200000, dist_th=0.05, seed=0,
                   u_rec=None, u_gt=None):
    """calc_3d_metric (eval_3d.py:91-117) with the reference's default: with ``align`` the reconstruction's vertices are first
    registered to the ground truth's (``align_transformation``) and moved (``apply_transform``); then ``metrics_3d`` -> its dict
    plus "transformation" (float64 [4,4] on the device; the identity without ``align``) and, with ``align``, "icp" (fitness,
    inlier_rmse, iterations, converged of the registration)."""
    if align:
        T, info = align_transformation(rec_verts, gt_verts, threshold, return_info=True)
        rec_verts = apply_transform(rec_verts, T)
    else:
        T, info = torch.eye(4, dtype=torch.float64, device=rec_verts.device), None
    out = metrics_3d(rec_verts, rec_faces, gt_verts, gt_faces, n_samples=n_samples, dist_th=dist_th, seed=seed, align=False,
                     u_rec=u_rec, u_gt=u_gt)
    out["transformation"] = T
    if info is not None:
        out["icp"] = {k: info[k] for k in ("fitness", "inlier_rmse", "correspondences", "iterations", "converged")}
    return out


# ------------------------------------------------------------------------------------------- 2-D evaluation (eval_2d.py)
def psnr(pred, gt, depth=None):
    """eval_2d.py:299-301: -10 log10(mse) with the mse over the three channels of the pixels with ``depth`` > 0 (every pixel without
    ``depth``).  pred, gt [H,W,3] or [F,H,W,3] on the device -> float64 device tensor (0-d or [F]); NaN where no pixel is valid."""
    return -10.0 * torch.log10(ops.ms_ssim(pred, gt, depth)["mse"])


def ms_ssim(pred, gt):
    """eval_2d.py:302: pytorch_msssim's ms_ssim(data_range=1.0, size_average=True) per image pair (the reference passes the images
    transposed to [1,3,W,H]; the definition is symmetric in the two axes) -> float64 device tensor (0-d or [F])."""
    return ops.ms_ssim(pred, gt)["ms_ssim"]


LPIPS_FEATURE_KEYS = (0, 3, 6, 8, 10)             # torchvision AlexNet: features.{k}.weight / .bias of the five convolutions


def _state_tensor(sd, key, shape, path):
    if key not in sd:
        raise ValueError(f"load_lpips_weights: {path}: key {key!r} is missing")
    t = sd[key]
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"load_lpips_weights: {path}: key {key!r} holds a {type(t).__name__}, not a tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"load_lpips_weights: {path}: key {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().float()


def load_lpips_weights(alexnet_path, lin_path) -> ops.LpipsWeights:
    """The LPIPS parameters from two files the caller has: ``alexnet_path`` = torchvision's AlexNet state dict (keys
    ``features.{0,3,6,8,10}.{weight,bias}``; other keys are ignored), ``lin_path`` = lpips v0.1's ``alex.pth`` (keys
    ``lin{0..4}.model.1.weight``, each [1,C,1,1]); both read with ``torch.load(..., weights_only=True)``.  Every shape is checked;
    a missing key, a wrong shape and a non-tensor entry raise ValueError naming the key.  -> ``ops.LpipsWeights`` (the device
    copies and the packed weight images are made once per device, on first use).  No file is fetched."""
    alex = torch.load(alexnet_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    for sd, path in ((alex, alexnet_path), (lin, lin_path)):
        if not isinstance(sd, dict):
            raise ValueError(f"load_lpips_weights: {path} holds a {type(sd).__name__}, not a state dict")
    convs, lins = [], []
    for l, (k, cin, cout, ks, _, _, _) in enumerate(ops.LPIPS_LAYERS):
        convs.append((_state_tensor(alex, f"features.{k}.weight", (cout, cin, ks, ks), alexnet_path),
                      _state_tensor(alex, f"features.{k}.bias", (cout,), alexnet_path)))
        lins.append(_state_tensor(lin, f"lin{l}.model.1.weight", (1, cout, 1, 1), lin_path).reshape(cout))
    return ops.LpipsWeights(convs, lins)


def lpips(pred, gt, weights, method=None):
    """eval_2d.py:304: LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True) per image pair, pred, gt [H,W,3] or
    [F,H,W,3] in [0,1] (``ops.lpips``) -> float64 tensor (0-d or [F]) on the images' device."""
    return ops.lpips(pred, gt, weights, method)["lpips"]


def semantic_metrics(conf, n_invalid=None) -> dict:
    """eval_2d.py:180-213 from the confusion matrix conf [C,C] (rows = ground truth; ``ops.label_confusion``), on the host in
    float64 -> {"miou", "fwiou", "class_avg_accuracy", "total_accuracy", "iou" [C] (NaN for classes in neither image)}.  The
    reference's classes are the labels present in the ground truth: with row = conf.sum(1), col = conf.sum(0), present = row > 0,
    iou_c = conf[c,c] / (row_c + col_c - conf[c,c]); miou = mean of iou over the present classes; fwiou = sum over them of
    iou_c row_c / sum row; class_avg_accuracy = mean over them of conf[c,c] / (row_c + 1e-10); total_accuracy = trace / sum.
    ``n_invalid`` != 0 (labels outside [0, C)) raises ValueError: the reference would treat each out-of-range value as one more
    class (one more term in the means for a ground-truth value, misses for a predicted one), which a C x C matrix cannot hold."""
    c = conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"semantic_metrics: conf must be [C,C], got {c.shape}")
    if n_invalid is not None and int(n_invalid) != 0:
        raise ValueError(f"semantic_metrics: {int(n_invalid)} pixels hold a label outside [0, {c.shape[0]})")
    c = c.astype(np.float64)
    row, col, diag = c.sum(1), c.sum(0), np.diag(c)
    total = row.sum()
    if not total > 0:
        raise ValueError("semantic_metrics: the confusion matrix is empty")
    present = row > 0
    union = row + col - diag
    iou = np.full(c.shape[0], np.nan)
    iou[union > 0] = diag[union > 0] / union[union > 0]
    return {"miou": float(iou[present].mean()), "fwiou": float((iou[present] * row[present]).sum() / total),
            "class_avg_accuracy": float((diag[present] / (row[present] + 1e-10)).mean()),
            "total_accuracy": float(diag.sum() / total), "iou": iou}


def render_metrics(mapper, frames, indices=None, every=10, features=None, n_pts_batch=None, jitters=None, stem=None, truncate=False,
                   code_method=None, lpips=None, lpips_method=None) -> dict:
    """The loop of eval_2d.py:398-411: for each chosen frame i (``indices``, or every ``every``-th frame) ``mapper.render_frame``
    from ``frames["est_c2w"][i]``, then PSNR over the pixels with gt_depth > 0, MS-SSIM and the four semantic figures of the
    arg-max label image against ``frames["gt_label"][i]`` (classes = the decoder's n_class).  The metric kernels are queued behind
    each render; the host reads everything back once, after the last frame.  ``features`` / ``jitters``: per chosen frame, what
    ``render_frame`` takes (None: no 2-D code / fresh draws).  ``stem``: the 2-D code from reference views, computed chunk by
    chunk (``render_frame(refer_frames=...)``; exclusive with ``features``) -- "self" = the frame itself at its estimated pose as
    the single view, what novel_view_render renders with (eval_2d.py:239-240), or a callable i -> refer_frames for anything else;
    ``truncate`` / ``code_method`` are passed through.  -> {"frames": [i...], "psnr", "ssim", "miou", "fwiou",
    "class_avg_accuracy", "total_accuracy": {"per_frame": float64 array, "mean": float}}.  ``lpips``: an ``ops.LpipsWeights``
    (``load_lpips_weights``): each frame's LPIPS is queued behind its MS-SSIM and the result gains "lpips": {"per_frame", "mean"},
    still with the one host read (``lpips_method``: ``ops.lpips``'s ``method``); without it the launches and the result are what they
    were, with no "lpips" key."""
    n = int(frames["gt_color"].shape[0])
    idx = list(range(0, n, int(every))) if indices is None else [int(i) for i in indices]
    if not idx:
        raise ValueError("render_metrics: no frames chosen")
    for name, seq in (("features", features), ("jitters", jitters)):
        if seq is not None and len(seq) != len(idx):
            raise ValueError(f"render_metrics: {name} must hold one entry per chosen frame ({len(idx)}), got {len(seq)}")
    if stem is not None and features is not None:
        raise ValueError("render_metrics: stem= and features= are exclusive")
    if stem is not None and stem != "self" and not callable(stem):
        raise ValueError(f"render_metrics: stem must be None, 'self' or a callable i -> refer_frames, got {stem!r}")
    if lpips is not None and not isinstance(lpips, ops.LpipsWeights):
        raise ValueError("render_metrics: lpips must be None or the weights load_lpips_weights returns")
    dev = mapper.device
    n_class = int(mapper.decoder.n_class)
    vals, mses, confs, bads, lps = [], [], [], [], []
    for k, i in enumerate(idx):
        gt_color, gt_depth, gt_label = frames["gt_color"][i], frames["gt_depth"][i], frames["gt_label"][i]
        refer = None
        if stem == "self":
            refer = {"gt_color": gt_color[None], "est_c2w": frames["est_c2w"][i][None]}
        elif stem is not None:
            refer = stem(i)
        color, _, label = mapper.render_frame(gt_color, gt_depth, gt_label, frames["est_c2w"][i],
                                              features=None if features is None else features[k], n_pts_batch=n_pts_batch,
                                              jitter=None if jitters is None else jitters[k], refer_frames=refer,
                                              truncate=truncate, code_method=code_method)
        v, m, _, _ = ops.ms_ssim_launch(color, gt_color.to(dev), gt_depth.to(dev))
        if lpips is not None:
            lps.append(ops.lpips_launch(color, gt_color.to(dev), lpips, lpips_method)[0])
        cf, bad = ops.label_confusion(gt_label.to(dev).reshape(label.shape), label, n_class)
        vals.append(v), mses.append(m), confs.append(cf.reshape(-1)), bads.append(bad.reshape(1))
    host = torch.cat((torch.cat(vals), torch.cat(mses), torch.cat(bads).double(), torch.cat(confs).double()) + tuple(lps)).cpu().numpy()
    F = len(idx)
    ssim, mse, bad = host[:F], host[F:2 * F], host[2 * F:3 * F]
    conf = host[3 * F:3 * F + F * n_class * n_class].reshape(F, n_class, n_class)
    sem = [semantic_metrics(conf[k], bad[k]) for k in range(F)]
    per = {"psnr": -10.0 * np.log10(mse), "ssim": ssim.copy()}
    for key in ("miou", "fwiou", "class_avg_accuracy", "total_accuracy"):
        per[key] = np.array([s[key] for s in sem], np.float64)
    if lpips is not None:
        per["lpips"] = host[3 * F + F * n_class * n_class:].copy()
    out = {key: {"per_frame": v, "mean": float(np.mean(v))} for key, v in per.items()}
    out["frames"] = idx
    return out


# ------------------------------------------------------------------------------------------- trajectory error (eval_ate.py)
def evaluate_ate(gt_c2w, est_c2w, scale=1.0) -> dict:
    """eval_ate.py: the absolute trajectory error of the estimated camera centres against the ground truth's after the
    closed-form rigid alignment (Horn / Kabsch), in numpy float64.  gt_c2w, est_c2w [K,4,4] (tensors or arrays).  Frames whose
    ground-truth pose holds inf or NaN are dropped from both lists (convert_poses); translations are divided by ``scale``; with the
    centred clouds e (estimate) and g, W = sum e g^T, U S V^T = svd(W^T), rot = U diag(1, 1, det(U) det(V^T)) V^T, trans = mean g -
    rot mean e; the error of a frame is |rot e + trans - g|.  -> {"compared_pose_pairs", "absolute_translational_error.rmse" /
    ".mean" / ".median" / ".std" / ".min" / ".max", "rot" [3,3], "trans" [3]}.  The reference's time-stamp association is the
    identity here (its stamps are the frame indices) and nothing is plotted.  Fewer than two valid pairs raise ValueError."""
    to_np = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)
    g, e = to_np(gt_c2w).reshape(-1, 4, 4), to_np(est_c2w).reshape(-1, 4, 4)
    if g.shape != e.shape:
        raise ValueError(f"evaluate_ate: {g.shape[0]} ground-truth poses and {e.shape[0]} estimated poses")
    keep = np.isfinite(g).all(axis=(1, 2))
    gp, ep = g[keep, :3, 3] / float(scale), e[keep, :3, 3] / float(scale)
    if gp.shape[0] < 2:
        raise ValueError(f"evaluate_ate: {gp.shape[0]} valid pose pairs (at least 2 are needed)")
    mg, me = gp.mean(0), ep.mean(0)
    Wm = (ep - me).T @ (gp - mg)
    U, _, Vt = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vt
    trans = mg - rot @ me
    err = np.sqrt((((ep @ rot.T) + trans - gp) ** 2).sum(1))
    return {"compared_pose_pairs": int(err.shape[0]),
            "absolute_translational_error.rmse": float(np.sqrt(err @ err / err.shape[0])),
            "absolute_translational_error.mean": float(err.mean()), "absolute_translational_error.median": float(np.median(err)),
            "absolute_translational_error.std": float(err.std()), "absolute_translational_error.min": float(err.min()),
            "absolute_translational_error.max": float(err.max()), "rot": rot, "trans": trans}


# ------------------------------------------------------------------------------------------- Depth L1 (eval_3d.py:120-210)
DEPTH_L1_CAM = dict(H=500, W=500, fx=300.0, fy=300.0, cx=249.5, cy=249.5)     # calc_2d_metric: focal 300, cx = H/2 - 0.5, cy = W/2 - 0.5
DEPTH_STACK_BUDGET = 512 << 20         # bytes the two depth stacks of one chunk of views may take (256 views at 500 x 500)


def _host64(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def view_box(verts):
    """get_cam_position (eval_3d.py:120-128) -> (extents float64 [3], transform float64 [4,4]): the box cameras are drawn from.
    The reference takes trimesh's minimum-volume ORIENTED bounding box of the ground-truth mesh; that search is not available
    here, and this function takes the AXIS-ALIGNED box of the vertices instead (the two agree for a room whose walls follow the
    axes; pass your own ``(extents, transform)`` to ``sample_views`` otherwise).  Then, as the reference: extents scaled by (0.3,
    0.7, 0.7), the transform (box frame -> world: the translation to the box centre) with +0.4 on its z translation."""
    v = _host64(verts).reshape(-1, 3)
    if not len(v) or not np.isfinite(v).all():
        raise ValueError("view_box: no vertices, or a non-finite coordinate")
    lo, hi = v.min(0), v.max(0)
    extents = (hi - lo) * np.array([0.3, 0.7, 0.7])
    transform = np.eye(4)
    transform[:3, 3] = 0.5 * (lo + hi)
    transform[2, 3] += 0.4
    return extents, transform


def look_at(origin, target, up=(0.0, 0.0, -1.0)):
    """viewmatrix (eval_3d.py:15-21) as a 4x4 camera-to-world matrix (float64): the camera at ``origin`` looks at ``target``; z =
    normalize(target - origin), x = normalize(up x z), y = normalize(z x x) (x right, y down, z forward)."""
    o = np.asarray(origin, np.float64).reshape(3)
    z = np.asarray(target, np.float64).reshape(3) - o
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64).reshape(3), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    y = y / np.linalg.norm(y)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, o
    return m


def _draw_views(rs, extents, transform, k):
    """k candidate poses in draw order: per candidate rand(3) for the origin, then uniform(-10000, 10000, 3) for the target."""
    out = np.empty((k, 4, 4))
    for i in range(k):
        origin = transform[:3, :3] @ ((rs.rand(3) - 0.5) * extents) + transform[:3, 3]
        target = np.round(rs.uniform(-10000.0, 10000.0, 3), 2)
        out[i] = look_at(origin, target)
    return out


def sample_views(extents, transform, n, unseen_pts=None, cam=None, seed=0, batch=256):
    """The view sampler of calc_2d_metric (eval_3d.py:159-178) -> c2w float64 [n,4,4] (numpy).  Origin: uniform in the box, as
    trimesh.sample.volume_rectangular draws it, (rand(3) - 0.5) * extents moved by ``transform``; target: uniform in +-10000 per
    axis, rounded to 2 decimals; pose = ``look_at``.  All draws come from one ``numpy.random.RandomState(seed)`` (the reference
    mixes numpy's and Python's global generators, unseeded): the same seed gives the same views.  With ``unseen_pts`` [N,3] (device
    tensor) a candidate that sees any of them (check_proj with the intrinsics ``cam``, default ``DEPTH_L1_CAM``) is rejected:
    candidates are drawn ``batch`` at a time (at least as many as are still needed), tested by ``ops.views_see_any`` with one
    host read per batch, and accepted in draw order until n are.  Without ``unseen_pts`` nothing is rejected and no GPU is needed.
    2000 batches without n accepted views raise RuntimeError."""
    extents = np.asarray(extents, np.float64).reshape(3)
    transform = np.asarray(transform, np.float64).reshape(4, 4)
    n = int(n)
    rs = np.random.RandomState(int(seed))
    if unseen_pts is None or n == 0:
        return _draw_views(rs, extents, transform, n)
    cam = dict(DEPTH_L1_CAM if cam is None else cam)
    out = np.empty((n, 4, 4))
    got = 0
    for _ in range(2000):
        cand = _draw_views(rs, extents, transform, max(int(batch), n - got))
        w2c = torch.from_numpy(world_to_camera(cand, flip_yz=True)).to(unseen_pts.device)
        sees = ops.views_see_any(unseen_pts, w2c, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]).cpu().numpy()
        ok = cand[~sees][:n - got]
        out[got:got + len(ok)] = ok
        got += len(ok)
        if got == n:
            return out
    raise RuntimeError(f"sample_views: only {got} of {n} views accepted after 2000 batches (the unseen cloud is visible from "
                       f"almost everywhere in the box)")


def _depth_cam(H, W, focal, cx, cy):
    return dict(H=int(H), W=int(W), fx=float(focal), fy=float(focal), cx=H / 2.0 - 0.5 if cx is None else float(cx),
                cy=W / 2.0 - 0.5 if cy is None else float(cy))


def _view_chunk(H, W, budget):
    return max(1, int(budget) // (2 * 4 * int(H) * int(W)))


def render_depth(verts, faces, c2w, H=500, W=500, focal=300.0, cx=None, cy=None, z_near=0.01, z_far=20.0, method="auto"):
    """Depth images [V,H,W] fp32 on the device of the mesh from the camera-to-world poses c2w [V,4,4] (x right, y down, z
    forward: what ``look_at`` / ``sample_views`` return), in place of open3d's visualiser (eval_3d.py:180-204): ``ops.
    rasterize_depth`` with the reference's intrinsics as defaults (cx = H/2 - 0.5, cy = W/2 - 0.5, as the reference writes them).
    The poses are inverted in float64 on the host and rounded to fp32.  open3d derives its near plane from the scene's bounding
    box; here it is the parameter ``z_near``."""
    cam = _depth_cam(H, W, focal, cx, cy)
    w2c = torch.from_numpy(world_to_camera(c2w, flip_yz=False)).to(verts.device)
    return ops.rasterize_depth(verts, faces, w2c, cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_near, z_far, method)


def depth_l1(rec_verts, rec_faces, gt_verts, gt_faces, c2w, H=500, W=500, focal=300.0, cx=None, cy=None, z_near=0.01, z_far=20.0,
             method="auto", budget=DEPTH_STACK_BUDGET) -> dict:
    """The loop of eval_3d.py:180-210 over given poses c2w [V,4,4]: both meshes rendered to depth, mean |d_gt - d_rec| per view
    over all pixels -> {"per_view": float64 array [V] (metres), "depth_l1_cm": their mean x 100}.  The views go through in chunks
    whose two depth stacks stay under ``budget`` bytes; one host read at the end carries the per-view errors and the status words
    (a non-finite vertex raises ValueError).  The face indices are validated up front (one host read per mesh)."""
    cam = _depth_cam(H, W, focal, cx, cy)
    dev = gt_verts.device
    w2c = torch.from_numpy(world_to_camera(c2w, flip_yz=False)).to(dev)
    V = int(w2c.shape[0])
    if V == 0:
        raise ValueError("depth_l1: no views")
    for v, f in ((rec_verts, rec_faces), (gt_verts, gt_faces)):
        ops._check_face_indices(ops._raster_arguments(v, f, w2c, cam["H"], cam["W"], method)[1], int(v.shape[0]))
    step = _view_chunk(cam["H"], cam["W"], budget)
    errs, stats = [], []
    args = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], z_near, z_far, method)
    for lo in range(0, V, step):
        d_gt, s_gt = ops.rasterize_depth_launch(gt_verts, gt_faces, w2c[lo:lo + step], *args)
        d_rec, s_rec = ops.rasterize_depth_launch(rec_verts, rec_faces, w2c[lo:lo + step], *args)
        errs.append(ops.depth_l1(d_gt, d_rec))
        stats += [s_gt[:1], s_rec[:1]]
    host = torch.cat(errs + [s.double() for s in stats]).cpu().numpy()
    if host[V:].any():
        raise ValueError("depth_l1: non-finite coordinate in a mesh")
    per = host[:V].copy()
    return {"per_view": per, "depth_l1_cm": float(per.mean() * 100.0)}


def calc_2d_metric(rec_verts, rec_faces, gt_verts, gt_faces, align=True, n_imgs=1000, unseen_pts=None, seed=0, threshold=0.1,
                   box=None, H=500, W=500, focal=300.0, z_near=0.01, z_far=20.0, method="auto", budget=DEPTH_STACK_BUDGET) -> dict:
    """calc_2d_metric (eval_3d.py:131-210) under its own name: with ``align`` the reconstruction is first registered to the ground
    truth (``align_transformation`` / ``apply_transform``, as ``calc_3d_metric``); ``n_imgs`` views are drawn inside ``box`` =
    (extents, transform) (default ``view_box(gt_verts)``) by ``sample_views`` (rejecting those that see ``unseen_pts``, the
    reference's ``*_pc_unseen.npy`` cloud, when given); then ``depth_l1`` -> its dict plus "c2w" (the views) and
    "transformation"."""
    if align:
        T = align_transformation(rec_verts, gt_verts, threshold)
        rec_verts = apply_transform(rec_verts, T)
    else:
        T = torch.eye(4, dtype=torch.float64, device=rec_verts.device)
    extents, transform = view_box(gt_verts) if box is None else box
    cam = _depth_cam(H, W, focal, None, None)
    c2w = sample_views(extents, transform, n_imgs, unseen_pts=unseen_pts, cam=cam, seed=seed)
    out = depth_l1(rec_verts, rec_faces, gt_verts, gt_faces, c2w, H=H, W=W, focal=focal, z_near=z_near, z_far=z_far, method=method,
                   budget=budget)
    out["c2w"] = c2w
    out["transformation"] = T
    return out
