"""numpy restatement of ops.vis_panels (include/dns_hip.h, "visualisation panels"): fig_plot's 3 x 3 sheet as one uint8 image.
The byte rules are written out here once; tests/test_vis_panels_ref.py holds them to matplotlib, tests/test_gpu_vis_panels.py holds
the kernel to them byte for byte."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_table():
    """The committed csrc/plasma_lut.hpp as uint8 [256,3]."""
    text = open(os.path.join(ROOT, "dns_slam_amd", "csrc", "plasma_lut.hpp")).read()
    body = text.split("= {")[1].split("}")[0]
    return np.array([int(v) for v in re.findall(r"\d+", body)], dtype=np.uint8).reshape(256, 3)


def depth_vmax(gt_depth):
    """The largest finite positive value as fp32; 0 without one."""
    d = np.asarray(gt_depth, dtype=np.float32)
    keep = np.isfinite(d) & (d > 0)
    return np.float32(d[keep].max()) if keep.any() else np.float32(0.0)


def plasma_index(x, vmax):
    """trunc(fl32(fl32(x / vmax) * 256)), below 0 -> 0, 256 and above -> 255; vmax == 0 -> 0.  x fp32, finite."""
    x = np.asarray(x, dtype=np.float32)
    vmax = np.float32(vmax)
    if vmax == 0:
        return np.zeros(x.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = ((x / vmax).astype(np.float32) * np.float32(256.0)).astype(np.float32)
    idx = np.zeros(x.shape, dtype=np.int64)
    mid = (t >= 0) & (t < 256)
    idx[mid] = t[mid].astype(np.int64)
    idx[t >= 256] = 255
    return idx


def scalar_panel(x, vmax, table, background):
    x = np.asarray(x, dtype=np.float32)
    finite = np.isfinite(x)
    out = table[plasma_index(np.where(finite, x, np.float32(0.0)), vmax)]
    out[~finite] = background
    return out


def colour_panel(x):
    """trunc(fl32(clip(x, 0, 1) * 255)); a NaN is taken as 0."""
    x = np.asarray(x, dtype=np.float32)
    c = np.where(x >= 0, np.where(x <= 1, x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return (c * np.float32(255.0)).astype(np.float32).astype(np.uint8)


def map_labels(label, lut):
    lab = np.asarray(label).astype(np.int32)
    if lut is None:
        return lab
    lut = np.asarray(lut, dtype=np.int32)
    inside = (lab >= 0) & (lab < len(lut))
    return np.where(inside, lut[np.clip(lab, 0, len(lut) - 1)], lab).astype(np.int32)


def sheet(gt_color, est_color, gt_depth, est_depth, gt_label, est_label, label_lut=None, max_label=101, gap=8, background=255,
          table=None):
    """-> (uint8 [3H + 2 gap, 3W + 2 gap, 3], vmax fp32)."""
    table = header_table() if table is None else table
    gt_color, est_color = np.asarray(gt_color, np.float32), np.asarray(est_color, np.float32)
    gt_depth, est_depth = np.asarray(gt_depth, np.float32), np.asarray(est_depth, np.float32)
    H, W = gt_depth.shape
    vmax = depth_vmax(gt_depth)
    gl, el = map_labels(gt_label, label_lut), map_labels(est_label, label_lut)
    with np.errstate(all="ignore"):
        rows = [
            [scalar_panel(gt_depth, vmax, table, background), scalar_panel(est_depth, vmax, table, background),
             scalar_panel(np.abs(gt_depth - est_depth), vmax, table, background)],
            [colour_panel(gt_color), colour_panel(est_color), colour_panel(np.abs(gt_color - est_color))],
            [scalar_panel(gl.astype(np.float32), max_label, table, background), scalar_panel(el.astype(np.float32), max_label, table, background),
             scalar_panel(np.abs(gl.astype(np.int64) - el.astype(np.int64)).astype(np.float32), max_label, table, background)],
        ]
    out = np.full((3 * H + 2 * gap, 3 * W + 2 * gap, 3), background, dtype=np.uint8)
    for r in range(3):
        for c in range(3):
            out[r * (H + gap):r * (H + gap) + H, c * (W + gap):c * (W + gap) + W] = rows[r][c]
    return out, vmax


def make_inputs(H, W, seed, n_class=8):
    """A deterministic test frame: colours partly outside [0,1], depths with zeros, labels of n_class classes."""
    rng = np.random.default_rng(seed)
    gt_color = rng.uniform(-0.2, 1.2, size=(H, W, 3)).astype(np.float32)
    est_color = rng.uniform(-0.2, 1.2, size=(H, W, 3)).astype(np.float32)
    gt_depth = rng.uniform(0.0, 6.0, size=(H, W)).astype(np.float32)
    gt_depth[rng.uniform(size=(H, W)) < 0.1] = 0.0
    est_depth = (gt_depth + rng.normal(scale=0.5, size=(H, W))).astype(np.float32)
    gt_label = rng.integers(0, n_class, size=(H, W)).astype(np.int64)
    est_label = rng.integers(0, n_class, size=(H, W)).astype(np.int64)
    return gt_color, est_color, gt_depth, est_depth, gt_label, est_label
