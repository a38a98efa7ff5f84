"""Host definitions of the 2-D evaluation metrics (dns_slam_amd.ops.ms_ssim / label_confusion, dns_slam_amd.evaluation), written
from the formulas in include/dns_hip.h, and the image pairs the tests share."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    """g[k] = exp(-(k-5)^2 / (2 1.5^2)), normalised, in fp32."""
    c = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def pooled_size(s):
    return (s + 2 * (s % 2) - 2) // 2 + 1


def ms_ssim_ref(pred, gt, dtype=torch.float64):
    """pred, gt [H,W,3] (CPU) -> (value float, levels [5,3] float64 tensor: the per-level, per-channel means before relu)."""
    x = pred.detach().cpu().float().to(dtype).permute(2, 0, 1)[None]
    y = gt.detach().cpu().float().to(dtype).permute(2, 0, 1)[None]
    g = window().to(dtype)
    kh, kw = g.view(1, 1, 11, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, 11).repeat(3, 1, 1, 1)
    filt = lambda t: Fn.conv2d(Fn.conv2d(t, kh, groups=3), kw, groups=3)
    terms = []
    for l in range(5):
        mx, my = filt(x), filt(y)
        sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        cs = (2 * sxy + C2) / (sxx + syy + C2)
        if l < 4:
            terms.append(cs.flatten(2).mean(-1)[0])
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = Fn.avg_pool2d(x, 2, padding=pad), Fn.avg_pool2d(y, 2, padding=pad)
        else:
            terms.append(((2 * mx * my + C1) / (mx * mx + my * my + C1) * cs).flatten(2).mean(-1)[0])
    levels = torch.stack(terms).double()
    w = torch.tensor(MS_WEIGHTS, dtype=torch.float64).view(5, 1)
    return float(torch.prod(torch.relu(levels) ** w, 0).mean()), levels


def mse_ref(pred, gt, depth=None):
    """-> (mse float (NaN without a valid pixel), n_valid int): float64 mean of the squared differences over the three channels of
    the pixels with depth > 0."""
    p, g = pred.detach().cpu().float().double(), gt.detach().cpu().float().double()
    m = torch.ones(p.shape[:-1], dtype=torch.bool) if depth is None else depth.detach().cpu() > 0
    n = int(m.sum())
    return (float(((p - g)[m] ** 2).mean()) if n else float("nan")), n


def psnr_ref(pred, gt, depth=None):
    mse, _ = mse_ref(pred, gt, depth)
    return -10.0 * math.log10(mse) if mse == mse else float("nan")


def confusion_ref(gt, pred, n_class):
    """-> (conf [n_class,n_class] int64, rows = gt; n_invalid)."""
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    ok = (g >= 0) & (g < n_class) & (p >= 0) & (p < n_class)
    conf = np.bincount(g[ok] * n_class + p[ok], minlength=n_class * n_class).reshape(n_class, n_class).astype(np.int64)
    return conf, int((~ok).sum())


def semantic_metrics_ref(gt, pred):
    """The four figures the direct way: boolean masks per class of the ground truth, on the label images."""
    g, p = np.asarray(gt).reshape(-1), np.asarray(pred).reshape(-1)
    classes = np.unique(g)
    iou, weight, acc = [], [], []
    for c in classes:
        gm, pm = g == c, p == c
        inter, union = np.logical_and(gm, pm).sum(), np.logical_or(gm, pm).sum()
        iou.append(inter / union if union > 0 else 0.0)
        weight.append(gm.sum() / g.size)
        acc.append(inter / (gm.sum() + 1e-10))
    iou = np.array(iou, np.float64)
    return {"miou": float(iou.mean()), "fwiou": float((iou * np.array(weight, np.float64)).sum()),
            "class_avg_accuracy": float(np.mean(acc)), "total_accuracy": float((g == p).sum() / g.size)}


def ate_ref(gt_xyz, est_xyz):
    """Least-squares rigid alignment of est [K,3] onto gt [K,3] by a route of its own (Horn's quaternion form: the top
    eigenvector of the symmetric 4x4), then the error norms -> (rot, trans, err [K])."""
    g, e = np.asarray(gt_xyz, np.float64), np.asarray(est_xyz, np.float64)
    mg, me = g.mean(0), e.mean(0)
    M = (e - me).T @ (g - mg)                       # M[a,b] = sum e_a g_b
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = M.reshape(-1)
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, v = np.linalg.eigh(N)
    q0, qx, qy, qz = v[:, -1]
    rot = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                    [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                    [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    trans = mg - rot @ me
    return rot, trans, np.sqrt(((e @ rot.T + trans - g) ** 2).sum(1))


# ---- the image pairs --------------------------------------------------------------------------------------------------------
SIZES_CPU = ((161, 163), (176, 161), (240, 320))
SIZES_GPU = ((161, 163), (176, 161), (200, 245))
CASES = ("noise05", "noise005", "affine", "constant", "inverted")      # "inverted" is the deliberately clamped one: value 0
PREMISE = 0.05                                                         # every level term >= this (inverted: a term <= -this per channel)


def smooth(H, W):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
    return torch.stack((0.5 + 0.4 * torch.sin(7 * xx + 3 * yy), 0.5 + 0.4 * torch.cos(5 * yy), xx * yy), -1).float()


def case_pair(name, H, W, seed=0):
    """-> (pred, gt) fp32 [H,W,3] on the CPU."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    s = smooth(H, W)
    if name == "noise05":
        return (s + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), s
    if name == "noise005":
        return s + 0.005 * torch.randn(H, W, 3, generator=g), s
    if name == "affine":
        return 1.2 * s - 0.1, s
    if name == "constant":
        return torch.full((H, W, 3), 0.3), torch.full((H, W, 3), 0.6)
    if name == "inverted":
        return 1.0 - s, s
    raise KeyError(name)


def premise_holds(name, levels):
    """The premise the GPU comparisons rest on: x^0.0448 is unboundedly sensitive near 0, so no term may sit there."""
    if name == "inverted":
        return bool((levels.min(0).values <= -PREMISE).all())
    return bool((levels >= PREMISE).all())
