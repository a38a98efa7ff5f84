"""Float64 restatement of the image stem (reference models/layers.py:56-58,95-98: conv 7x7 stride 2 pad 3 without bias,
nn.BatchNorm2d, ReLU) in both normalisation modes, from the parameters, with the error bounds an exact-fp32 implementation must meet.

    stem_ref(images [n,H,W,3], params, batch_stats) -> (y [n,h,w,64] float64, bound [n,h,w,64] float64)

``params``: a dict holding ``conv1.weight`` [64,3,7,7], ``bn1.weight``, ``bn1.bias``, ``bn1.running_mean``, ``bn1.running_var``
(tensors or arrays; the fp32 values are widened exactly) and optionally ``eps`` (1e-5).  Everything is computed in float64 by
unfolding the zero-padded image into the [n h w, 147] tap matrix, so there is no library convolution in the reference.

Bounds (u = 2^-24; c the exact convolution, A = conv(|x|, |w|)):

* frozen (eval() mode), s = gamma / sqrt(var + eps):  |y - y64| <= 160 u (|s| A + |mean s| + |beta|) -- gamma_n of a 147-term fp32
  sum in any order, plus the roundings of s, t and the epilogue; ReLU is 1-Lipschitz.
* batch (train mode, biased variance over n h w), statistics in float64 from the fp32 conv values: with e = 150 u A, e_bar / e_rms its
  per-channel mean / rms over the batch, sigma' = sqrt(var + eps), z = (c - mean) / sigma':
  |y - y64| <= 1.01 |gamma| / sigma' (e + e_bar + |z| e_rms) + 8 u (|gamma z| + |beta|).  The mean moves by at most e_bar, the
  standard deviation by at most e_rms (triangle inequality in L2).
"""
import numpy as np
import torch

U = 2.0 ** -24


def _f64(v):
    return torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).double()


def out_shape(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def taps(images):
    """[n,H,W,3] float64 -> [n, h, w, 147] with column (ky 7 + kx) 3 + c = the zero-padded pixel (2 oy + ky - 3, 2 ox + kx - 3, c)."""
    n, H, W, _ = images.shape
    h, w = out_shape(H, W)
    pad = torch.zeros(n, H + 6, W + 6, 3, dtype=images.dtype)
    pad[:, 3:3 + H, 3:3 + W] = images
    cols = []
    for ky in range(7):
        for kx in range(7):
            cols.append(pad[:, ky:ky + 2 * h - 1:2, kx:kx + 2 * w - 1:2, :])
    return torch.cat(cols, -1)


def conv64(images, weight):
    """The exact convolution c and A = conv(|x|, |w|): [n,h,w,64] float64 each."""
    x, wt = _f64(images), _f64(weight)
    wm = wt.permute(2, 3, 1, 0).reshape(147, 64)
    t = taps(x)
    return t @ wm, t.abs() @ wm.abs()


def stem_ref(images, params, batch_stats):
    eps = float(params.get("eps", 1e-5))
    gamma, beta = _f64(params["bn1.weight"]), _f64(params["bn1.bias"])
    c, A = conv64(images, params["conv1.weight"])
    if not batch_stats:
        mean, var = _f64(params["bn1.running_mean"]), _f64(params["bn1.running_var"])
        s = gamma / torch.sqrt(var + eps)
        y = torch.relu((c - mean) * s + beta)
        bound = 160 * U * (s.abs() * A + (mean * s).abs() + beta.abs())
        return y, bound
    if c.shape[0] * c.shape[1] * c.shape[2] == 1:
        raise ValueError("stem_ref: batch statistics of a single value")
    mean = c.mean((0, 1, 2))
    var = ((c - mean) ** 2).mean((0, 1, 2))                 # biased
    sig = torch.sqrt(var + eps)
    z = (c - mean) / sig
    y = torch.relu(gamma * z + beta)
    e = 150 * U * A
    e_bar = e.mean((0, 1, 2))
    e_rms = torch.sqrt((e ** 2).mean((0, 1, 2)))
    bound = 1.01 * gamma.abs() / sig * (e + e_bar + z.abs() * e_rms) + 8 * U * ((gamma * z).abs() + beta.abs())
    return y, bound


def random_params(seed, weight="he"):
    """Stem parameters with no trivial term: conv weight He-normal (std sqrt(2 / (7 7 64))) or 0.2 randn; random gamma (both signs),
    beta, running mean and running variance."""
    g = torch.Generator().manual_seed(seed)
    std = (2.0 / (7 * 7 * 64)) ** 0.5 if weight == "he" else 0.2
    return {"conv1.weight": torch.randn(64, 3, 7, 7, generator=g) * std,
            "bn1.weight": (0.5 + torch.rand(64, generator=g)) * torch.where(torch.rand(64, generator=g) < 0.25, -1.0, 1.0),
            "bn1.bias": torch.randn(64, generator=g) * 0.3,
            "bn1.running_mean": torch.randn(64, generator=g) * 0.2,
            "bn1.running_var": 0.05 + torch.rand(64, generator=g) * 2.0}


def random_images(seed, n, H, W, kind):
    """kind: 'unit' in [0,1], 'byte' in [0,255], 'flat' = 0.5 + 1e-3 rand (small channel variances)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, H, W, 3, generator=g)
    return {"unit": r, "byte": r * 255.0, "flat": 0.5 + 1e-3 * r}[kind]
