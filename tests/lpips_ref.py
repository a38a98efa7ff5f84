"""Float64 restatement of LPIPS (AlexNet) as include/dns_hip.h defines it: lpips 0.1.4 as torchmetrics 0.11.1 calls it with
net_type='alex', normalize=True (reference eval_2d.py:81-82,304), written from the published definition.  Neither package nor any
pretrained weight is available to the tests, so the weights are drawn from a seed and this file is what the kernels are held to.

    lpips_ref(pred [F,H,W,3], gt [F,H,W,3], weights) -> dict
        "lpips" [F], "layers" [F,5] float64;
        "pred", "gt": per image stack a list of five dicts {"x": the layer's input [F,H_l,W_l,Cin] (scaled image / pooled map),
        "pre": the convolution + bias before the ReLU, "A": conv(|x|, |w|), "feat": the feature}, everything float64 channels-last.

``weights``: {"convs": [(weight [Cout,Cin,k,k], bias [Cout])] x 5, "lins": [lin [C]] x 5} (fp32 values, widened exactly).  The
convolution is the unfolded tap matrix [F h w, k k Cin] times the weight matrix: there is no library convolution in the reference.
"""
import numpy as np
import torch

U = 2.0 ** -24
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (Cin, Cout, kernel, stride, pad, pooled input) of the five AlexNet convolutions; state-dict indices 0, 3, 6, 8, 10
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))
FEATURE_KEYS = (0, 3, 6, 8, 10)
SIZES = ((31, 31), (67, 95), (131, 70))
SEED = 7                                               # of the pairs the tests share (weights: seed 0)

# Tolerances of a fp32 evaluation against this restatement, relative, per kind of pair: (lpips, each layers entry).
# MEASURED on the CPU: the error of the fp32 composition of F.conv2d / F.max_pool2d (ops.lpips(method="torch")) on exactly the
# tests' inputs (SIZES x F in (1, 2), pair seed 7, weight seed 0), the largest over those cases:
#     indep: lpips 1.5e-7, layers 1.35e-6        near: lpips 2.67e-6, layers 6.4e-6
# (near: lpips ~ 5e-4 is a sum of squares of differences ~ 2e-2 of normalised features, so a feature error of 1e-6 is 5e-5 of a
# difference).  ALLOWED: 8 times the measured figure -- another summation order of the convolutions moves the error, and nothing
# else should.  `same` pairs must give exactly 0.
MEASURED_FP32 = {"indep": (1.5e-7, 1.35e-6), "near": (2.67e-6, 6.4e-6)}
TOL = {k: (8 * a, 8 * b) for k, (a, b) in MEASURED_FP32.items()}


def _f64(v):
    return torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).double()


def scale_image(x):
    """step 1: clamp to [0,1] (a NaN stays), 2x - 1, (. - shift) / scale; the fp32 constants of the definition widened"""
    x = _f64(x)
    x = torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))
    shift = torch.tensor(SHIFT, dtype=torch.float32).double()
    scale = torch.tensor(SCALE, dtype=torch.float32).double()
    return (2.0 * x - 1.0 - shift) / scale


def out_extent(size, ks, stride, pad):
    return (size + 2 * pad - ks) // stride + 1


def taps(x, ks, stride, pad):
    """[n,H,W,C] float64 -> [n,h,w,ks ks C], column (ky ks + kx) C + c = the zero-padded value at (s oy + ky - pad, s ox + kx - pad, c)"""
    n, H, W, C = x.shape
    h, w = out_extent(H, ks, stride, pad), out_extent(W, ks, stride, pad)
    p = torch.zeros(n, H + 2 * pad, W + 2 * pad, C, dtype=x.dtype)
    p[:, pad:pad + H, pad:pad + W] = x
    cols = []
    for ky in range(ks):
        for kx in range(ks):
            cols.append(p[:, ky:ky + stride * (h - 1) + 1:stride, kx:kx + stride * (w - 1) + 1:stride, :])
    return torch.cat(cols, -1)


def conv64(x, weight, bias, stride, pad):
    """-> (conv + bias, A = conv(|x|, |w|)) [n,h,w,Cout] float64"""
    x, wt = _f64(x), _f64(weight)
    cout, cin, ks, _ = wt.shape
    wm = wt.permute(2, 3, 1, 0).reshape(ks * ks * cin, cout)
    t = taps(x, ks, stride, pad)
    pre = t @ wm
    if bias is not None:
        pre = pre + _f64(bias)
    return pre, t.abs() @ wm.abs()


def relu64(x):
    return torch.where(x != x, x, torch.clamp(x, min=0.0))


def max_pool64(x):
    """3x3, stride 2, no padding, floor mode; a NaN in a window wins"""
    n, h, w, C = x.shape
    ph, pw = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    wins = torch.stack([x[:, dy:dy + 2 * (ph - 1) + 1:2, dx:dx + 2 * (pw - 1) + 1:2] for dy in range(3) for dx in range(3)])
    out = wins.max(0).values
    return torch.where((wins != wins).any(0), torch.full_like(out, float("nan")), out)


def tower(images, weights):
    """-> the five layer dicts of an image stack [F,H,W,3]"""
    x = scale_image(images)
    out = []
    for (w, b), (_, _, _, stride, pad, pooled) in zip(weights["convs"], LAYERS):
        if pooled:
            x = max_pool64(x)
        pre, A = conv64(x, w, b, stride, pad)
        feat = relu64(pre)
        out.append({"x": x, "pre": pre, "A": A, "feat": feat})
        x = feat
    return out


def head64(fa, fb, lin):
    """d [F] of one layer from features [F,h,w,C]"""
    fa, fb, lin = _f64(fa), _f64(fb), _f64(lin)
    na = fa / (torch.sqrt((fa * fa).sum(-1, keepdim=True)) + 1e-10)
    nb = fb / (torch.sqrt((fb * fb).sum(-1, keepdim=True)) + 1e-10)
    return (((na - nb) ** 2) * lin).sum(-1).flatten(1).mean(1)


def lpips_ref(pred, gt, weights):
    if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[-1] != 3:
        raise ValueError(f"lpips_ref: two [F,H,W,3] stacks, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if min(pred.shape[1], pred.shape[2]) < 31:
        raise ValueError("lpips_ref: sides below 31 leave the second pool empty")
    tp, tg = tower(pred, weights), tower(gt, weights)
    layers = torch.stack([head64(a["feat"], b["feat"], lin) for a, b, lin in zip(tp, tg, weights["lins"])], 1)
    return {"lpips": layers.sum(1), "layers": layers, "pred": tp, "gt": tg}


def random_weights(seed):
    """He-normal convolutions (std sqrt(2 / K), K = k k Cin), bias 0.1 randn, lin uniform in [0, 0.1]"""
    g = torch.Generator().manual_seed(seed)
    convs, lins = [], []
    for cin, cout, ks, _, _, _ in LAYERS:
        convs.append((torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (ks * ks * cin)) ** 0.5, torch.randn(cout, generator=g) * 0.1))
    for _, cout, _, _, _, _ in LAYERS:
        lins.append(torch.rand(cout, generator=g) * 0.1)
    return {"convs": convs, "lins": lins}


def random_pairs(seed, F, H, W, kind):
    """kind: 'indep' = two independent uniform images; 'near' = gt + 0.02 randn (leaves [0,1] here and there: the clamp is
    exercised); 'same' = identical images.  -> (pred, gt) [F,H,W,3] fp32"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(F, H, W, 3, generator=g)
    if kind == "indep":
        return torch.rand(F, H, W, 3, generator=g), gt
    if kind == "near":
        return gt + 0.02 * torch.randn(F, H, W, 3, generator=g), gt
    if kind == "same":
        return gt.clone(), gt
    raise ValueError(kind)


def state_dicts(weights):
    """The two state dicts with the key names of torchvision's AlexNet and lpips v0.1's alex.pth"""
    alex, lin = {}, {}
    for k, (w, b) in zip(FEATURE_KEYS, weights["convs"]):
        alex[f"features.{k}.weight"], alex[f"features.{k}.bias"] = w.clone(), b.clone()
    for l, v in enumerate(weights["lins"]):
        lin[f"lin{l}.model.1.weight"] = v.clone().view(1, -1, 1, 1)
    return alex, lin


_CACHE = {}


def cached(seed, F, H, W, kind, wseed=0):
    """(pred, gt, weights, lpips_ref(...)) computed once per process and shared by the tests; treat it as read-only"""
    key = (seed, F, H, W, kind, wseed)
    if key not in _CACHE:
        if ("w", wseed) not in _CACHE:
            _CACHE[("w", wseed)] = random_weights(wseed)
        wts = _CACHE[("w", wseed)]
        pred, gt = random_pairs(seed, F, H, W, kind)
        _CACHE[key] = (pred, gt, wts, lpips_ref(pred, gt, wts))
    return _CACHE[key]
