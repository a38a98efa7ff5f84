"""CPU: the float64 restatement of LPIPS (tests/lpips_ref.py) against a float64 composition of torch's own convolution and pool and
against hand-computed values; ops.lpips(method="torch") / evaluation.lpips on CPU tensors against the restatement
(lpips_ref.TOL: 8 times the measured fp32 error, figures in lpips_ref.py); evaluation.load_lpips_weights; refused arguments."""
import pytest
import torch
import torch.nn.functional as Fn

import lpips_ref as lr

KINDS = ("indep", "near", "same")
CASES = [(F, H, W, kind) for (H, W) in lr.SIZES for F in (1, 2) for kind in KINDS]


def _weights_obj(w):
    from dns_slam_amd import ops
    return ops.LpipsWeights(w["convs"], w["lins"])


def _torch64(pred, gt, w):
    """float64 composition of F.conv2d / F.max_pool2d, channels first"""
    shift = torch.tensor(lr.SHIFT, dtype=torch.float32).double().view(1, 3, 1, 1)
    scale = torch.tensor(lr.SCALE, dtype=torch.float32).double().view(1, 3, 1, 1)
    outs = []
    for img in (pred, gt):
        x = img.double().permute(0, 3, 1, 2).clamp(0, 1)
        x = (2.0 * x - 1.0 - shift) / scale
        feats = []
        for (wt, b), (_, _, _, stride, pad, pooled) in zip(w["convs"], lr.LAYERS):
            if pooled:
                x = Fn.max_pool2d(x, 3, 2)
            x = torch.relu(Fn.conv2d(x, wt.double(), b.double(), stride=stride, padding=pad))
            feats.append(x)
        outs.append(feats)
    ds = []
    for fa, fb, lin in zip(outs[0], outs[1], w["lins"]):
        na = fa / (torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10)
        ds.append((((na - nb) ** 2) * lin.double().view(1, -1, 1, 1)).sum(1).flatten(1).mean(1))
    layers = torch.stack(ds, 1)
    return layers.sum(1), layers, outs


@pytest.mark.parametrize("F,H,W,kind", CASES)
def test_restatement_agrees_with_float64_torch(F, H, W, kind):
    pred, gt, w, ref = lr.cached(lr.SEED, F, H, W, kind)
    val, layers, outs = _torch64(pred, gt, w)
    for l in range(5):
        a, b = ref["pred"][l]["feat"], outs[0][l].permute(0, 2, 3, 1)
        assert a.shape == b.shape
        assert (a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max()))
    print(f"lpips {ref['lpips'].tolist()}  |ref - torch64| {(ref['lpips'] - val).abs().max():.3g}")
    assert (ref["layers"] - layers).abs().max() <= 1e-12
    assert (ref["lpips"] - val).abs().max() <= 1e-12


@pytest.mark.parametrize("H,W", lr.SIZES)
def test_same_is_zero_and_swap_is_symmetric(H, W):
    pred, gt, w, ref = lr.cached(lr.SEED, 2, H, W, "same")
    assert (ref["lpips"] == 0).all() and (ref["layers"] == 0).all()
    pred, gt, w, ref = lr.cached(lr.SEED, 2, H, W, "indep")
    swapped = lr.lpips_ref(gt, pred, w)
    assert torch.equal(swapped["lpips"], ref["lpips"]) and torch.equal(swapped["layers"], ref["layers"])


def test_zero_lin_gives_zero():
    pred, gt, w, _ = lr.cached(lr.SEED, 1, 31, 31, "indep")
    w0 = {"convs": w["convs"], "lins": [torch.zeros_like(l) for l in w["lins"]]}
    assert (lr.lpips_ref(pred, gt, w0)["lpips"] == 0).all()
    from dns_slam_amd import ops
    assert (ops.lpips(pred, gt, _weights_obj(w0), method="torch")["lpips"] == 0).all()


def test_relu_outputs_are_not_mostly_zero():
    """The GPU test's element-wise bound would be vacuous on outputs the ReLU zeroes: at least a quarter of every feature of the
    shared inputs is non-zero."""
    for (H, W) in lr.SIZES:
        for kind in ("indep", "near"):
            _, _, _, ref = lr.cached(lr.SEED, 2, H, W, kind)
            for side in ("pred", "gt"):
                for l in range(5):
                    frac = float((ref[side][l]["feat"] > 0).double().mean())
                    assert frac >= 0.25, (H, W, kind, side, l, frac)


def test_constant_image_scaling_and_zero_pad_after_scaling():
    """Step 1 on a constant image, by hand; and conv1's zero padding is zero in the SCALED space: on a constant image the corner
    output misses exactly the taps with ky < 2 or kx < 2 (pad 2), each worth w s_c -- not w (s_c - scaled(0)_c)."""
    w = lr.random_weights(3)
    v = torch.tensor([0.25, 0.5, 0.9])
    img = v.view(1, 1, 1, 3).expand(1, 47, 47, 3).contiguous()
    s = lr.scale_image(img)
    shift = torch.tensor(lr.SHIFT, dtype=torch.float32).double()
    scale = torch.tensor(lr.SCALE, dtype=torch.float32).double()
    want = (2.0 * v.double() - 1.0 - shift) / scale
    assert (s - want).abs().max() == 0
    # out-of-range values clamp: 1.5 -> 1, -0.5 -> 0
    cl = lr.scale_image(torch.tensor([[[[1.5, -0.5, 0.5]]]]))
    assert (cl.view(3) - (torch.tensor([1.0, -1.0, 0.0]).double() - shift) / scale).abs().max() == 0
    pre = lr.tower(img, w)[0]["pre"]                        # [1,10,10,64]
    wt = w["convs"][0][0].double()                          # [64,3,11,11]
    missing = torch.ones(11, 11, dtype=torch.bool)
    missing[2:, 2:] = False
    delta = (wt * want.view(1, 3, 1, 1))[:, :, missing].sum((1, 2))
    assert (pre[0, 3, 3] - pre[0, 0, 0] - delta).abs().max() <= 1e-12
    # the fp32 torch composition agrees (to fp32 rounding of a 363-term sum)
    from dns_slam_amd import ops
    x = torch.cat((img, img)).permute(0, 3, 1, 2)
    x = (2.0 * x - 1.0 - torch.tensor(lr.SHIFT).view(1, 3, 1, 1)) / torch.tensor(lr.SCALE).view(1, 3, 1, 1)
    y = Fn.conv2d(x, w["convs"][0][0], w["convs"][0][1], stride=4, padding=2)
    assert ((y[0, :, 3, 3] - y[0, :, 0, 0]).double() - delta).abs().max() <= 365 * lr.U * float((wt.abs() * want.abs().view(1, 3, 1, 1)).sum((1, 2, 3)).max())


@pytest.mark.parametrize("F,H,W,kind", CASES)
def test_torch_method_on_cpu_agrees_with_restatement(F, H, W, kind):
    from dns_slam_amd import evaluation, ops
    pred, gt, w, ref = lr.cached(lr.SEED, F, H, W, kind)
    wo = _weights_obj(w)
    out = ops.lpips(pred, gt, wo, method="torch")
    assert out["lpips"].dtype == torch.float64 and tuple(out["lpips"].shape) == (F,) and tuple(out["layers"].shape) == (F, 5)
    assert torch.equal(evaluation.lpips(pred, gt, wo, method="torch"), out["lpips"])
    assert torch.equal(ops.lpips(pred, gt, wo)["lpips"], out["lpips"])           # CPU tensors: None means "torch"
    if kind == "same":
        assert (out["lpips"] == 0).all() and (out["layers"] == 0).all()
        return
    e_tot = float(((out["lpips"] - ref["lpips"]).abs() / ref["lpips"]).max())
    e_lay = float(((out["layers"] - ref["layers"]).abs() / ref["layers"]).max())
    print(f"{H}x{W} F={F} {kind}: relative error lpips {e_tot:.3g}, layers {e_lay:.3g} (allowed {lr.TOL[kind]})")
    assert e_tot <= lr.TOL[kind][0] and e_lay <= lr.TOL[kind][1]
    single = ops.lpips(pred[0], gt[0], wo, method="torch")
    assert single["lpips"].dim() == 0 and tuple(single["layers"].shape) == (5,)


def test_load_lpips_weights_round_trip(tmp_path):
    from dns_slam_amd import evaluation
    w = lr.random_weights(5)
    alex, lin = lr.state_dicts(w)
    alex["classifier.1.weight"] = torch.zeros(4, 4)                               # other keys are ignored
    pa, pl = tmp_path / "alexnet.pth", tmp_path / "alex.pth"
    torch.save(alex, pa), torch.save(lin, pl)
    wo = evaluation.load_lpips_weights(str(pa), str(pl))
    for (a, b), (c, d) in zip(wo.convs, w["convs"]):
        assert torch.equal(a, c) and torch.equal(b, d)
    for a, b in zip(wo.lins, w["lins"]):
        assert torch.equal(a, b)
    pred, gt, _, _ = lr.cached(lr.SEED, 1, 31, 31, "indep")
    assert torch.equal(evaluation.lpips(pred, gt, wo, method="torch"), evaluation.lpips(pred, gt, _weights_obj(w), method="torch"))


@pytest.mark.parametrize("which,key,edit", [
    ("alex", "features.6.bias", "missing"), ("lin", "lin3.model.1.weight", "missing"),
    ("alex", "features.3.weight", "shape"), ("lin", "lin0.model.1.weight", "shape"),
    ("alex", "features.10.weight", "type"), ("lin", "lin4.model.1.weight", "type")])
def test_load_lpips_weights_names_the_offending_key(tmp_path, which, key, edit):
    from dns_slam_amd import evaluation
    alex, lin = lr.state_dicts(lr.random_weights(5))
    sd = alex if which == "alex" else lin
    if edit == "missing":
        del sd[key]
    elif edit == "shape":
        sd[key] = sd[key][..., :-1].contiguous() if which == "alex" else sd[key].reshape(-1)
    else:
        sd[key] = [1.0, 2.0]
    pa, pl = tmp_path / "alexnet.pth", tmp_path / "alex.pth"
    torch.save(alex, pa), torch.save(lin, pl)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        evaluation.load_lpips_weights(str(pa), str(pl))


def test_refused_arguments():
    from dns_slam_amd import ops
    wo = _weights_obj(lr.random_weights(0))
    ok = torch.rand(1, 31, 31, 3)
    for method in ("torch", "fused", None):
        with pytest.raises(ValueError):
            ops.lpips(torch.rand(1, 30, 40, 3), torch.rand(1, 30, 40, 3), wo, method=method)      # a side below 31
        with pytest.raises(ValueError):
            ops.lpips(torch.rand(1, 40, 30, 3), torch.rand(1, 40, 30, 3), wo, method=method)
        with pytest.raises(ValueError):
            ops.lpips(ok, torch.rand(1, 31, 32, 3), wo, method=method)                            # mismatched shapes
        with pytest.raises(ValueError):
            ops.lpips(torch.rand(1, 31, 31, 4), torch.rand(1, 31, 31, 4), wo, method=method)      # last dimension not 3
    with pytest.raises(ValueError):
        ops.lpips(ok, ok, wo, method="fused")                                                     # CPU tensors: no fused path
    with pytest.raises(ValueError):
        ops.lpips(ok, ok, wo, method="eager")
    with pytest.raises(ValueError):
        ops.lpips(ok, ok, {"convs": [], "lins": []}, method="torch")
    with pytest.raises(ValueError):
        ops.conv_cl(torch.rand(1, 8, 8, 64), torch.rand(64, 64, 3, 3), None, 1, 1)                # CPU tensors
    with pytest.raises(ValueError):
        ops.max_pool_cl(torch.rand(1, 8, 8, 64))
    with pytest.raises(ValueError):
        ops.lpips_head(torch.rand(1, 4, 4, 64), torch.rand(1, 4, 4, 64), torch.rand(64))
    with pytest.raises(ValueError):
        ops.LpipsWeights(lr.random_weights(0)["convs"][:4], lr.random_weights(0)["lins"])
