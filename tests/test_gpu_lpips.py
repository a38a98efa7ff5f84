"""GPU: LPIPS as the project's own kernels (csrc/lpips.hip: ops.conv_cl, ops.max_pool_cl, ops.lpips_head, ops.lpips,
evaluation.render_metrics(lpips=...)) against the float64 restatement tests/lpips_ref.py.

Bounds.  u = 2^-24.
* ops.conv_cl, element-wise and with no element exempt: |y - y64| <= 1.01 (K + 2) u (A + |b|), A = conv(|x|, |w|), K = k k Cin: the
  worst case of a K-term fp32 sum in any order, plus the bias add; ReLU is 1-Lipschitz.  The float64 reference is evaluated on the
  fp32 inputs the kernel is handed.  With ``scale_input`` the scaling rounds twice (the clamp and 2x - 1 are exact; the
  subtraction of the shift and the division round once each), which moves an input by at most 2 u relative: (K + 4) in place of
  (K + 2).
* ops.lpips(method="fused") against the restatement, lpips and every layers entry, relative: lpips_ref.TOL = 8 times the error
  MEASURED on the CPU for the fp32 composition of F.conv2d / F.max_pool2d on the same inputs, the largest over the cases below:
      indep: lpips 1.5e-7 -> 1.2e-6, layers 1.35e-6 -> 1.08e-5;      near: lpips 2.67e-6 -> 2.14e-5, layers 6.4e-6 -> 5.12e-5.
  Another summation order moves the error, and nothing else should.  `same` pairs give exactly 0.0.
* ops.lpips_head in float64 against float64: 1e-12 relative.
Sizes: 31 x 31 makes every layer minimal and the last three 1 x 1; 67 x 95 and 131 x 70 are no multiples of any tile and span
several conv1 tiles (8 x 32 output pixels per workgroup)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import lpips_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = lr.U
_W = {}


def _weights(w):
    from dns_slam_amd import ops
    if id(w) not in _W:
        _W[id(w)] = ops.LpipsWeights(w["convs"], w["lins"])
    return _W[id(w)]


def _check_conv(y, pre, A, bias, K, relu, what, extra=2):
    want = lr.relu64(pre) if relu else pre
    bound = 1.01 * (K + extra) * U * (A + bias.double().abs())
    err = (y.double().cpu() - want).abs()
    ratio = float((err / bound).max())
    nz = float((want > 0).double().mean())
    print(f"{what} relu={relu}: worst error / bound {ratio:.3f}, non-zero outputs {nz:.2f}")
    assert y.shape == want.shape
    assert bool((err <= bound).all()), (what, relu, ratio)
    if relu:
        assert nz >= 0.25, (what, nz)


@pytest.mark.parametrize("layer", range(5))
@pytest.mark.parametrize("H,W", lr.SIZES)
def test_conv_cl_within_the_derived_bound(H, W, layer):
    from dns_slam_amd import ops
    _, _, w, ref = lr.cached(lr.SEED, 2, H, W, "indep")
    cin, cout, ks, stride, pad, _ = lr.LAYERS[layer]
    wt, b = w["convs"][layer]
    x32 = ref["pred"][layer]["x"].float()                      # the restatement's input of this layer, as the kernel is handed it
    assert tuple(x32.shape[1:]) == tuple(ref["pred"][layer]["x"].shape[1:]) and x32.shape[-1] == cin
    pre, A = lr.conv64(x32, wt, b, stride, pad)
    xd, wd, bd = x32.to(DEV), wt.to(DEV), b.to(DEV)
    for relu in (False, True):
        y = ops.conv_cl(xd, wd, bd, stride, pad, relu=relu)
        _check_conv(y, pre, A, b, ks * ks * cin, relu, f"conv{layer + 1} {H}x{W}")
    y1 = ops.conv_cl(xd[1:], wd, bd, stride, pad)              # an image's bits do not depend on its batch
    assert torch.equal(y1[0], y[1])
    if layer == 0:
        pred, _, _, _ = lr.cached(lr.SEED, 2, H, W, "near")      # leaves [0,1] here and there: the clamp is exercised
        pre, A = lr.conv64(lr.scale_image(pred), wt, b, stride, pad)
        for relu in (False, True):
            y = ops.conv_cl(pred.to(DEV), wd, bd, stride, pad, relu=relu, scale_input=True)
            _check_conv(y, pre, A, b, ks * ks * cin, relu, f"conv1 scaled {H}x{W}", extra=4)


def test_conv_cl_without_bias_and_nan():
    from dns_slam_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 9, 37, 64, generator=g)
    wt = torch.randn(128, 64, 3, 3, generator=g) * 0.05
    pre, A = lr.conv64(x, wt, None, 1, 1)
    y = ops.conv_cl(x.to(DEV), wt.to(DEV), None, 1, 1, relu=False)
    assert bool(((y.double().cpu() - pre).abs() <= 1.01 * (576 + 2) * U * A).all())
    x[0, 4, 20, 7] = float("nan")
    y = ops.conv_cl(x.to(DEV), wt.to(DEV), None, 1, 1, relu=True).cpu()
    nan = torch.isnan(y)
    assert bool(nan[0, 3:6, 19:22].all()) and int(nan.sum()) == 9 * 128       # the ReLU keeps it; nothing else is touched


@pytest.mark.parametrize("shape", [(2, 7, 7, 64), (1, 16, 23, 192), (3, 5, 3, 4), (1, 32, 17, 256)])
def test_max_pool_equals_torch(shape):
    from dns_slam_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g)
    x[0, 2, 1, 1] = float("nan")
    x[-1, 4, 2, 0] = float("-inf")
    want = Fn.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    got = ops.max_pool_cl(x.to(DEV)).cpu()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(want).sum()) >= 1
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("F,h,w,C", [(1, 1, 1, 64), (2, 7, 7, 64), (2, 16, 23, 192), (1, 13, 11, 384), (3, 3, 43, 256)])
def test_lpips_head_against_float64(F, h, w, C):
    from dns_slam_amd import ops
    g = torch.Generator().manual_seed(5)
    fa, fb = torch.relu(torch.randn(F, h, w, C, generator=g)), torch.relu(torch.randn(F, h, w, C, generator=g))
    fa[0, 0, 0] = 0.0                                          # all-zero pixels: 0 / 1e-10 = 0, on one side and on both
    fa[-1, -1, -1] = 0.0
    fb[-1, -1, -1] = 0.0
    lin = torch.rand(C, generator=g) * 0.1
    want = lr.head64(fa, fb, lin)
    got = ops.lpips_head(fa.to(DEV), fb.to(DEV), lin.to(DEV)).cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (F,)
    assert bool(((got - want).abs() <= 1e-12 * want.abs()).all()), (got, want)
    assert bool((ops.lpips_head(fa.to(DEV), fa.to(DEV), lin.to(DEV)) == 0).all())


CASES = [(F, H, W, kind) for (H, W) in lr.SIZES for F in (1, 2) for kind in ("indep", "near", "same")]


@pytest.mark.parametrize("F,H,W,kind", CASES)
def test_lpips_fused_against_restatement_and_torch(F, H, W, kind):
    from dns_slam_amd import evaluation, ops
    pred, gt, w, ref = lr.cached(lr.SEED, F, H, W, kind)
    wo = _weights(w)
    pd, gd = pred.to(DEV), gt.to(DEV)
    out = ops.lpips(pd, gd, wo, method="fused")
    assert out["lpips"].dtype == torch.float64 and tuple(out["lpips"].shape) == (F,) and tuple(out["layers"].shape) == (F, 5)
    assert out["lpips"].is_cuda
    val, layers = out["lpips"].cpu(), out["layers"].cpu()
    assert torch.equal(ops.lpips(pd, gd, wo)["lpips"].cpu(), val) or ops.LPIPS_DEFAULT != "fused"
    assert torch.equal(evaluation.lpips(pd, gd, wo, method="fused").cpu(), val)
    again = ops.lpips(pd, gd, wo, method="fused")
    assert torch.equal(again["lpips"].cpu(), val) and torch.equal(again["layers"].cpu(), layers)      # two calls: the same bits
    th = ops.lpips(pd, gd, wo, method="torch")
    tval, tlayers = th["lpips"].cpu(), th["layers"].cpu()
    if kind == "same":
        assert bool((val == 0).all()) and bool((layers == 0).all())
        print(f"{H}x{W} F={F} same: torch composition {tval.tolist()} (the library's convolutions do not give an image the same bits "
              f"at every batch position and in every call: measured 3e-18 .. 5e-16 here)")
        return
    e_tot = float(((val - ref["lpips"]).abs() / ref["lpips"]).max())
    e_lay = float(((layers - ref["layers"]).abs() / ref["layers"]).max())
    t_tot = float(((tval - ref["lpips"]).abs() / ref["lpips"]).max())
    t_lay = float(((tlayers - ref["layers"]).abs() / ref["layers"]).max())
    d_tot = float(((val - tval).abs() / ref["lpips"]).max())
    d_lay = float(((layers - tlayers).abs() / ref["layers"]).max())
    tol = lr.TOL[kind]
    print(f"{H}x{W} F={F} {kind}: relative error fused lpips {e_tot:.3g} layers {e_lay:.3g}; torch lpips {t_tot:.3g} layers {t_lay:.3g}; "
          f"fused - torch lpips {d_tot:.3g} layers {d_lay:.3g}; allowed {tol[0]:.3g}, {tol[1]:.3g}")
    assert e_tot <= tol[0] and e_lay <= tol[1]
    assert d_tot <= tol[0] and d_lay <= tol[1]
    single = ops.lpips(pd[0], gd[0], wo, method="fused")
    assert single["lpips"].dim() == 0 and tuple(single["layers"].shape) == (5,)
    # a pair evaluated alone has the bits it has inside the batch
    assert torch.equal(single["lpips"].cpu(), val[0]) and torch.equal(single["layers"].cpu(), layers[0])
    if F == 2:
        last = ops.lpips(pd[1:], gd[1:], wo, method="fused")
        assert torch.equal(last["lpips"].cpu(), val[1:]) and torch.equal(last["layers"].cpu(), layers[1:])


@pytest.mark.parametrize("H,W", lr.SIZES)
def test_nan_pixel_stays_in_its_pair(H, W):
    from dns_slam_amd import ops
    pred, gt, w, _ = lr.cached(lr.SEED, 2, H, W, "indep")
    wo = _weights(w)
    clean = ops.lpips(pred.to(DEV), gt.to(DEV), wo, method="fused")
    bad = pred.clone()
    bad[0, H // 2, W // 3, 1] = float("nan")
    out = ops.lpips(bad.to(DEV), gt.to(DEV), wo, method="fused")
    assert bool(torch.isnan(out["lpips"][0])) and bool(torch.isnan(out["layers"][0, 0]))
    assert torch.equal(out["lpips"][1], clean["lpips"][1]) and torch.equal(out["layers"][1], clean["layers"][1])
    th = ops.lpips(bad.to(DEV), gt.to(DEV), wo, method="torch")
    assert bool(torch.isnan(th["lpips"][0])) and not bool(torch.isnan(th["lpips"][1]))


def test_refused_before_any_launch():
    from dns_slam_amd import ops
    _, _, w, _ = lr.cached(lr.SEED, 1, 31, 31, "indep")
    wo = _weights(w)
    ok = torch.rand(1, 31, 31, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.lpips(ok.cpu(), ok.cpu(), wo, method="fused")
    with pytest.raises(ValueError):
        ops.lpips(ok, ok.cpu(), wo, method="fused")
    with pytest.raises(ValueError):
        ops.lpips(ok[:, :30], ok[:, :30], wo, method="fused")
    with pytest.raises(ValueError):
        ops.lpips(ok, torch.rand(1, 31, 32, 3, device=DEV), wo)
    with pytest.raises(ValueError):
        ops.lpips(torch.rand(1, 31, 31, 4, device=DEV), torch.rand(1, 31, 31, 4, device=DEV), wo)
    x = torch.rand(1, 8, 8, 64, device=DEV)
    with pytest.raises(ValueError):
        ops.conv_cl(x, torch.rand(100, 64, 3, 3, device=DEV), None, 1, 1)            # Cout no multiple of 64
    with pytest.raises(ValueError):
        ops.conv_cl(x, torch.rand(64, 32, 3, 3, device=DEV), None, 1, 1)             # Cin mismatch
    with pytest.raises(ValueError):
        ops.conv_cl(x, torch.rand(64, 64, 3, 3, device=DEV), None, 1, 3)             # pad >= kernel
    with pytest.raises(ValueError):
        ops.conv_cl(x.cpu(), torch.rand(64, 64, 3, 3, device=DEV), None, 1, 1)
    with pytest.raises(ValueError):
        ops.conv_cl(x, torch.rand(64, 64, 3, 3, device=DEV), None, 1, 1, scale_input=True)
    with pytest.raises(ValueError):
        ops.max_pool_cl(torch.rand(1, 2, 8, 64, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_head(x, x, torch.rand(32, device=DEV))


def _scene():
    """A 168 x 176 synthetic scene of 4 frames and a randomised decoder (MS-SSIM's five scales need 161 pixels a side)."""
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.mapping import Mapper
    from util import randomise_
    cam = synthetic.camera(H=168, W=176, fx=170.0, fy=170.0)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=3)
    cfg = synthetic.default_cfg(n_pixels=200, hash_size=14, voxel_size=0.08, smooth_pts=10)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    mapper = Mapper(cfg, dec, bound, cam, device=DEV)
    mapper.set_decoder(frames)
    randomise_(dec, 5)
    with torch.no_grad():
        dec.pe_fn.grid_fn.params.mul_(2000.0)
    randomise_([mapper.fine_decoders.pool], 6)
    return mapper, frames


def test_render_metrics_with_lpips():
    from dns_slam_amd import evaluation as E
    from dns_slam_amd import ops
    mapper, frames = _scene()
    _, _, w, _ = lr.cached(lr.SEED, 1, 31, 31, "indep")
    wo = _weights(w)
    idx = [0, 2]
    torch.manual_seed(1)
    jitters = [mapper.draw_jitter(1) for _ in idx]
    plain = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters)
    out = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters, lpips=wo, lpips_method="fused")
    assert "lpips" not in plain and set(out) == set(plain) | {"lpips"}
    for key in plain:
        if key == "frames":
            assert out[key] == plain[key]
        else:
            assert np.array_equal(out[key]["per_frame"], plain[key]["per_frame"]) and out[key]["mean"] == plain[key]["mean"], key
    assert out["lpips"]["per_frame"].shape == (2,) and out["lpips"]["per_frame"].dtype == np.float64
    assert out["lpips"]["mean"] == float(np.mean(out["lpips"]["per_frame"]))
    for k, i in enumerate(idx):
        col, _, _ = mapper.render_frame(frames["gt_color"][i], frames["gt_depth"][i], frames["gt_label"][i], frames["est_c2w"][i],
                                        n_pts_batch=8192, jitter=jitters[k])
        want = float(E.lpips(col, frames["gt_color"][i].to(DEV), wo, method="fused"))
        assert out["lpips"]["per_frame"][k] == want and want > 0.0
    dflt = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters, lpips=wo)       # method=None
    assert np.isfinite(dflt["lpips"]["per_frame"]).all() and np.array_equal(dflt["ssim"]["per_frame"], plain["ssim"]["per_frame"])
    print(f"render_metrics lpips: fused {out['lpips']['per_frame'].tolist()}, default ({ops.LPIPS_DEFAULT}) {dflt['lpips']['per_frame'].tolist()}")
    with pytest.raises(ValueError):
        E.render_metrics(mapper, frames, indices=idx, lpips={"convs": []})
