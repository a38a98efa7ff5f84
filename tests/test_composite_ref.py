"""tests/composite_ref.py on the CPU: the hand-written float64 gradients against autograd through oracle/render_math.raw2nerf_color,
and the project's own fp32 oracle against the bound the GPU kernels are held to (tests/test_gpu_composite.py) -- the reference and
its bound must leave room for a correct fp32 implementation in every regime before a kernel is judged by them."""
import pytest
import torch

import composite_ref as cref
from oracle import render_math as rm


def _oracle(raw, z, logits, grads, dtype):
    """rm.raw2nerf_color + the logit composite + autograd in `dtype` -> dict over cref.OUT_KEYS."""
    r = raw.to(dtype).clone().requires_grad_(True)
    lg = logits.to(dtype).clone().requires_grad_(True) if logits is not None else None
    d, v, c, w = rm.raw2nerf_color(r, z.to(dtype))
    loss = (d * grads["depth"].to(dtype)).sum() + (v * grads["var"].to(dtype)).sum() + (c * grads["rgb"].to(dtype)).sum() \
        + (w * grads["weights"].to(dtype)).sum()
    sem = None
    if lg is not None:
        sem = torch.sum(w[..., None] * lg, -2)
        loss = loss + (sem * grads["sem"].to(dtype)).sum()
    loss.backward()
    return {"depth": d.detach(), "var": v.detach(), "rgb": c.detach(), "weights": w.detach(),
            "sem": sem.detach() if sem is not None else torch.zeros(raw.shape[0], 0, dtype=dtype),
            "d_raw": r.grad, "d_logits": lg.grad if lg is not None else torch.zeros(*raw.shape[:2], 0, dtype=dtype)}


@pytest.mark.parametrize("S", [1, 47, 200])
def test_float64_gradients_equal_autograd_on_mild_inputs(S):
    cs = cref.case("mild", 9, S, 5)
    ref, _ = cref.composite64(cs["raw"], cs["z"], cs["logits"], cs["grads"], pure=True)
    want = _oracle(cs["raw"], cs["z"], cs["logits"], cs["grads"], torch.float64)
    for k in cref.OUT_KEYS:
        scale = float(want[k].abs().max()) if want[k].numel() else 0.0
        assert float((ref[k] - want[k]).abs().max()) <= 1e-12 * scale, k


def test_rgb_logits_variant_is_the_plain_one_on_sigmoid_colours():
    cs = cref.case("surface", 5, 65, 3, rgb_logits=True)
    a, _ = cref.composite64(cs["raw"], cs["z"], cs["logits"], cs["grads"], rgb_logits=True)
    raw2 = cs["raw"].double().clone()
    raw2[..., :3] = torch.sigmoid(raw2[..., :3])
    b, _ = cref.composite64(raw2, cs["z"], cs["logits"], cs["grads"])
    col = raw2[..., :3]
    for k in ("depth", "var", "rgb", "weights", "sem", "d_logits"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["d_raw"][..., 3], b["d_raw"][..., 3])
    assert torch.allclose(a["d_raw"][..., :3], b["d_raw"][..., :3] * col * (1 - col), rtol=1e-14, atol=0)


@pytest.mark.parametrize("regime", cref.REGIMES)
def test_fp32_oracle_stays_inside_the_bound(regime):
    """rm.raw2nerf_color in fp32 with autograd -- a correct fp32 implementation with its own sigmoid, product order and gradient
    formulas -- against the float64 reference and the bound of composite_ref.bound, in every regime at every S the GPU test uses.
    Also printed (not asserted): the ratio against the PURE float64 function without the spread term; where that is large the
    operation itself is ill-conditioned in alpha (var on `edge` rays), which is what the spread term is for."""
    worst, worst_pure = {}, {}
    for S in cref.S_EDGES:
        cs = cref.case(regime, 33, S, 5)
        got = _oracle(cs["raw"], cs["z"], cs["logits"], cs["grads"], torch.float32)
        ref, spread = cref.reference(regime, 33, S, 5)
        pure, zero = cref.composite64(cs["raw"], cs["z"], cs["logits"], cs["grads"], pure=True)
        for k in cref.OUT_KEYS:
            assert bool(torch.isfinite(ref[k]).all()), (regime, S, k)
            worst[k] = max(worst.get(k, 0.0), cref.worst_ratio(k, got[k], ref, spread))
            worst_pure[k] = max(worst_pure.get(k, 0.0), cref.worst_ratio(k, got[k], pure, zero))
    print(f"{regime}: fp32 oracle / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    print(f"{regime}: fp32 oracle / (bound without spread, pure float64 alpha) " + ", ".join(f"{k} {v:.3g}" for k, v in worst_pure.items()))
    assert max(worst.values()) <= 1.0, worst


def test_non_finite_rays_are_nan_where_the_arithmetic_says():
    cs = cref.case("mild", 4, 47, 5)
    raw = cs["raw"].clone()
    raw[1, :, 3] = -20.0                                   # every alpha rounds to 0 in fp32: 0 / 0
    ref, _ = cref.composite64(raw, cs["z"], cs["logits"], cs["grads"])
    for k in cref.OUT_KEYS:
        assert bool(torch.isnan(ref[k][1]).all()), k
        assert bool(torch.isfinite(ref[k][[0, 2, 3]]).all()), k
    raw = cs["raw"].clone()
    raw[2, 5, 3], raw[2, 9, 3] = float("inf"), float("-inf")
    ref, _ = cref.composite64(raw, cs["z"], cs["logits"], cs["grads"])
    for k in cref.OUT_KEYS:
        assert bool(torch.isfinite(ref[k]).all()), k
    assert float(ref["weights"][2, 9]) == 0.0 and bool((ref["weights"][2, 6:] < 1e-9).all())
    assert float(ref["d_raw"][2, 5, 3]) == 0.0 and float(ref["d_raw"][2, 9, 3]) == 0.0
