"""The compositing kernels (csrc/composite.hip, dev_composite.hpp: ray_forward is shared with the fused tracker) against the float64
reference of tests/composite_ref.py in the occupancy regimes of a trained scene -- alpha exactly 1 at surfaces, transmittance
stepping through 1e-10, 1e-20, ... into underflow, nearly empty rays --, at the sample counts around the 1 / 2 / 4
samples-per-lane switches, with more classes than lanes, and through all three entry routes.  Bound and regimes: composite_ref.
Beyond the bound, the invariants its spread term could swallow: weights >= 0 summing to 1, var >= 0, depth inside the ray's z range,
everything finite where the reference is."""
import pytest
import torch

import composite_ref as cref
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_LOGITS = 1            # include/dns_hip.h DNS_COMPOSITE_RGB_LOGITS


def _ops():
    from dns_slam_amd import ops
    return ops


def _autograd(cs):
    """ops.composite with all five output gradients in one backward."""
    ops = _ops()
    raw = cs["raw"].to(DEV).requires_grad_(True)
    lg = cs["logits"].to(DEV).requires_grad_(True) if cs["logits"] is not None else None
    depth, var, rgb, w, sem = ops.composite(raw, cs["z"].to(DEV), lg)
    g = cs["grads"]
    outs, gs = [depth, var, rgb, w], [g["depth"], g["var"], g["rgb"], g["weights"]]
    if lg is not None:
        outs.append(sem)
        gs.append(g["sem"])
    torch.autograd.backward(outs, [t.to(DEV) for t in gs])
    N, S = cs["z"].shape
    return {"depth": depth, "var": var, "rgb": rgb, "weights": w, "sem": sem, "d_raw": raw.grad,
            "d_logits": lg.grad if lg is not None else torch.zeros(N, S, 0)}


def _raw_entry(cs, only=None, want_d_logits=True, flags=None):
    """dns_composite_fwd / _bwd (flags None) or the _ex pair, straight through the C ABI; only: the output gradients handed over
    (the others are NULL pointers); want_d_logits False: d_logits is NULL."""
    ops = _ops()
    raw, z = cs["raw"].to(DEV), cs["z"].to(DEV)
    lg = cs["logits"].to(DEV) if cs["logits"] is not None else None
    N, S = z.shape
    Cn = lg.shape[-1] if lg is not None else 0
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    depth, var, rgb, w, sem = new(N), new(N), new(N, 3), new(N, S), (new(N, Cn) if Cn else None)
    d_raw, d_lg = new(N, S, 4), (new(N, S, Cn) if (Cn and want_d_logits) else None)
    gd = {k: (v.to(DEV).contiguous() if (v is not None and (only is None or k in only)) else None) for k, v in cs["grads"].items()}
    p, st = ops.ptr, ops.stream_ptr()
    fwd = (p(raw), p(z), p(lg), N, S, Cn, p(depth), p(var), p(rgb), p(w), p(sem))
    bwd = (p(raw), p(z), p(lg), N, S, Cn, p(gd["depth"]), p(gd["var"]), p(gd["rgb"]), p(gd["weights"]), p(gd["sem"]), p(d_raw), p(d_lg))
    if flags is None:
        ops.check(ops.lib.dns_composite_fwd(*fwd, st), "dns_composite_fwd")
        ops.check(ops.lib.dns_composite_bwd(*bwd, st), "dns_composite_bwd")
    else:
        ops.check(ops.lib.dns_composite_fwd_ex(*fwd, flags, st), "dns_composite_fwd_ex")
        ops.check(ops.lib.dns_composite_bwd_ex(*bwd, flags, st), "dns_composite_bwd_ex")
    torch.cuda.synchronize()
    out = {"depth": depth, "var": var, "rgb": rgb, "weights": w, "sem": sem if Cn else torch.zeros(N, 0), "d_raw": d_raw}
    if d_lg is not None or not Cn:
        out["d_logits"] = d_lg if Cn else torch.zeros(N, S, 0)
    return out


def _check(got, ref, spread, z, what):
    bad = {}
    for k in cref.OUT_KEYS:
        if k not in got:
            continue
        r = cref.worst_ratio(k, got[k], ref, spread)
        scale = float(ref[k][torch.isfinite(ref[k])].abs().max()) if bool(torch.isfinite(ref[k]).any()) else 0.0
        fin = torch.isfinite(ref[k])
        e = float((got[k].detach().double().cpu().reshape(ref[k].shape) - ref[k])[fin].abs().max()) / scale if scale > 0 else 0.0
        REPORT.append((f"composite64 {what} {k}", e, r, 1e-5))
        print(f"composite64 {what} {k}: worst ratio {r:.3g}")
        if not r <= 1.0:
            bad[k] = r
    assert not bad, f"{what}: outside 1e-5 |ref| + 1e-6 scale + 4 spread (or a NaN / Inf out of place): {bad}"
    # invariants, on the rays whose reference is finite
    ok = torch.isfinite(ref["weights"]).all(-1)
    w = got["weights"].detach().double().cpu()[ok]
    zz = z.double()[ok]
    assert bool((w >= 0).all()), f"{what}: negative weight"
    assert w.numel() == 0 or float((w.sum(-1) - 1).abs().max()) <= 1e-6, f"{what}: weights sum {w.sum(-1)}"
    assert bool((got["var"].detach().cpu()[ok] >= 0).all()), f"{what}: negative variance"
    # a convex combination of z whose fp32 weights sum to 1 within 1e-6 (just asserted) leaves [z_min, z_max] by at most that
    # fraction of z_max; a one-sample ray (w = u / u = 1) gives z itself
    d = got["depth"].detach().double().cpu()[ok]
    slack = 1e-6 * zz[:, -1] if zz.shape[1] > 1 else torch.zeros_like(d)
    assert bool((d >= zz[:, 0] - slack).all() and (d <= zz[:, -1] + slack).all()), f"{what}: depth outside the ray's z range"


@pytest.mark.parametrize("S", cref.S_EDGES)
@pytest.mark.parametrize("regime", cref.REGIMES)
def test_composite_regimes_through_autograd(regime, S):
    cs = cref.case(regime, 33, S, 5)
    ref, spread = cref.reference(regime, 33, S, 5)
    _check(_autograd(cs), ref, spread, cs["z"], f"{regime} S={S}")


@pytest.mark.parametrize("C_", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("regime", ["mild", "surface"])
def test_composite_class_counts_around_the_wave(regime, C_):
    """lanes-over-classes loops: no class, fewer than, exactly and more than 64 (second and third trips)."""
    cs = cref.case(regime, 33, 65, C_)
    ref, spread = cref.reference(regime, 33, 65, C_)
    _check(_autograd(cs), ref, spread, cs["z"], f"{regime} C={C_}")


@pytest.mark.parametrize("N", [1, 3, 4, 5])
@pytest.mark.parametrize("regime", ["mild", "surface"])
def test_composite_ray_counts_around_the_workgroup(regime, N):
    """four rays per workgroup: a partly filled one, exactly one, one and a quarter."""
    cs = cref.case(regime, N, 47, 5)
    ref, spread = cref.reference(regime, N, 47, 5)
    _check(_autograd(cs), ref, spread, cs["z"], f"{regime} N={N}")


@pytest.mark.parametrize("only,want_d_logits", [(("depth",), True), (("weights",), True), (("sem",), True), (None, False)])
@pytest.mark.parametrize("regime", cref.REGIMES)
def test_composite_entry_points_with_null_gradients(regime, only, want_d_logits):
    """dns_composite_fwd / _bwd with one output gradient at a time (the others NULL), and with every gradient but no d_logits."""
    cs = cref.case(regime, 33, 65, 5)
    ref, spread = cref.reference(regime, 33, 65, 5, only=only)
    got = _raw_entry(cs, only, want_d_logits)
    assert ("d_logits" in got) == want_d_logits
    _check(got, ref, spread, cs["z"], f"{regime} raw entry only={only} d_logits={want_d_logits}")


@pytest.mark.parametrize("S", [1, 64, 65, 256])
@pytest.mark.parametrize("regime", cref.REGIMES)
def test_composite_rgb_logits_variant(regime, S):
    """dns_composite_fwd_ex / _bwd_ex with DNS_COMPOSITE_RGB_LOGITS: the colour sigmoid inside the kernels, forward and backward."""
    cs = cref.case(regime, 33, S, 5, rgb_logits=True)
    ref, spread = cref.reference(regime, 33, S, 5, rgb_logits=True)
    _check(_raw_entry(cs, flags=RGB_LOGITS), ref, spread, cs["z"], f"{regime} S={S} rgb logits")


def _poisoned(kind, cs):
    raw = cs["raw"].clone()
    if kind == "dead":
        raw[1, :, 3] = -20.0                               # every alpha is 0: w = 0 / 0 (D9)
        return raw, 1
    if kind == "inf":
        raw[2, 5, 3], raw[2, 9, 3] = float("inf"), float("-inf")
        return raw, 2
    raw[0, 7, 1] = float("nan")                            # one colour channel of one sample
    return raw, 0


@pytest.mark.parametrize("S", [47, 129])
@pytest.mark.parametrize("kind", ["dead", "inf", "nan_colour"])
def test_composite_non_finite_rays_stay_in_their_wave(kind, S):
    """NaN exactly where the reference has it, and the other three rays of the workgroup bit-identical to a run without the
    poisoned ray."""
    cs = cref.case("mild", 4, S, 5)
    raw, ray = _poisoned(kind, cs)
    bad = dict(cs, raw=raw)
    ref, spread = cref.composite64(raw, cs["z"], cs["logits"], cs["grads"])
    if kind == "dead":
        assert bool(torch.isnan(ref["depth"][ray])) and bool(torch.isnan(ref["d_raw"][ray]).all())
    if kind == "nan_colour":
        assert bool(torch.isnan(ref["rgb"][ray, 1])) and bool(torch.isfinite(ref["rgb"][ray, [0, 2]]).all())
        assert bool(torch.isnan(ref["d_raw"][ray, :, 3]).all())
    got = _autograd(bad)
    _check(got, ref, spread, cs["z"], f"{kind} S={S}")
    clean = _autograd(cs)
    others = [r for r in range(4) if r != ray]
    for k in cref.OUT_KEYS:
        assert torch.equal(got[k].detach().cpu()[others], clean[k].detach().cpu()[others]), f"{kind}: {k} of a neighbouring ray changed"
        assert bool(torch.isfinite(got[k].detach().cpu()[others]).all()), k
