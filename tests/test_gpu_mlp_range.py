"""The split-operand and half-row MLP kernels (csrc/mlp_split.hpp, mlp_split_bwd.inc, mlp_half*.{hpp,hip,inc}) against the float64
reference of tests/mlp_ref.py across operand RANGE -- rows, columns, weight rows, weight sets and input segments many binades apart,
the +-110 exponent clamp, exact zeros -- and on non-finite inputs.  Every finite comparison is element-wise against the bound
mlp_ref derives from the stated operand formats (no tuned tolerance); the margin used is recorded in parity_report.json.
P = 101 points: three full 32-point tiles and a 5-point tail."""
import ctypes as C

import pytest
import torch

import mlp_ref as mr
from test_gpu_split_rows import _lib, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 5                                                   # tests/test_mlp_ref.py checks this seed's near-kink share on the CPU
N1 = mr.N1


def _ops():
    from dns_slam_amd import ops
    return ops


class _save_hidden:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.ops = _ops()
        self.old, self.ops.MLP_SAVE_HIDDEN = self.ops.MLP_SAVE_HIDDEN, self.on

    def __exit__(self, *a):
        self.ops.MLP_SAVE_HIDDEN = self.old


def _absmax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _autograd(fn, inputs, params, dy):
    """y, [d input...], d params of fn(*inputs, params) on the GPU"""
    ins = [t.to(DEV).requires_grad_(True) for t in inputs]
    p = params.to(DEV).requires_grad_(True)
    y = fn(*ins, p)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), [t.grad.cpu() for t in ins], p.grad.cpu()


def _prepare(what, x, params, dy, shape, mode, name=None, **kw):
    """The reference, the near-kink flags and the dy both sides use.  Where the format allows it (mlp_ref.kinks_zeroed) the
    flagged points' dy rows are zeroed and their share is held to 2 %; elsewhere every point keeps its dy and the bound carries
    the undetermined-unit term, so no point leaves the comparison.  The share goes on record either way."""
    import util
    ref = mr.analyse(x, params, dy, shape, mode, **kw)
    zero = mr.kinks_zeroed(mode, name)
    dy, kinks = mr.mask_kinks(dy, ref["pre"], ref["e_pre"], zero)
    share = int(kinks.sum()) / x.shape[0]
    print(f"{what} near-kink points: {int(kinks.sum())} of {x.shape[0]}{'' if zero else ' (dy kept)'}")
    util.REPORT.append((f"{what} near-kink share{'' if zero else ' (dy kept, not limited)'}", share, share / 0.02 if zero else float("nan"), 0.02))
    if zero:
        assert share <= 0.02, f"{what}: {int(kinks.sum())} near-kink points"
        return mr.analyse(x, params, dy, shape, mode, **kw), kinks, dy
    return ref, torch.zeros_like(kinks), dy


def _check_params(what, dp, ref, shape):
    used = mr.used_count(shape)
    dp = dp.reshape(-1, dp.shape[-1])
    want, bound = ref["dparams"].reshape(dp.shape[0], -1), ref["e_dparams"].reshape(dp.shape[0], -1)
    mr.assert_within(f"{what} dparams", dp[:, :used], want, bound)
    assert _absmax(dp[:, used:]) == 0.0, f"{what}: the zero-padded rows of W_out received a gradient"


def _check(what, y, dx, dp, ref, kinks, shape):
    mr.assert_within(f"{what} y", y, ref["y"], ref["e_y"])
    assert bool(torch.isfinite(y).all())
    mr.assert_within(f"{what} dx", dx, ref["dx"], ref["e_dx"])
    assert _absmax(dx[kinks]) == 0.0, f"{what}: dx of a point whose dy is zero"
    _check_params(what, dp, ref, shape)


VARIANTS = [("exact", False), ("exact", True), ("fp16", False)]      # (mode, MLP_SAVE_HIDDEN)


@pytest.mark.parametrize("shape", mr.NETS)
@pytest.mark.parametrize("name", mr.FINITE)
def test_mlp_range(name, shape):
    """ops.mlp, exact and fp16, with and without kept hidden activations."""
    ops = _ops()
    x, params, dy0 = mr.finite_case(name, shape, SEED)
    for mode, save in VARIANTS:
        what = f"mlp {name} {shape} {mode}{' kept h' if save else ''}:"
        ref, kinks, dy = _prepare(what, x, params, dy0, shape, mode, name)
        with _save_hidden(save):
            y, (dx,), dp = _autograd(lambda a, p: ops.mlp(a, p, *shape, fp16=mode == "fp16"), [x], params, dy)
        _check(what, y, dx, dp, ref, kinks, shape)


@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_grouped_range(shape):
    """a pool whose sets need exponents 20 binades apart; a single-point set and a point without a set give zeros"""
    ops = _ops()
    x, pool, dy0, slot = mr.group_case(shape, SEED)
    for mode, save in VARIANTS:
        ref, kinks, dy = _prepare(f"mlp_grouped {shape} {mode}:", x, pool, dy0, shape, mode, group=slot)
        with _save_hidden(save):
            y, (dx,), dp = _autograd(lambda a, p: ops.mlp_grouped(a, p, slot.to(DEV), *shape, fp16=mode == "fp16"), [x], pool, dy)
        _check(f"mlp_grouped {shape} {mode}{' kept h' if save else ''}:", y, dx, dp, ref, kinks, shape)
        for p in (11, 50):
            assert float(y[p].abs().max()) == 0.0 and float(dx[p].abs().max()) == 0.0
        assert float(dp[3].abs().max()) == 0.0


@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_cat_two_segment_range(shape):
    """fp32 rows in two segments whose magnitudes differ by 2^10, 2^20, 2^30 (one scale per point over both)"""
    ops = _ops()
    n_in, n_out, nn, nl = shape
    x1, x2, params, dy0 = mr.two_segment_case(shape, N1[n_in], SEED)
    for mode, save in VARIANTS:
        ref, kinks, dy = _prepare(f"mlp_cat {shape} {mode}:", x1, params, dy0, shape, mode, x2=x2)
        with _save_hidden(save):
            y, (d1, d2), dp = _autograd(lambda a, b, p: ops.mlp_cat(a, b, p, n_out, nn, nl, fp16=mode == "fp16"), [x1, x2], params, dy)
        _check(f"mlp_cat {shape} {mode}{' kept h' if save else ''}:", y, torch.cat((d1, d2), 1), dp, ref, kinks, shape)


def _split_rows(x):
    """the split-row format's definition (test_gpu_split_rows._split_rows) with sr::scale_exp's exponent for EVERY row maximum:
    0 for a non-finite one, whose Inf then has lo = Inf - Inf = NaN, as the device producers write it"""
    e = mr.scale_exp(x.abs().amax(dim=1)).to(torch.int32)
    xs = torch.ldexp(x, e[:, None])
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return torch.cat((hi, lo), 1).contiguous(), e.contiguous()


def _split_launch(x1, x2, params, dy, shape, fp16):
    """dns_mlp_fwd_split / dns_mlp_bwd_split on rows split by the format's definition (one or two segments)"""
    ops, lib, DnsSplitRows, check, ptr, stream_ptr = _lib()
    n_in, n_out, nn, nl = shape
    P = x1.shape[0]
    flag = ops.MLP_FP16_FLAG if fp16 else 0
    keep, segs = [], []
    for seg in (x1, x2):
        if seg is None:
            segs.append(None)
            continue
        xs, ex = _split_rows(seg)
        if fp16:
            xs = xs[:, :seg.shape[1]].contiguous()
        xs, ex = xs.to(DEV), ex.to(DEV)
        keep += [xs, ex]
        segs.append(_rows(DnsSplitRows, xs, ex, seg.shape[1], lo=not fp16))
    r1 = C.byref(segs[0])
    r2 = C.byref(segs[1]) if segs[1] is not None else None
    n1 = x1.shape[1] if x2 is not None else 0
    p, dyd = params.to(DEV), dy.to(DEV)
    y = torch.zeros(P, n_out, device=DEV)
    d1 = torch.zeros(P, x1.shape[1], device=DEV)
    d2 = torch.zeros(P, x2.shape[1], device=DEV) if x2 is not None else None
    dp = torch.zeros_like(p)
    ws = torch.zeros(int(lib.dns_mlp_bwd_ws_floats(P, nn, nl)), device=DEV)
    check(lib.dns_mlp_fwd_split(r1, r2, n1, ptr(p), n_in, n_out, nn, nl, ptr(y), n_out, P, None, None, 0, flag, stream_ptr()),
          "dns_mlp_fwd_split")
    check(lib.dns_mlp_bwd_split(r1, r2, n1, ptr(dyd), n_out, ptr(p), n_in, n_out, nn, nl, ptr(d1), d1.shape[1], ptr(d2),
                                d2.shape[1] if d2 is not None else 0, ptr(dp), ptr(ws), P, None, None, 0, flag, stream_ptr()),
          "dns_mlp_bwd_split")
    torch.cuda.synchronize()
    dx = d1 if d2 is None else torch.cat((d1, d2), 1)
    return y.cpu(), dx.cpu(), dp.cpu(), ws.cpu()[:P * nn].reshape(P, nn)


def _check_split(what, got, ref, kinks, shape):
    """the split-row backward leaves dW_in to the streaming kernel: its part of dparams is not written; dH_1 is"""
    y, dx, dp, _ = got
    n_in, n_out, nn, nl = shape
    mr.assert_within(f"{what} y", y, ref["y"], ref["e_y"])
    mr.assert_within(f"{what} dx", dx, ref["dx"], ref["e_dx"])
    assert _absmax(dx[kinks]) == 0.0
    used, w_in = mr.used_count(shape), nn * n_in
    mr.assert_within(f"{what} dparams (W_h, W_out)", dp[w_in:used], ref["dparams"][w_in:], ref["e_dparams"][w_in:])
    assert _absmax(dp[used:]) == 0.0 and _absmax(dp[:w_in]) == 0.0


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_split_rows_range(shape, fp16):
    """split rows: row magnitudes and the clamp on one segment; two segments with their OWN exponents, aligned in the kernel
    (max(e - e_k, -24)), at ratios up to 2^30 either way"""
    n_in = shape[0]
    mode = "fp16" if fp16 else "exact"
    for name in ("rows", "clamp", "inrow-30"):
        x, params, dy0 = mr.finite_case(name, shape, SEED)
        ref, kinks, dy = _prepare(f"split rows {name} {shape} {mode}:", x, params, dy0, shape, mode, name)
        _check_split(f"split rows {name} {shape} {mode}:", _split_launch(x, None, params, dy, shape, fp16), ref, kinks, shape)
    if N1[n_in] % 16 == 0:
        x1, x2, params, dy0 = mr.two_segment_case(shape, N1[n_in], SEED)
        ref, kinks, dy = _prepare(f"split rows two segments {shape} {mode}:", x1, params, dy0, shape, mode, x2=x2, own_exps=True)
        _check_split(f"split rows two segments {shape} {mode}:", _split_launch(x1, x2, params, dy, shape, fp16), ref, kinks, shape)


def _half_launch(x16, params, dy, shape):
    ops = _ops()
    P = x16.shape[0]
    xd, p, dyd = x16.to(DEV), params.to(DEV), dy.to(DEV)
    y = ops.mlp_fwd_half(xd, p, *shape)
    dx = torch.full((P, shape[0]), float("nan"), device=DEV)
    dp = torch.zeros_like(p)
    ops.mlp_bwd_half(xd, dyd, p, *shape, d_x=dx, d_params=dp)
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), dp.cpu()


@pytest.mark.parametrize("shape", mr.NETS)
@pytest.mark.parametrize("name", ["clamp", "inrow-12", "inrow-12w"])
def test_mlp_half_rows_range(name, shape):
    """half rows carry no scale: the cases that stay inside f16's own range (rows of 2^-120 are zero rows in f16)"""
    x, params, dy0 = mr.finite_case(name, shape, SEED)
    x16 = x.half()
    ref, kinks, dy = _prepare(f"half rows {name} {shape}:", x16.float(), params, dy0, shape, "half")
    y, dx, dp = _half_launch(x16, params, dy, shape)
    _check(f"half rows {name} {shape}:", y, dx, dp, ref, kinks, shape)


@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_zeros_are_exact(shape):
    """An all-zero x row, an all-zero dy row and a point with every first-layer unit inactive give exactly zero y / dx rows; a
    batch of ONLY such points gives exactly zero weight gradients; a zero W_h gives exactly zero y, dx, dW_in and dW_out."""
    ops = _ops()
    n_in, n_out, nn, nl = shape
    x, params, dy = mr.base_inputs(shape, SEED)
    mats = mr.param_mats(params, shape)
    mats[0][:, 0] = mats[0][:, 0].abs() + 1.0               # column 0 of W_in positive: x = (-100, small ...) switches every unit off
    P = x.shape[0]
    kind = torch.arange(P) % 4                              # 0 ordinary, 1 zero x row, 2 zero dy row, 3 every unit inactive
    x[kind == 1] = 0.0
    dy[kind == 2] = 0.0
    x[kind == 3, 0] = -100.0
    x[kind == 3, 1:] *= 0.01
    assert bool((mr.forward64(x, params, shape)[1][0][kind == 3] < 0).all())
    runs = {"exact": lambda a, d, w: _autograd(lambda t, p: ops.mlp(t, p, *shape), [a], w, d),
            "fp16": lambda a, d, w: _autograd(lambda t, p: ops.mlp(t, p, *shape, fp16=True), [a], w, d),
            "half": lambda a, d, w: (lambda r: (r[0], [r[1]], r[2]))(_half_launch(a.half(), w, d, shape))}
    if n_in % 16 == 0:
        runs["split"] = lambda a, d, w: (lambda r: (r[0], [r[1]], r[2]))(_split_launch(a, None, w, d, shape, False))
    null = kind != 0
    for tag, run in runs.items():
        y, (dx,), dp = run(x, dy, params)
        assert float(y[(kind == 1) | (kind == 3)].abs().max()) == 0.0, tag
        assert float(dx[null].abs().max()) == 0.0, tag
        assert float(y[kind == 0].abs().max()) > 0 and float(dx[kind == 0].abs().max()) > 0 and float(dp.abs().max()) > 0
        y, (dx,), dp = run(x[null], dy[null], params)      # only null points: nothing reaches the weights
        assert float(dx.abs().max()) == 0.0 and float(dp.abs().max()) == 0.0, tag
        if nl == 2:
            w0 = params.clone()
            mr.param_mats(w0, shape)[1].zero_()
            y, (dx,), dp = run(x, dy, w0)
            assert float(y.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0, tag
            o = nn * n_in
            assert float(dp[:o].abs().max()) == 0.0 and float(dp[o + nn * nn:].abs().max()) == 0.0, tag


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------
def _poison(kind):
    if kind == "-nan":                                      # a NaN with the sign bit set
        return torch.tensor([-4194304], dtype=torch.int32).view(torch.float32)[0]
    return torch.tensor(float(kind))


def _nonfinite_rows(ref):
    return ~torch.isfinite(ref).all(dim=-1)


def _assert_poisoned(what, got, ref):
    """every entry that is non-finite in the float64 reference is non-finite from the kernel (the kind need not match)"""
    bad = ~torch.isfinite(ref)
    assert bool(bad.any()), f"{what}: the reference is finite -- the case does not test anything"
    miss = bad & torch.isfinite(got)
    assert not bool(miss.any()), f"{what}: {int(miss.sum())} of {int(bad.sum())} non-finite reference entries came back finite"


PP, PC = 37, 5                                              # the poisoned point (second tile) and column


def _nonfinite_case(run, what, shape, poison, x, params, dy, dp_from=0):
    """run(x, params, dy) -> y, dx, dparams (cpu).  One poisoned column of one point of x, of dy, one weight.  dp_from: the
    first entry of dparams the entry point writes (the split-row backward leaves dW_in to the streaming kernel)."""
    v = _poison(poison)
    clean = run(x, params, dy)
    xp = x.clone()
    xp[PP, PC] = v
    y, _, _ = run(xp, params, dy)
    ref = mr.backward64(xp, params, dy, shape)
    assert bool(_nonfinite_rows(ref["y"])[PP])
    _assert_poisoned(f"{what} x={poison}: y", y, ref["y"])
    others = torch.arange(x.shape[0]) != PP
    assert torch.equal(y[others], clean[0][others]), f"{what} x={poison}: the other points' outputs changed"
    dyp = dy.clone()
    dyp[PP, PC] = v
    _, dx, dp = run(x, params, dyp)
    ref = mr.backward64(x, params, dyp, shape)
    assert bool(_nonfinite_rows(ref["dx"])[PP])
    _assert_poisoned(f"{what} dy={poison}: dx", dx, ref["dx"])
    _assert_poisoned(f"{what} dy={poison}: dparams", dp.reshape(-1)[dp_from:mr.used_count(shape)], ref["dparams"][dp_from:])
    assert torch.equal(dx[others], clean[1][others]), f"{what} dy={poison}: the other points' input gradients changed"
    wp = params.clone()
    mr.param_mats(wp, shape)[0][3, PC] = v
    y, _, _ = run(x, wp, dy)
    ref = mr.backward64(x, wp, dy, shape)
    _assert_poisoned(f"{what} weight={poison}: y", y, ref["y"])


@pytest.mark.parametrize("poison", ["nan", "-nan", "inf", "-inf"])
@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_propagates_non_finite(shape, fp16, poison):
    """fp32 rows (ops.mlp; MLP_SAVE_HIDDEN off and on: the backward's recompute path and the kept activations)"""
    ops = _ops()
    x, params, dy = mr.base_inputs(shape, SEED)
    for save in (False, True):
        def run(a, w, d):
            with _save_hidden(save):
                y, (dx,), dp = _autograd(lambda t, p: ops.mlp(t, p, *shape, fp16=fp16), [a], w, d)
            return y, dx, dp
        _nonfinite_case(run, f"mlp {shape} fp16={fp16} kept h={save}", shape, poison, x, params, dy)


@pytest.mark.parametrize("poison", ["nan", "-nan", "inf", "-inf"])
def test_mlp_cat_and_grouped_propagate_non_finite(poison):
    ops = _ops()
    shape = (112, 8, 32, 1)
    n_in, n_out, nn, nl = shape
    x, params, dy = mr.base_inputs(shape, SEED)

    def run_cat(a, w, d):
        y, (d1, d2), dp = _autograd(lambda s, t, p: ops.mlp_cat(s, t, p, n_out, nn, nl), [a[:, :48].contiguous(), a[:, 48:].contiguous()], w, d)
        return y, torch.cat((d1, d2), 1), dp
    _nonfinite_case(run_cat, "mlp_cat", shape, poison, x, params, dy)
    slot = torch.zeros(x.shape[0], dtype=torch.int64)

    def run_grouped(a, w, d):
        y, (dx,), dp = _autograd(lambda t, p: ops.mlp_grouped(t, p, slot.to(DEV), *shape), [a], w[None].contiguous(), d)
        return y, dx, dp[0]
    _nonfinite_case(run_grouped, "mlp_grouped", shape, poison, x, params, dy)


@pytest.mark.parametrize("poison", ["nan", "-nan", "inf", "-inf"])
@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_half_rows_propagate_non_finite(shape, poison):
    """half rows: the packed ReLU keeps a NaN of either sign (csrc/mlp_half.hpp pk_relu)"""
    x, params, dy = mr.base_inputs(shape, SEED)
    x = x.half().float()
    _nonfinite_case(lambda a, w, d: _half_launch(a.half(), w, d, shape), f"half rows {shape}", shape, poison, x, params, dy)


@pytest.mark.parametrize("poison", ["nan", "-nan", "inf", "-inf"])
@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("shape", mr.NETS)
def test_mlp_split_rows_propagate_non_finite(shape, fp16, poison):
    """a non-finite value that arrives in a split row (its exponent is 0: a non-finite maximum leaves the scale at 1), in dy, in
    a weight"""
    x, params, dy = mr.base_inputs(shape, SEED)
    _nonfinite_case(lambda a, w, d: _split_launch(a, None, w, d, shape, fp16)[:3], f"split rows {shape} fp16={fp16}", shape, poison,
                    x, params, dy, dp_from=shape[2] * shape[0])
