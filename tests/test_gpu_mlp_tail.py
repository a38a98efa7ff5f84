"""The tail-column form of the split-operand MLP kernels (csrc/mlp_split.hpp "tail column", mlp_split_bwd.inc TAIL): networks
with n_out = 1 and 33 run their last output column on the vector ALU -- against the float64 reference and the bound
tests/mlp_ref.py derives for the MATRIX path (the tail's plain fp32 FMAs make no operand error and drop no product term; its
summation tree is at most 11 roundings deep at 64 hidden units, inside the model's accumulation term: no tolerance is added here),
with the margins recorded in parity_report.json as tests/test_gpu_mlp_range.py does.  Neighbouring widths (32, 34, 3) keep the
matrix-only path and are held to the same reference.  Inputs and seed: tests/mlp_tail_cases.py (near-kink share pinned on the
CPU by tests/test_mlp_tail_ref.py)."""
import pytest
import torch

import mlp_ref as mr
import mlp_tail_cases as tc
from test_gpu_mlp_range import _absmax, _assert_poisoned, _autograd, _check, _check_params, _nonfinite_rows, _ops, _poison, _prepare, _save_hidden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = tc.SEED
P = tc.P_VAR
WIDE = [s for s in tc.TAIL_NETS if s[0] == 80]              # DNS_MLP_DX_FROM(48) needs more than 48 input columns


def _raw(shape, x, w, dy, x2=None, fwd_flags=0, bwd_flags=0, dx0=None, dx20=None, want_dp=True, keep_h=False, dwin_after=False,
         count=None):
    """dns_mlp_fwd + dns_mlp_bwd through the C ABI.  shape: the ABI's (n_in = storage width of W_in); x / x2: the segment(s) as
    given; w: parameters or prepared images.  dx0 / dx20: initial contents of d_x / d_x2 (default NaN: whatever the kernel leaves
    untouched stays visible).  Returns y, d_x, d_x2, d_params on the CPU."""
    ops = _ops()
    from dns_slam_amd._lib import check, ptr, stream_ptr
    lib = ops.lib
    n_in, n_out, nn, nl = shape
    n = x.shape[0]
    xd, x2d, dyd, wd = x.to(DEV), None if x2 is None else x2.to(DEV), dy.to(DEV), w.to(DEV)
    n1 = x.shape[1] if x2 is not None else 0
    y = torch.full((n, n_out), float("nan"), device=DEV)
    nanlike = lambda t: torch.full(t.shape, float("nan"), device=DEV)
    dx = nanlike(x) if dx0 is None else dx0.to(DEV).clone()
    dx2 = None if x2 is None else (nanlike(x2) if dx20 is None else dx20.to(DEV).clone())
    dp = torch.zeros(count if count is not None else wd.numel(), device=DEV) if want_dp else None
    ws = torch.zeros(int(lib.dns_mlp_bwd_ws_floats(n, nn, nl)), device=DEV) if want_dp else None
    hs = torch.empty(nl * n * nn, device=DEV) if keep_h else None
    st = stream_ptr()
    check(lib.dns_mlp_fwd(ptr(xd), xd.stride(0), ptr(x2d), 0 if x2d is None else x2d.stride(0), n1, ptr(wd), n_in, n_out, nn, nl, ptr(y),
                          n_out, n, None, None, 0, ptr(hs), fwd_flags, st), "dns_mlp_fwd")
    flags = bwd_flags | (ops.MLP_NO_DWIN_FLAG if dwin_after else 0)
    check(lib.dns_mlp_bwd(ptr(xd), xd.stride(0), ptr(x2d), 0 if x2d is None else x2d.stride(0), n1, ptr(dyd), n_out, ptr(wd), n_in, n_out,
                          nn, nl, ptr(dx), dx.stride(0), ptr(dx2), 0 if dx2 is None else dx2.stride(0), ptr(dp), ptr(ws), n, None, None, 0,
                          ptr(hs), flags, st), "dns_mlp_bwd")
    if dwin_after:
        assert _absmax(dp[:nn * n_in]) == 0.0                   # the first layer's block is untouched until ...
        check(lib.dns_mlp_dwin(ptr(xd), xd.stride(0), ptr(x2d), 0 if x2d is None else x2d.stride(0), n1, n_in, nn, nl, ptr(dp), ptr(ws), n,
                               None, None, 0, bwd_flags & 0xff0000, st), "dns_mlp_dwin")
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu()
    return c(y), c(dx), c(dx2), c(dp)


def _prepared(shape, params, live=0):
    ops = _ops()
    from dns_slam_amd._lib import check, ptr, stream_ptr
    lib = ops.lib
    n_in, n_out, nn, nl = shape
    nf = int(lib.dns_mlp_prepared_floats(live or n_in, n_out, nn, nl))
    assert nf > 0 and nf % 4 == 0
    prep = torch.empty(nf, device=DEV)
    pd = params.to(DEV)
    check(lib.dns_mlp_prepare(ptr(pd), n_in, n_out, nn, nl, 1, 0, ptr(prep), ops.MLP_LIVE_IN(live) if live else 0, stream_ptr()),
          "dns_mlp_prepare")
    torch.cuda.synchronize()
    return prep


# One reference per case, shared by the tests that need it (never modified)
_CACHE = {}


def _case(shape, n=P):
    key = (shape, n)
    if key not in _CACHE:
        x, params, dy0 = tc.plain_case(shape, n, SEED)
        ref, kinks, dy = _prepare(f"tail {shape} P={n}:", x, params, dy0, shape, "exact")
        _CACHE[key] = (x, params, dy, ref, kinks)
    return _CACHE[key]


@pytest.mark.parametrize("n", tc.POINTS)
@pytest.mark.parametrize("shape", tc.TAIL_NETS + tc.OLD_NETS)
def test_mlp_tail_points(shape, n):
    """ops.mlp at 1, 32, 33, 101 and 517 points: the tail form (n_out = 1, 33) and its neighbours on the matrix-only path"""
    ops = _ops()
    x, params, dy, ref, kinks = _case(shape, n)
    y, (dx,), dp = _autograd(lambda a, p: ops.mlp(a, p, *shape), [x], params, dy)
    _check(f"tail {shape} P={n}:", y, dx, dp, ref, kinks, shape)


@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_grouped(shape):
    """4 weight sets behind row_index / tile_group: a set of exactly min_count points, an empty set, points without a set"""
    ops = _ops()
    x, pool, dy0, slot = tc.group_case(shape, SEED)
    ref, kinks, dy = _prepare(f"tail grouped {shape}:", x, pool, dy0, shape, "exact", group=slot, min_count=tc.MIN_COUNT)
    y, (dx,), dp = _autograd(lambda a, p: ops.mlp_grouped(a, p, slot.to(DEV), *shape, min_count=tc.MIN_COUNT), [x], pool, dy)
    _check(f"tail grouped {shape}:", y, dx, dp, ref, kinks, shape)
    none = slot < 0
    assert _absmax(y[none]) == 0.0 and _absmax(dx[none]) == 0.0 and _absmax(dp[2]) == 0.0
    assert _absmax(y[slot == 1]) > 0 and _absmax(dp[1]) > 0


@pytest.mark.parametrize("shape", tc.LIVE_NETS)
def test_mlp_tail_live_two_segment(shape):
    """segments of 48 + 32 live columns, DNS_MLP_LIVE_IN(80) on a 112-wide W_in: the 80-input network on W_in's first 80 columns;
    then the same launch adding into d_x and d_x2 (two-segment accumulate): fp32 sums of the overwriting launch's values, bit for bit"""
    ops = _ops()
    n_in, n_out, nn, nl = shape
    x1, x2, params, dy0, live = tc.live_case(shape, SEED)
    ls = tc.live_shape(shape)
    what = f"tail live {shape}:"
    ref, kinks, dy = _prepare(what, x1, live, dy0, ls, "exact", x2=x2)
    flag = ops.MLP_LIVE_IN(tc.LIVE)
    y, d1, d2, dp = _raw(shape, x1, params, dy, x2=x2, fwd_flags=flag, bwd_flags=flag)
    mr.assert_within(f"{what} y", y, ref["y"], ref["e_y"])
    mr.assert_within(f"{what} dx", torch.cat((d1, d2), 1), ref["dx"], ref["e_dx"])
    w_in = dp[:nn * n_in].reshape(nn, n_in)
    assert _absmax(w_in[:, tc.LIVE:]) == 0.0, "the dead columns of W_in received a gradient"
    got = torch.cat((w_in[:, :tc.LIVE].reshape(-1), dp[nn * n_in:]))
    _check_params(what, got, ref, ls)
    g = torch.Generator().manual_seed(SEED + 50)
    a1, a2 = torch.randn(x1.shape, generator=g), torch.randn(x2.shape, generator=g)
    _, s1, s2, _ = _raw(shape, x1, params, dy, x2=x2, fwd_flags=flag, bwd_flags=flag | 3, dx0=a1, dx20=a2)
    assert torch.equal(s1, a1 + d1) and torch.equal(s2, a2 + d2)


@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_dx_forms(shape):
    """d_x overwritten (against the reference), read-add-write (the fp32 sum of the same values, bit for bit) and, on the 80-input
    networks, DNS_MLP_DX_FROM(48): columns from 48 on as before, the ones below untouched"""
    ops = _ops()
    x, params, dy, ref, kinks = _case(shape)
    y, dx, _, dp = _raw(shape, x, params, dy)
    _check(f"tail raw {shape}:", y, dx, dp, ref, kinks, shape)
    a = torch.randn(x.shape, generator=torch.Generator().manual_seed(SEED + 60))
    _, s, _, _ = _raw(shape, x, params, dy, bwd_flags=1, dx0=a)
    assert torch.equal(s, a + dx)
    if shape in WIDE:
        _, f, _, dpf = _raw(shape, x, params, dy, bwd_flags=ops.MLP_DX_FROM(48))
        assert torch.equal(f[:, 48:], dx[:, 48:]) and bool(torch.isnan(f[:, :48]).all())
        _check_params(f"tail DX_FROM(48) {shape}:", dpf, ref, shape)


@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_kept_hidden_and_separate_dwin(shape):
    """MLP_SAVE_HIDDEN (the backward reads the activations the forward kept) and DNS_MLP_NO_DWIN followed by dns_mlp_dwin"""
    ops = _ops()
    x, params, dy, ref, kinks = _case(shape)
    with _save_hidden(True):
        y, (dx,), dp = _autograd(lambda a, p: ops.mlp(a, p, *shape), [x], params, dy)
    _check(f"tail kept h {shape}:", y, dx, dp, ref, kinks, shape)
    y, dx, _, dp = _raw(shape, x, params, dy, keep_h=True)
    _check(f"tail kept h (raw) {shape}:", y, dx, dp, ref, kinks, shape)
    y2, dx2, _, dp2 = _raw(shape, x, params, dy, dwin_after=True)
    _check(f"tail dwin apart {shape}:", y2, dx2, dp2, ref, kinks, shape)


@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_identities(shape):
    """bit for bit: prepared images against images built in the kernel; d_x of the frozen form (no d_params: 8 waves) against
    d_x of the weight-gradient form; y and d_x from call to call"""
    ops = _ops()
    x, params, dy, ref, kinks = _case(shape)
    y, dx, _, dp = _raw(shape, x, params, dy)
    y2, dx2, _, _ = _raw(shape, x, params, dy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    prep = _prepared(shape, params)
    f = ops.MLP_PREPARED_FLAG
    yp, dxp, _, dpp = _raw(shape, x, prep, dy, fwd_flags=f, bwd_flags=f, count=params.numel())
    assert torch.equal(y, yp) and torch.equal(dx, dxp)
    _check_params(f"tail prepared {shape}:", dpp, ref, shape)
    _, dxf, _, _ = _raw(shape, x, params, dy, want_dp=False)
    _, dxfp, _, _ = _raw(shape, x, prep, dy, fwd_flags=f, bwd_flags=f, want_dp=False)
    assert torch.equal(dx, dxf) and torch.equal(dx, dxfp)


def _tail_row(params, shape):
    return mr.param_mats(params, shape)[-1][shape[1] - 1]


@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_edges(shape):
    """W_out's tail row zero: exact zeros in the tail output and in everything its dY column feeds; dY only in the tail column;
    dY everywhere but there (the tail row of dW_out is then exactly zero)"""
    n_in, n_out, nn, nl = shape
    x, params, dy, ref, kinks = _case(shape)
    only = torch.zeros_like(dy)
    only[:, -1] = dy[:, -1]
    w0 = params.clone()
    _tail_row(w0, shape).zero_()
    y, dx, _, dp = _raw(shape, x, w0, only)
    assert _absmax(y[:, -1]) == 0.0 and (n_out == 1 or _absmax(y[:, :-1]) > 0)
    assert _absmax(dx) == 0.0, "a zero tail row passed a gradient"
    o = mr.used_count(shape) - n_out * nn
    assert _absmax(dp[:o]) == 0.0 and _absmax(dp[o + (n_out - 1) * nn:]) > 0     # only dW_out's tail row: dY^T H
    what = f"tail dy only in the tail column {shape}:"
    r = mr.analyse(x, params, only, shape, "exact")
    y, dx, _, dp = _raw(shape, x, params, only)
    _check(what, y, dx, dp, r, kinks, shape)
    assert _absmax(dx) > 0
    if n_out > 1:
        rest = dy.clone()
        rest[:, -1] = 0.0
        what = f"tail dy everywhere but the tail column {shape}:"
        r = mr.analyse(x, params, rest, shape, "exact")
        y, dx, _, dp = _raw(shape, x, params, rest)
        _check(what, y, dx, dp, r, kinks, shape)
        assert _absmax(dp[o + (n_out - 1) * nn:o + n_out * nn]) == 0.0


PP, PC = 37, 5                                              # the poisoned point (second tile) and column / hidden unit


@pytest.mark.parametrize("poison", ["nan", "-nan", "inf", "-inf"])
@pytest.mark.parametrize("shape", tc.TAIL_NETS)
def test_mlp_tail_propagates_non_finite(shape, poison):
    """NaN / -NaN / +-Inf in W_out's tail row, in the tail column of dY and in one x row: every entry that is non-finite in the
    float64 reference is non-finite from the kernels, and the other points keep their bits (test_gpu_mlp_range._nonfinite_case)"""
    n_in, n_out, nn, nl = shape
    x, params, dy = tc.plain_case(shape, P, SEED)
    v = _poison(poison)
    what = f"tail {shape} {poison}"
    run = lambda a, w, d: _raw(shape, a, w, d)
    cy, cdx, _, _ = run(x, params, dy)
    others = torch.arange(P) != PP
    wp = params.clone()
    _tail_row(wp, shape)[PC] = v
    y, dx, _, _ = run(x, wp, dy)
    ref = mr.backward64(x, wp, dy, shape)
    assert bool(_nonfinite_rows(ref["y"]).any())
    _assert_poisoned(f"{what} in W_out's tail row: y", y, ref["y"])
    _assert_poisoned(f"{what} in W_out's tail row: dx", dx, ref["dx"])
    dyp = dy.clone()
    dyp[PP, n_out - 1] = v
    _, dx, _, dp = run(x, params, dyp)
    ref = mr.backward64(x, params, dyp, shape)
    assert bool(_nonfinite_rows(ref["dx"])[PP])
    _assert_poisoned(f"{what} in dY's tail column: dx", dx, ref["dx"])
    _assert_poisoned(f"{what} in dY's tail column: dparams", dp[:mr.used_count(shape)], ref["dparams"])
    assert torch.equal(dx[others], cdx[others]), f"{what} in dY's tail column: the other points' input gradients changed"
    xp = x.clone()
    xp[PP, PC] = v
    y, _, _, _ = run(xp, params, dy)
    ref = mr.backward64(xp, params, dy, shape)
    assert bool(_nonfinite_rows(ref["y"])[PP])
    _assert_poisoned(f"{what} in x: y", y, ref["y"])
    assert torch.equal(y[others], cy[others]), f"{what} in x: the other points' outputs changed"
