"""Every form of the point encoder (csrc/encode.hip, csrc/dev_encode.hpp) against the float64 reference of tests/encode_ref.py, entry
by entry, no entry left out: forward values of the joint row (tiled kernel), OneBlob alone (tiled), the grid alone and separate
strided buffers (untiled kernel), x_out, the dy_dx buffer, and d_x from the saved Jacobian and from the re-gather -- at the edges the
named inputs of encode_ref.py hold (coordinates 0, 1, outside the box, on cell faces and bin edges, |x| around 4), at P = 1, 127,
128, 129 and 257, on three grids and at the n_bins where the host picks another path (16, 8: three OneBlob phases, the window form;
12: one phase, 16-byte staging; 5: scalar flush and staging; 4: the all-edges loop).

Bound per element:  |got - exp| <= k 2^-24 A + TINY,  A the reference's term-wise absolute sum, TINY = 2^-126 (a subnormal result).
k is the count of fp32 roundings on the longest chain of dependent operations to the element, read off the kernels' source
(derivation: the docstring of tests/encode_ref.py):

    features                     K_Y  = 11
    OneBlob bin                  K_OB = 14
    dy_dx                        K_J  = 7
    d_x, saved Jacobian          9 + L              per grid term   (L levels)
    d_x, re-gather               8 + L              per grid term
    d_x, OneBlob term            12 + max(n_bins - 1, 10) + L   (L = 0 without grid columns)
    with a bound                 + 1 on every d_x count; x_out is held bit for bit

Every case appends its worst |got - exp| / bound to util.REPORT.  Non-finite coordinates and table entries: the reference's pattern
of non-finite entries must be the kernel's, every other entry stays inside its bound.
"""
import os
import subprocess
import sys

import ctypes as C
import pytest
import torch

import encode_ref as er
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, TINY = er.U, er.TINY
SENTINEL = 12345.0

_GRID = {}


def _ops():
    from dns_slam_amd import ops
    return ops


def _bound():
    return torch.tensor(er.BOUND, dtype=torch.float64)


def _grid(grid, kind="uniform"):
    """(product GridMeta, flat device table); the product's level table must be the oracle's."""
    ops = _ops()
    if grid not in _GRID:
        hs, res, L = er.GRIDS[grid]
        pm = ops.GridMeta(hs, res, n_levels=L)
        want = [dict(scale=l.scale, resolution=l.resolution, size=l.size, offset=l.offset, hashed=bool(l.hashed)) for l in er.meta_of(grid).levels]
        assert pm.levels() == want and pm.total_rows == er.meta_of(grid).total_rows, grid
        _GRID[grid] = pm
    key = (grid, kind)
    if key not in _GRID:
        _GRID[key] = er.table(grid, kind).reshape(-1).to(DEV)
    return _GRID[grid], _GRID[key]


def _hold(what, got, exp, tol):
    """The pattern of non-finite entries is the reference's and every other entry is inside its bound -> worst ratio."""
    got = got.detach().cpu().double()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    worst, i = er.worst_ratio(got, exp, tol)
    fin = torch.isfinite(exp) & torch.isfinite(tol)
    scale = float(exp[fin].abs().max()) if bool(fin.any()) else 0.0
    d = float((got - exp)[fin].abs().max()) if bool(fin.any()) else 0.0
    REPORT.append((what, d / scale if scale else d, worst, U))
    print(f"{what}: worst ratio {worst:.3f} at flat index {i} (got {float(got.reshape(-1)[i]):.9e}, want {float(exp.reshape(-1)[i]):.9e}, "
          f"tol {float(tol.reshape(-1)[i]):.3e})")
    same = torch.isfinite(got) == torch.isfinite(exp)
    assert bool(same.all()), f"{what}: {int((~same).sum())} entries finite on one side only, first at flat index {int(torch.nonzero(~same.reshape(-1))[0])}"
    assert worst <= 1.0, f"{what}: worst ratio {worst:.2f}"
    return worst


def forward_reference(name, grid, n_bins, form, kind="uniform"):
    parts = []
    if form != "grid":
        y, A = er.oneblob_reference(name, grid, n_bins)
        parts.append((y, er.K_OB * U * A + TINY))
    if form != "pe":
        y, A, _, _ = er.grid_reference(name, grid, kind)
        parts.append((y, er.K_Y * U * A + TINY))
    return torch.cat([p[0] for p in parts], -1), torch.cat([p[1] for p in parts], -1)


def run_forward(name, grid, n_bins, form, kind="uniform"):
    """form: joint (tiled kernel), pe (OneBlob alone, tiled), grid (alone, untiled) -- through ops.encode."""
    ops = _ops()
    pm, tab = _grid(grid, kind)
    src = er.points(name, grid)[0]
    got = ops.encode(src.to(DEV), None if form == "pe" else tab, None if form == "pe" else pm, _bound() if name == "world" else None,
                     n_bins, form != "grid", form != "pe")
    return _hold(f"encode64 fwd {form} {name} grid {grid} n_bins {n_bins} {kind}", got, *forward_reference(name, grid, n_bins, form, kind))


def run_dx(name, grid, n_bins, form, saved, kind="uniform", gkind="randn", atomic=False):
    """d_x through ops.encode's backward.  saved: the forward keeps dy_dx (ops.SAVE_DY_DX); atomic: the table wants its gradient as
    per-corner atomics from the same kernel, which then re-gathers whatever was saved."""
    ops = _ops()
    pm, tab = _grid(grid, kind)
    src = er.points(name, grid)[0]
    L = pm.n_levels
    g_pe, g_grid = er.grad_cols(er.grads(src.shape[0], gkind), n_bins, L)
    gy = torch.cat(([g_pe] if form != "grid" else []) + ([g_grid] if form != "pe" else []), -1).to(DEV)
    keep = ops.SAVE_DY_DX, ops.SCATTER_FORM
    try:
        ops.SAVE_DY_DX = saved
        ops.SCATTER_FORM = (ops.SCATTER_ATOMIC, 0) if atomic else keep[1]
        xp = src.to(DEV).requires_grad_(True)
        t = tab.clone().requires_grad_(True) if atomic else tab
        y = ops.encode(xp, None if form == "pe" else t, None if form == "pe" else pm, _bound() if name == "world" else None, n_bins,
                       form != "grid", form != "pe")
        y.backward(gy)
    finally:
        ops.SAVE_DY_DX, ops.SCATTER_FORM = keep
    if atomic:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())
    exp, tol = er.dx_reference(name, grid, n_bins, kind, gkind, pe=form != "grid", grd=form != "pe", bound=name == "world",
                               saved=saved and not atomic)
    how = ("saved" if saved else "regather") + (" atomic" if atomic else "")
    return _hold(f"encode64 d_x {form} {how} {name} grid {grid} n_bins {n_bins} {kind}/{gkind}", xp.grad, exp, tol)


def abi_forward(src, bound, n_bins, grid, kind, pad_pe=None, pad_grid=None, want_dydx=True):
    """dns_encode_fwd through the C ABI.  pad_pe / pad_grid None: one joint buffer (the tiled kernel); else OneBlob and grid rows in
    separate buffers that many columns wider than the rows, sentinel-filled (the untiled kernel, as the MLP input rows are written).
    -> (pe buffer or joint buffer, grid buffer or None, x_out or None, dy_dx [L, 3, P, 2] or None)"""
    ops = _ops()
    from dns_slam_amd._lib import check, ptr, stream_ptr
    pm, tab = _grid(grid, kind)
    P, pe, gd = src.shape[0], 3 * n_bins, pm.out_dim
    b6 = ops._bound6(_bound()) if bound else None
    xo = torch.full((P, 3), SENTINEL, device=DEV) if bound else None
    jac = torch.full((pm.n_levels * 3 * P * 2,), SENTINEL, device=DEV) if want_dydx else None
    s = src.to(DEV).contiguous()
    if pad_pe is None:
        a, b = torch.full((P, pe + gd), SENTINEL, device=DEV), None
        args = (ptr(a), pe + gd, C.c_void_p(a.data_ptr() + 4 * pe), pe + gd)
    else:
        a, b = torch.full((P, pe + pad_pe), SENTINEL, device=DEV), torch.full((P, gd + pad_grid), SENTINEL, device=DEV)
        args = (ptr(a), pe + pad_pe, ptr(b), gd + pad_grid)
    check(ops.lib.dns_encode_fwd(ptr(s), b6, P, n_bins, ptr(tab), C.byref(pm.c), ptr(xo), *args, ptr(jac), stream_ptr()), "dns_encode_fwd")
    torch.cuda.synchronize()
    return a, b, xo, (jac.reshape(pm.n_levels, 3, P, 2) if want_dydx else None)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n_bins", er.N_BINS)
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_forward_joint_row(name, grid, n_bins):
    run_forward(name, grid, n_bins, "joint")


@pytest.mark.parametrize("n_bins", er.N_BINS)
@pytest.mark.parametrize("name", er.INPUTS)
def test_forward_oneblob_alone(name, n_bins):
    run_forward(name, "16_592", n_bins, "pe")


@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_forward_grid_alone(name, grid):
    run_forward(name, grid, 16, "grid")


@pytest.mark.parametrize("form", ["joint", "grid"])
@pytest.mark.parametrize("grid", list(er.GRIDS))
def test_forward_spread_table(grid, form):
    """Table magnitudes 10^[-6, 3]: sums that cancel, A >> |y|."""
    run_forward("edges", grid, 16, form, "spread")


@pytest.mark.parametrize("n_bins", er.N_BINS)
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", ["edges", "world", "P129"])
def test_forward_strided_buffers_x_out_and_dy_dx(name, grid, n_bins):
    """Separate OneBlob and grid buffers with row strides wider than the rows (the untiled kernel): values, untouched padding, x_out
    bit for bit, and the dy_dx it writes."""
    src, x = er.points(name, grid)
    bound = name == "world"
    a, b, xo, jac = abi_forward(src, bound, n_bins, grid, "uniform", pad_pe=5, pad_grid=3)
    pe, gd = 3 * n_bins, b.shape[1] - 3
    what = f"strided {name} grid {grid} n_bins {n_bins}"
    assert bool((a[:, pe:] == SENTINEL).all()) and bool((b[:, gd:] == SENTINEL).all()), f"{what}: padding columns written"
    exp, tol = forward_reference(name, grid, n_bins, "joint")
    _hold(f"encode64 fwd {what}", torch.cat((a[:, :pe], b[:, :gd]), -1), exp, tol)
    if bound:
        assert torch.equal(xo.cpu().view(torch.int32), x.view(torch.int32)), f"{what}: x_out is not the reference's normalisation"
    _, _, J, AJ = er.grid_reference(name, grid)
    _hold(f"encode64 dy_dx {what}", jac, J, er.K_J * U * AJ + TINY)


@pytest.mark.parametrize("kind", ["uniform", "spread"])
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_dy_dx_of_the_tiled_forward(name, grid, kind):
    src, x = er.points(name, grid)
    n_bins = 16 if kind == "uniform" else 5
    a, _, xo, jac = abi_forward(src, name == "world", n_bins, grid, kind)
    _hold(f"encode64 fwd tiled abi {name} grid {grid} n_bins {n_bins} {kind}", a, *forward_reference(name, grid, n_bins, "joint", kind))
    if name == "world":
        assert torch.equal(xo.cpu().view(torch.int32), x.view(torch.int32))
    _, _, J, AJ = er.grid_reference(name, grid, kind)
    _hold(f"encode64 dy_dx tiled {name} grid {grid} {kind}", jac, J, er.K_J * U * AJ + TINY)


# ----------------------------------------------------------------------------- d_x
@pytest.mark.parametrize("saved", [True, False], ids=["saved", "regather"])
@pytest.mark.parametrize("n_bins", er.N_BINS)
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_d_x_joint_row(name, grid, n_bins, saved):
    spread = (er.INPUTS.index(name) + er.N_BINS.index(n_bins)) % 2 == 1
    run_dx(name, grid, n_bins, "joint", saved, "spread" if spread else "uniform", "spread" if spread else "randn")


@pytest.mark.parametrize("gkind", ["randn", "spread"])
@pytest.mark.parametrize("n_bins", er.N_BINS)
@pytest.mark.parametrize("name", er.INPUTS)
def test_d_x_oneblob_alone(name, n_bins, gkind):
    run_dx(name, "16_592", n_bins, "pe", True, "uniform", gkind)


@pytest.mark.parametrize("saved", [True, False], ids=["saved", "regather"])
@pytest.mark.parametrize("kind", ["uniform", "spread"])
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_d_x_grid_alone(name, grid, kind, saved):
    run_dx(name, grid, 16, "grid", saved, kind, "spread" if kind == "spread" else "randn")


@pytest.mark.parametrize("saved", [True, False], ids=["saved", "regather"])
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", ["edges", "world", "P129"])
def test_d_x_beside_the_atomic_table_gradient(name, grid, saved):
    """SCATTER_ATOMIC: the kernel that writes d_x also writes d_table and takes the re-gather branch even with a saved Jacobian."""
    run_dx(name, grid, 16, "joint", saved, atomic=True)
    run_dx(name, grid, 5, "joint", saved, "spread", "spread", atomic=True)


# ----------------------------------------------------------------------------- phase splits (DNS_ENC_PHASES is read once per process)
@pytest.mark.parametrize("phases", ["1,1", "3,8"])
def test_phase_splits_in_a_fresh_process(phases):
    env = dict(os.environ, DNS_ENC_PHASES=phases)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "encode_phases_child.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"child exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"OK phases {phases}" in r.stdout, r.stdout[-2000:]
    for line in r.stdout.splitlines():
        if line.startswith("REPORT "):
            _, worst, what = line.split(" ", 2)
            REPORT.append((f"{what} [DNS_ENC_PHASES={phases}]", float("nan"), float(worst), U))


# ----------------------------------------------------------------------------- non-finite
def _nonfinite_points():
    x = er.points("P129", "16_592")[1].clone()
    nan, inf = float("nan"), float("inf")
    x[3, 0], x[64, 1], x[128, 2] = nan, inf, -inf          # first workgroup, its middle, the one-row tail
    x[77] = torch.tensor([nan, inf, -inf])
    return x, ~torch.isfinite(x).all(-1)


def _hold_rows(what, got, exp, tol, bad, row_dim):
    """Pattern everywhere; values only in the rows without a non-finite coordinate (the others' finite entries depend on the cell a
    NaN is given, which no contract fixes)."""
    shape = [1] * exp.dim()
    shape[row_dim] = -1
    tol = torch.where(bad.reshape(shape).expand_as(tol), torch.full_like(tol, float("inf")), tol)
    return _hold(what, got, exp, tol)


@pytest.mark.parametrize("n_bins", [16, 5])
@pytest.mark.parametrize("grid", ["16_592", "14_128_L4"])
def test_non_finite_coordinates(grid, n_bins):
    """NaN, +Inf, -Inf on one axis of a few rows (and on all three of one): a non-finite coordinate shows in every column that
    depends on it -- the reference's pattern -- and never leaves a finite OneBlob row; all other rows stay inside their bounds."""
    ops = _ops()
    pm, tab = _grid(grid)
    meta = er.meta_of(grid)
    x, bad = _nonfinite_points()
    L = pm.n_levels
    yo, Ao = er.oneblob64(x, n_bins)
    yg, Ag, J, AJ = er.grid64(x, er.table(grid), meta)
    assert bool(torch.isnan(yo[3, :n_bins]).all()) and bool(torch.isfinite(yo[3, n_bins:]).all())       # the reference itself
    tol_ob, tol_g = er.K_OB * U * Ao + TINY, er.K_Y * U * Ag + TINY
    what = f"encode64 non-finite x grid {grid} n_bins {n_bins}"
    xd = x.to(DEV)
    _hold_rows(f"{what} joint", ops.encode(xd, tab, pm, None, n_bins), torch.cat((yo, yg), -1), torch.cat((tol_ob, tol_g), -1), bad, 0)
    _hold_rows(f"{what} OneBlob alone", ops.encode(xd, None, None, None, n_bins, True, False), yo, tol_ob, bad, 0)
    _hold_rows(f"{what} grid alone", ops.encode(xd, tab, pm, None, n_bins, False, True), yg, tol_g, bad, 0)
    _, _, _, jac = abi_forward(x, False, n_bins, grid, "uniform")
    _hold_rows(f"{what} dy_dx", jac, J, er.K_J * U * AJ + TINY, bad, 2)
    g_pe, g_grid = er.grad_cols(er.grads(x.shape[0]), n_bins, L)
    d_ob, A_ob = er.oneblob_dx64(x, n_bins, g_pe)
    d_g, A_g = er.grid_dx64(J, AJ, g_grid)
    keep = ops.SAVE_DY_DX
    try:
        for saved in (True, False):
            ops.SAVE_DY_DX = saved
            kg = er.k_dx_saved(L) if saved else er.k_dx_regather(L)
            for form, gy, exp, tol in (("joint", torch.cat((g_pe, g_grid), -1), d_ob + d_g, er.k_ob_dx(n_bins, L) * U * A_ob + kg * U * A_g),
                                       ("pe", g_pe, d_ob, er.k_ob_dx(n_bins, 0) * U * A_ob), ("grid", g_grid, d_g, kg * U * A_g)):
                xp = xd.clone().requires_grad_(True)
                ops.encode(xp, None if form == "pe" else tab, None if form == "pe" else pm, None, n_bins, form != "grid",
                           form != "pe").backward(gy.to(DEV))
                _hold_rows(f"{what} d_x {form} {'saved' if saved else 'regather'}", xp.grad, exp, tol + TINY, bad, 0)
                if form != "grid":                   # a non-finite coordinate never leaves an all-finite gradient row
                    assert not bool(torch.isfinite(xp.grad.cpu()[bad]).all(-1).any())
    finally:
        ops.SAVE_DY_DX = keep


@pytest.mark.parametrize("grid", ["16_592", "12_64"])
def test_non_finite_table_entries(grid):
    """One table entry NaN, one Inf.  The Inf sits at a corner that a point with fraction exactly 0 reads with weight 0: 0 * Inf is
    NaN, as IEEE and the reference have it.  Rows that read neither entry are unaffected."""
    ops = _ops()
    pm, _ = _grid(grid)
    meta = er.meta_of(grid)
    x = er.points("edges", grid)[1]
    rows, fr = er.tr.hashgrid_indices(x, meta)
    level = 2
    p0 = int(torch.nonzero((fr[:, level] == 0).all(-1))[0])            # weight 1 on corner 0, 0 on the seven others
    r_inf, r_nan = int(rows[p0, level, 7]), int(rows[200, 0, 3])
    assert r_inf != int(rows[p0, level, 0]) and float(fr[200, 0].min()) > 0
    tab = er.table(grid).clone()
    tab[r_inf, 1], tab[r_nan, 0] = float("inf"), float("nan")
    reads = ((rows == r_inf) | (rows == r_nan)).any(-1).any(-1)
    assert bool(reads[p0]) and bool(reads[200]) and int((~reads).sum()) > 100
    yg, Ag, J, AJ = er.grid64(x, tab, meta)
    assert bool(torch.isnan(yg[p0, 2 * level + 1])) and bool(torch.isfinite(yg[~reads]).all())
    td = tab.reshape(-1).to(DEV)
    what = f"encode64 non-finite table grid {grid}"
    _hold(f"{what} joint", ops.encode(x.to(DEV), td, pm, None, 16)[:, 48:], yg, er.K_Y * U * Ag + TINY)
    g_grid = er.grad_cols(er.grads(x.shape[0]), 16, pm.n_levels)[1]
    d_g, A_g = er.grid_dx64(J, AJ, g_grid)
    keep = ops.SAVE_DY_DX
    try:
        for saved in (True, False):
            ops.SAVE_DY_DX = saved
            xp = x.to(DEV).requires_grad_(True)
            ops.encode(xp, td, pm, None, 16, False, True).backward(g_grid.to(DEV))
            kg = er.k_dx_saved(pm.n_levels) if saved else er.k_dx_regather(pm.n_levels)
            _hold(f"{what} d_x {'saved' if saved else 'regather'}", xp.grad, d_g, kg * U * A_g + TINY)
    finally:
        ops.SAVE_DY_DX = keep
