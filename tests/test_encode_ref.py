"""tests/encode_ref.py held on the CPU: it equals a plain per-point, per-level, per-corner loop; its d_x equals a central difference
of its own forward; it contains the float32 oracle inside the bounds tests/test_gpu_encode.py uses, on every named input; and those
bounds REJECT seven wrong encoders on the `edges` input (each emulated in float32 torch) -- a mutant the bound accepted would mean
the inputs or the bound are too weak to hold the kernels."""
import numpy as np
import pytest
import torch

import encode_ref as er
from oracle import tcnn_ref as tr

U, TINY = er.U, er.TINY


# ----------------------------------------------------------------------------- the reference against plain loops
def _loop_point(x, tab, meta, g_grid):
    """One point in Python floats: features, Jacobian and d_x (with their absolute sums), corner by corner."""
    rows, fr = tr.hashgrid_indices(x[None], meta)
    y, A, J, AJ = [], [], [], []
    dx, Adx = [0.0] * 3, [0.0] * 3
    for l, lvl in enumerate(meta.levels):
        f = [float(fr[0, l, a]) for a in range(3)]
        v = [[float(tab[int(rows[0, l, c]), k]) for k in range(2)] for c in range(8)]
        for k in range(2):
            acc = aacc = 0.0
            for c in range(8):
                w = 1.0
                for a in range(3):
                    w *= f[a] if (c >> a) & 1 else 1.0 - f[a]
                acc += w * v[c][k]
                aacc += w * abs(v[c][k])
            y.append(acc)
            A.append(aacc)
        for a in range(3):
            for k in range(2):
                acc = aacc = 0.0
                for c in range(8):
                    if (c >> a) & 1:
                        continue
                    w = 1.0
                    for o in range(3):
                        if o != a:
                            w *= f[o] if (c >> o) & 1 else 1.0 - f[o]
                    acc += w * (v[c | (1 << a)][k] - v[c][k])
                    aacc += w * (abs(v[c | (1 << a)][k]) + abs(v[c][k]))
                J.append((l, a, k, float(lvl.scale) * acc))
                AJ.append(float(lvl.scale) * aacc)
                dx[a] += float(lvl.scale) * acc * float(g_grid[2 * l + k])
                Adx[a] += float(lvl.scale) * aacc * abs(float(g_grid[2 * l + k]))
    return y, A, J, AJ, dx, Adx


@pytest.mark.parametrize("grid", list(er.GRIDS))
def test_grid_reference_equals_a_plain_loop(grid):
    meta, tab = er.meta_of(grid), er.table(grid)
    x = er.points("edges", grid)[1]
    n_hand = 60
    pick = [0, 3, 4, 5, 6, 22, n_hand, 200, 256]         # hand rows (0, nextafter, an integer-pos row, dealt values) and uniform rows
    pick += [int(i) for i in torch.nonzero((x < 0).all(-1)).reshape(-1)[:1]]     # negative on all three axes
    y, Ay, J, AJ = er.grid_reference("edges", grid)
    g_grid = er.grad_cols(er.grads(x.shape[0]), 16, meta.n_levels)[1]
    dx, Adx = er.grid_dx64(J, AJ, g_grid)
    for p in pick:
        ly, lA, lJ, lAJ, ldx, lAdx = _loop_point(x[p], tab, meta, g_grid[p])
        assert np.allclose(y[p].numpy(), ly, rtol=0, atol=1e-14 * max(lA)), p
        assert np.allclose(Ay[p].numpy(), lA, rtol=1e-14, atol=0), p
        for (l, a, k, val), aval in zip(lJ, lAJ):
            assert abs(float(J[l, a, p, k]) - val) <= 1e-14 * aval + 1e-300, (p, l, a, k)
            assert abs(float(AJ[l, a, p, k]) - aval) <= 1e-14 * aval, (p, l, a, k)
        assert np.allclose(dx[p].numpy(), ldx, rtol=0, atol=1e-13 * max(lAdx)), p
        assert np.allclose(Adx[p].numpy(), lAdx, rtol=1e-13, atol=0), p


def _loop_oneblob(x, n):
    def cdf(v):
        u = v * n
        return min(max(15.0 / 16.0 * u * (1 - 2.0 / 3.0 * u * u + 0.2 * u ** 4) + 0.5, 0.0), 1.0)

    def pdf(v):
        u = v * n
        return 0.0 if u * u > 1 else 15.0 / 16.0 * n * (1 - u * u) ** 2
    G = [sum(cdf(b / n - x + s) for s in (0.0, -1.0, 1.0)) for b in range(n)]
    Gp = [sum(pdf(b / n - x + s) for s in (0.0, -1.0, 1.0)) for b in range(n)]
    G.append(G[0] + 1.0)
    Gp.append(Gp[0])
    return [G[b + 1] - G[b] for b in range(n)], [-(Gp[b + 1] - Gp[b]) for b in range(n)]


@pytest.mark.parametrize("n_bins", er.N_BINS)
def test_oneblob_reference_equals_a_plain_loop(n_bins):
    x = er.points("edges", "12_64")[1]
    g = er.grad_cols(er.grads(x.shape[0]), n_bins, 16)[0]
    y, A = er.oneblob64(x, n_bins)
    dx, Adx = er.oneblob_dx64(x, n_bins, g)
    assert bool((A >= y.abs()).all()) and bool((Adx >= dx.abs()).all())
    for p in list(range(0, 80, 3)) + [200, 256]:
        for a in range(3):
            ly, ld = _loop_oneblob(float(x[p, a]), n_bins)
            assert np.allclose(y[p, a * n_bins:(a + 1) * n_bins].numpy(), ly, rtol=0, atol=1e-13), (p, a)
            want = sum(float(g[p, a * n_bins + b]) * ld[b] for b in range(n_bins))
            assert abs(float(dx[p, a]) - want) <= 1e-12 * float(Adx[p, a]), (p, a)
        assert abs(float(y[p].sum()) - 3.0) < 1e-12                   # the bins of an axis partition the kernel's unit mass


def test_oneblob_reference_keeps_a_nan():
    x = torch.tensor([[float("nan"), float("inf"), -float("inf")], [0.25, 0.5, 0.75]])
    y, _ = er.oneblob64(x, 8)
    dx, _ = er.oneblob_dx64(x, 8, torch.ones(2, 24))
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(dx[0]).all())
    assert bool(torch.isfinite(y[1]).all()) and bool(torch.isfinite(dx[1]).all())


# ----------------------------------------------------------------------------- d_x against a central difference
@pytest.mark.parametrize("grid", list(er.GRIDS))
def test_grid_jacobian_equals_a_central_difference_of_the_forward(grid):
    meta, tab = er.meta_of(grid), er.table(grid)
    x = er._uniform(400, 77)
    rows, fr = tr.hashgrid_indices(x, meta)
    keep = ((fr > 0.01) & (fr < 0.99)).all(-1).all(-1)                  # strictly inside a cell on every level
    assert int(keep.sum()) >= 20
    x, rows, f = x[keep], rows[keep], fr[keep].double()
    _, _, J, AJ = er.grid64(x, tab, meta)
    v = tab.double()[rows]
    h = 1e-3                                                             # in units of the fraction: d/dx = scale d/df
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        cd = (er.interp64(f + e, v)[0] - er.interp64(f - e, v)[0]) / (2 * h)           # [P, L, 2]
        s = torch.tensor([float(l.scale) for l in meta.levels], dtype=torch.float64)[None, :, None]
        want = (s * cd).permute(1, 0, 2)
        assert bool(((J[:, a] - want).abs() <= 1e-11 * AJ[:, a] + 1e-300).all()), a


@pytest.mark.parametrize("n_bins", er.N_BINS)
def test_oneblob_derivative_equals_a_central_difference_of_the_forward(n_bins):
    x = (torch.rand(300, 3, generator=torch.Generator().manual_seed(78)) * 3.0 - 1.0).double()
    g = torch.randn(300, 3 * n_bins, generator=torch.Generator().manual_seed(79)).double()
    dx, _ = er.oneblob_dx64(x, n_bins, g)
    h = 1e-6
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        cd = ((er.oneblob64(x + e, n_bins)[0] - er.oneblob64(x - e, n_bins)[0]) * g).sum(-1) / (2 * h)
        # (the quartic's third derivative is ~ 60 n^4: the difference's own error is ~ 1e-11 n^4 per unit gradient)
        assert bool(((dx[:, a] - cd).abs() <= 1e-10 * n_bins ** 4 * g.abs().sum(-1)).all()), a


# ----------------------------------------------------------------------------- the float32 oracle inside the bounds
def _oracle(x, tab, meta, n_bins, g_pe, g_grid):
    xo = x.clone().requires_grad_(True)
    ob, gr = tr.oneblob_forward(xo, n_bins), tr.hashgrid_forward(xo, tab, meta)
    (d_pe,) = torch.autograd.grad(ob, xo, g_pe, retain_graph=True)
    (d_grid,) = torch.autograd.grad(gr, xo, g_grid)
    return ob.detach(), gr.detach(), d_pe, d_grid


def _oracle_saturation_allowance(x, n_bins, g_pe):
    """A defect of the ORACLE's derivative alone, which no kernel has (they evaluate the pdf, not a mask).  Autograd differentiates
    clamp(r, 0, 1) with the mask 0 <= r <= 1 on the fp32 r: towards the support's edge the cdf approaches saturation like
    1.25 (1 - |u|)^3, and once that is below r's own rounding error -- K 2^-24 a(u) with the polynomial's six roundings and
    a(1) = 2.25 -- r may round past 0 or 1 inside the support, where the mask then drops the evaluation's pdf entirely, or onto
    exactly 0 or 1 just outside it, where the (inclusive) mask lets the polynomial's slope 15/16 n (1 - u^2)^2 through although the
    pdf is zero.  Allowed: that slope, for every evaluation with 1.25 |1 - |u||^3 <= 6 * 2.25 * 2^-24, times the gradients of the two
    bins that share the edge."""
    P, D = x.shape
    u, _ = er._ob_args(x, n_bins)
    near = 1.25 * (1.0 - u.abs()).abs() ** 3 <= 6 * 2.25 * U
    drop = torch.where(near, (15.0 / 16.0) * n_bins * (1 - u * u) ** 2, torch.zeros_like(u)).sum(-1)   # [P, D, n] per left edge b
    g = g_pe.double().abs().reshape(P, D, n_bins)
    return (drop * (g + torch.roll(g, 1, -1))).sum(-1)


@pytest.mark.parametrize("kind", ["uniform", "spread"])
@pytest.mark.parametrize("grid", list(er.GRIDS))
@pytest.mark.parametrize("name", er.INPUTS)
def test_reference_contains_the_float32_oracle(name, grid, kind):
    meta = er.meta_of(grid)
    n_bins = er.N_BINS[(er.INPUTS.index(name) + list(er.GRIDS).index(grid)) % len(er.N_BINS)]
    x = er.points(name, grid)[1]
    gkind = "spread" if kind == "spread" else "randn"
    g_pe, g_grid = er.grad_cols(er.grads(x.shape[0], gkind), n_bins, meta.n_levels)
    ob, gr, d_pe, d_grid = _oracle(x, er.table(grid, kind), meta, n_bins, g_pe, g_grid)
    y, Ay, _, _ = er.grid_reference(name, grid, kind)
    r_y = er.worst_ratio(gr, y, er.K_Y * U * Ay + TINY)[0]
    yo, Ao = er.oneblob_reference(name, grid, n_bins)
    r_ob = er.worst_ratio(ob, yo, er.K_OB * U * Ao + TINY)[0]
    r_dg = er.worst_ratio(d_grid, *er.dx_reference(name, grid, n_bins, kind, gkind, pe=False))[0]
    dp, tol_p = er.dx_reference(name, grid, n_bins, kind, gkind, grd=False)
    r_dp = er.worst_ratio(d_pe, dp, tol_p + _oracle_saturation_allowance(x, n_bins, g_pe))[0]
    print(f"{name} {grid} {kind} n_bins {n_bins}: worst ratios features {r_y:.3f}, OneBlob {r_ob:.3f}, d_x grid {r_dg:.3f}, d_x OneBlob {r_dp:.3f}")
    assert max(r_y, r_ob, r_dg, r_dp) <= 1.0
    if kind == "spread" and x.shape[0] >= 257:
        canc = float((Ay / y.abs().clamp_min(1e-300)).max())
        print(f"largest A / |y| {canc:.3g}")
        assert canc > 100.0                                              # what the spread table is for: A >> |y| somewhere


# ----------------------------------------------------------------------------- mutants: wrong encoders in float32
def _cells(x, lvl, fused_pos):
    s = torch.tensor(lvl.scale)
    pos = (x.double() * s.double() + 0.5).float() if fused_pos else x * s + 0.5
    fl = torch.floor(pos)
    g = fl.to(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return g, pos - fl


def _emu_grid(x, tab, meta, fused_pos=False, swap_yz=False, no_scale_level=None, dy_for_dx=False):
    """The kernel's grid_level in float32 torch, with the named defect -> features [P, 2 L], Jacobian [L, 3, P, 2]."""
    P, L = x.shape[0], meta.n_levels
    ys, J = [], torch.zeros(L, 3, P, 2)
    for l, lvl in enumerate(meta.levels):
        g, f = _cells(x, lvl, fused_pos)
        v = []
        for c in range(8):
            idx = tr.grid_index((g[:, 0] + (c & 1)) & 0xFFFFFFFF, (g[:, 1] + ((c >> 1) & 1)) & 0xFFFFFFFF,
                                (g[:, 2] + ((c >> 2) & 1)) & 0xFFFFFFFF, lvl) + lvl.offset
            v.append(tab[idx])
        W = [(1.0 - f[:, a], f[:, a]) for a in range(3)]
        acc = torch.zeros(P, 2)
        for c in range(8):
            by, bz = ((c >> 2) & 1, (c >> 1) & 1) if swap_yz else ((c >> 1) & 1, (c >> 2) & 1)
            acc = acc + (W[0][c & 1] * W[1][by] * W[2][bz])[:, None] * v[c]
        ys.append(acc)
        for a in range(3):
            o1, o2 = [k for k in range(3) if k != a]
            pa = 1 if (dy_for_dx and a == 0) else a                     # the axis whose corner pairs are differenced
            los = [c for c in range(8) if not (c >> pa) & 1]
            ja = torch.zeros(P, 2)
            for n, (i, j) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                lo = ((i << o1) | (j << o2)) if pa == a else los[n]
                ja = ja + (W[o1][i] * W[o2][j])[:, None] * (v[lo | (1 << pa)] - v[lo])
            J[l, a] = ja if no_scale_level == l else torch.tensor(lvl.scale) * ja
    return torch.cat(ys, -1), J


def _emu_oneblob(x, n_bins, wrap=True, window=None):
    """kernel_one_blob as the kernels spell it, in float32 torch.  window = w: only the 2 w + 1 bins around floor(x n + s n) of each
    image and the last bin are evaluated, the others are zero (the kernels' window form has w = 2)."""
    n = torch.tensor(float(n_bins))

    def cdf(v):
        u = v * n
        u2 = u * u
        u4 = u2 * u2
        return torch.clamp((15.0 / 16.0) * u * (1.0 - (2.0 / 3.0) * u2 + (1.0 / 5.0) * u4) + 0.5, 0.0, 1.0)
    b = torch.arange(n_bins, dtype=torch.float32) / n
    d = b[None, None, :] - x[:, :, None]
    G = cdf(d) + cdf(d - 1.0) + cdf(d + 1.0)
    y = torch.cat((G[..., 1:], G[..., :1] + (1.0 if wrap else 0.0)), -1) - G
    if window is not None:
        j = torch.arange(n_bins)[None, None, :]
        live = j == n_bins - 1
        for s in (-1.0, 0.0, 1.0):
            k = torch.floor(x * n + s * n).to(torch.int64)[:, :, None]
            live = live | ((j >= k - window) & (j <= k + window))
        y = torch.where(live, y, torch.zeros_like(y))
    return y.reshape(x.shape[0], -1)


@pytest.fixture(scope="module")
def edges():
    grid = "16_592"
    return grid, er.meta_of(grid), er.points("edges", grid)[1], er.table(grid)


def _rejects(got, exp, tol):
    r, i = er.worst_ratio(got, exp, tol)
    n_over = int((((got.double() - exp).abs() > tol) & torch.isfinite(exp)).sum())
    print(f"worst ratio {r:.3g} at {i}; {n_over} entries over the bound")
    return r > 1.0


def test_the_emulation_without_a_defect_is_accepted(edges):
    """(or the rejections below would prove nothing)"""
    grid, meta, x, tab = edges
    y, Ay, J, AJ = er.grid_reference("edges", grid)
    ey, eJ = _emu_grid(x, tab, meta)
    assert not _rejects(ey, y, er.K_Y * U * Ay + TINY)
    assert not _rejects(eJ, J, er.K_J * U * AJ + TINY)
    for n_bins in er.N_BINS:
        yo, Ao = er.oneblob_reference("edges", grid, n_bins)
        assert not _rejects(_emu_oneblob(x, n_bins), yo, er.K_OB * U * Ao + TINY)
        if n_bins >= 8:
            m = (x.abs() < 4.0).all(-1)                                   # where the kernels use the window form
            assert not _rejects(_emu_oneblob(x, n_bins, window=2)[m], yo[m], (er.K_OB * U * Ao + TINY)[m])


def test_mutant_pos_in_one_rounding(edges):
    grid, meta, x, tab = edges
    y, Ay, J, AJ = er.grid_reference("edges", grid)
    ey, eJ = _emu_grid(x, tab, meta, fused_pos=True)
    assert _rejects(ey, y, er.K_Y * U * Ay + TINY)                      # the fraction is off by up to half an ulp of pos
    assert _rejects(eJ, J, er.K_J * U * AJ + TINY)                      # and at a face the cell itself


def test_mutant_y_and_z_corner_bits_exchanged(edges):
    grid, meta, x, tab = edges
    y, Ay, _, _ = er.grid_reference("edges", grid)
    assert _rejects(_emu_grid(x, tab, meta, swap_yz=True)[0], y, er.K_Y * U * Ay + TINY)


def test_mutant_one_level_without_its_scale(edges):
    grid, meta, x, tab = edges
    _, _, J, AJ = er.grid_reference("edges", grid)
    for l in (0, meta.n_levels - 1):
        eJ = _emu_grid(x, tab, meta, no_scale_level=l)[1]
        assert _rejects(eJ, J, er.K_J * U * AJ + TINY)
        g_grid = er.grad_cols(er.grads(x.shape[0]), 16, meta.n_levels)[1]
        dx = (eJ * g_grid.reshape(-1, meta.n_levels, 2).permute(1, 0, 2)[:, None]).sum((0, 3)).T
        assert _rejects(dx, *er.dx_reference("edges", grid, 16, pe=False))


def test_mutant_axis_pairing_of_dy_taken_for_dx(edges):
    grid, meta, x, tab = edges
    _, _, J, AJ = er.grid_reference("edges", grid)
    eJ = _emu_grid(x, tab, meta, dy_for_dx=True)[1]
    assert _rejects(eJ[:, 0], J[:, 0], (er.K_J * U * AJ + TINY)[:, 0])
    assert not _rejects(eJ[:, 1:], J[:, 1:], (er.K_J * U * AJ + TINY)[:, 1:])


@pytest.mark.parametrize("n_bins", er.N_BINS)
def test_mutant_last_bin_without_its_wrap(edges, n_bins):
    grid, _, x, _ = edges
    yo, Ao = er.oneblob_reference("edges", grid, n_bins)
    assert _rejects(_emu_oneblob(x, n_bins, wrap=False), yo, er.K_OB * U * Ao + TINY)


def test_mutant_d_x_not_divided_by_the_extent():
    grid = "16_592"
    for pe, grd in ((True, True), (True, False), (False, True)):
        plain, _ = er.dx_reference("world", grid, 16, pe=pe, grd=grd, bound=False)
        assert _rejects(plain.float(), *er.dx_reference("world", grid, 16, pe=pe, grd=grd, bound=True))


@pytest.mark.parametrize("n_bins", [16, 8, 12])
def test_mutant_window_without_its_margin(edges, n_bins):
    """The window form evaluates the five bins around floor(x n): the quartic's support (one bin to each side of x) can reach three
    of them, the outer two are margin against the rounding of x n.  What the margin buys is BITS, not accuracy: with three bins the
    only loss is a sliver of the support that rounding pushed across a bin edge, worth at most one rounding of the bin itself
    (asserted: <= 2^-24 from the all-edges form, and inside the bound) -- no bound made of the arithmetic's own roundings can see
    that, and it is the bit comparison of the five-bin form with the all-edges loop (above, and tools/encode_digest.py between
    trees) that holds the margin.  The mutant the bound must reject is the window with no room beyond the bin that holds x: it
    drops the neighbours the quartic reaches into."""
    grid, _, x, _ = edges
    yo, Ao = er.oneblob_reference("edges", grid, n_bins)
    m = (x.abs() < 4.0).all(-1)
    tol = (er.K_OB * U * Ao + TINY)[m]
    full = _emu_oneblob(x, n_bins)[m]
    assert torch.equal(_emu_oneblob(x, n_bins, window=2)[m], full)
    three = _emu_oneblob(x, n_bins, window=1)[m]
    assert float((three - full).abs().max()) <= U and not _rejects(three, yo[m], tol)
    assert _rejects(_emu_oneblob(x, n_bins, window=0)[m], yo[m], tol)
