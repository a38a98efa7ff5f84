"""Float64 reference of the point encoder (csrc/encode.hip, csrc/dev_encode.hpp): fp64 normalisation, tcnn's kernel_one_blob and the
multi-resolution hash grid -- forward values, the per-level Jacobian the forward keeps as dy_dx, and the input gradient d_x -- with
the seeded, NAMED inputs the encoder tests feed it and the rounding counts their bounds are made of.  CPU only
(tests/test_encode_ref.py holds it to a plain loop, to a central difference and to the float32 oracle, and shows that the bounds
reject seven wrong encoders; tests/test_gpu_encode.py holds every form of the kernels to it).

What is exact input and what is float64.  Cell and fraction of a point on a level are the shared fp32 contract
(oracle/tcnn_ref.hashgrid_indices: pos = x * scale + 0.5 in two roundings, then floor) and are taken as given; everything after them
-- 1 - f, the corner weights, every product and sum -- is float64.  OneBlob is evaluated in float64 from the fp32 coordinate; its
clamp keeps a NaN (torch.clamp), and a non-finite coordinate gives a NaN derivative.

Beside every quantity stands its TERM-WISE ABSOLUTE SUM A (the same expression with |.| on every product), and a kernel's element is
held to  |got - exp| <= k 2^-24 A + TINY.  k is the number of fp32 roundings on the longest chain of dependent operations from the
inputs (fraction, table value, upstream gradient, coordinate) to the element, counted from the source text of dev_encode.hpp and
encode.hip, never from a result (operands rounded in parallel -- the three 1 - f of corner 0 -- sit on chains of their own; counting
them as well would give 13 for the features, the test holds the smaller figure):

  K_Y  = 11      features: 1 - f (1), two weight products (2), times the table value (1), seven additions (the first of the eight
                 terms joins 0 exactly and then passes seven sums)
  K_J  = 7       Jacobian: 1 - f (1), the product of two weights (1), times the corner difference (1; the difference itself is on
                 a shorter chain), three additions, times the level's scale (1)
  K_DX_SAVED(L)    = K_J + 2 + L = 9 + L    j.x g0 (1) + j.y g1 (1), then the level's sum joins dx and passes up to L such additions
  K_DX_REGATHER(L) = 8 + L    dot = v.x g0 + v.y g1 (2), corner difference (1), times the weight (1), three additions (3), times
                 the scale (1), L additions into dx
  K_OB = 14      OneBlob bin: u = ((b / n - x) -+ 1) n (4), the quintic in Horner-free form u2, u4, u4 / 5, the sum, the product,
                 + 0.5 (6), the sum of the three images (2), the wrap's + 1 (1), right - left (1)
  K_OB_DX(n, L) = 4 + 4 + 2 + 1 + 1 + max(n - 1, 10) + L    u (4), u2, 1 - u2 and two products (4), three images (2), right - left
                 (1), times the upstream gradient (1), the bins' accumulation (all n of them in the all-edges loop, at most two
                 five-bin windows and the last bin in the window form: the first joins 0 exactly), then the L level sums of a joint
                 row; with a bound every d_x count grows by 1 (the division is float64, its result rounded once)

OneBlob's A is a condition number, not only a sum: the argument u = (b/n - x + s) n is a difference of fp32 values, so its error is
K_U 2^-24 M with M = n (|b/n| + |x| + |s|), and it reaches the bin through the kernel's slope.  Per kernel evaluation
A = a(u) + M (|f'(u)| + max|f''| K_U 2^-24 M), a(u) the polynomial's own absolute sum (15/16 |u| (1 + 2/3 u^2 + 1/5 u^4) + 1/2 for
the cdf, 15/16 n (1 + u^2)^2 for the pdf) inside the support and a hair outside it (|u| <= 1.001: fp32 may land on the other side of
the support's edge), the saturated value elsewhere.

TINY = 2^-126 (the smallest normal float): a result that fp32 would hold as a subnormal, flushed or not.
"""
import math

import numpy as np
import torch

from oracle import tcnn_ref as tr

U = 2.0 ** -24
TINY = 2.0 ** -126
K_Y, K_J, K_U, K_OB = 11, 7, 4, 14
BOUND = ((-1.5, 2.0), (-0.5, 1.75), (0.25, 4.0))          # asymmetric, as in tools/encode_digest.py
GRIDS = {"16_592": (16, 592, 16), "12_64": (12, 64, 16), "14_128_L4": (14, 128, 4)}   # (log2 T, finest resolution, levels)
N_BINS = (16, 8, 12, 5, 4)
P_NAMES = ("P1", "P127", "P128", "P129")
INPUTS = ("edges", "world") + P_NAMES
G_WIDTH = 3 * 16 + 2 * 16                                  # upstream gradients are drawn this wide and sliced


def k_dx_saved(L):
    return K_J + 2 + L


def k_dx_regather(L):
    return 8 + L


def k_ob_dx(n_bins, L):
    return 4 + 4 + 2 + 1 + 1 + max(n_bins - 1, 10) + L


_META, _POINTS, _TABLE, _GRAD, _REF = {}, {}, {}, {}, {}


def meta_of(grid: str) -> tr.GridMeta:
    if grid not in _META:
        hs, res, L = GRIDS[grid]
        _META[grid] = tr.grid_meta(hs, res, n_levels=L)
    return _META[grid]


# ----------------------------------------------------------------------------- the reference
def normalise(xw: torch.Tensor, bound=BOUND) -> torch.Tensor:
    """load_point: float(((double)v - b0) / (b1 - b0)) per axis."""
    b = torch.tensor(bound, dtype=torch.float64)
    return ((xw.double() - b[:, 0]) / (b[:, 1] - b[:, 0])).float()


def bound_extent(bound=BOUND) -> torch.Tensor:
    b = torch.tensor(bound, dtype=torch.float64)
    return b[:, 1] - b[:, 0]


def interp64(f: torch.Tensor, v: torch.Tensor):
    """Trilinear interpolation y = sum_c w_c v_c and A = sum_c w_c |v_c|: fractions f [P, L, 3], corner values v [P, L, 8, 2]
    (corner c: bit 0 x + 1, bit 1 y + 1, bit 2 z + 1), float64 -> [P, L, 2]."""
    W = torch.stack((1.0 - f, f), -1)
    y = torch.zeros(v.shape[0], v.shape[1], 2, dtype=torch.float64)
    Ay = torch.zeros_like(y)
    for c in range(8):
        w = W[:, :, 0, c & 1] * W[:, :, 1, (c >> 1) & 1] * W[:, :, 2, (c >> 2) & 1]
        y = y + w[..., None] * v[:, :, c]
        Ay = Ay + w.abs()[..., None] * v[:, :, c].abs()
    return y, Ay


def grid64(x: torch.Tensor, table: torch.Tensor, meta: tr.GridMeta):
    """x [P, 3] fp32, table [rows, 2] fp32 -> y, Ay [P, 2 L] and J, AJ [L, 3, P, 2] (the dy_dx layout), float64.  A non-finite
    coordinate has no cell: its fraction is NaN (Inf - Inf in the kernel), its rows are those of coordinate 0 and carry no meaning
    -- only which entries are finite does (an axis' own Jacobian does not depend on its fraction)."""
    fin = torch.isfinite(x)
    rows, fr = tr.hashgrid_indices(torch.where(fin, x, torch.zeros_like(x)), meta)
    f = torch.where(fin[:, None, :], fr.double(), torch.full_like(fr, float("nan"), dtype=torch.float64))   # [P, L, 3]
    W = torch.stack((1.0 - f, f), -1)                                   # [P, L, 3, 2]: weight of bit 0 / 1 per axis
    v = table.double()[rows]                                             # [P, L, 8, 2]
    P, L = x.shape[0], meta.n_levels
    y, Ay = interp64(f, v)
    s = torch.tensor([float(l.scale) for l in meta.levels], dtype=torch.float64)[None, :, None]
    J = torch.zeros(L, 3, P, 2, dtype=torch.float64)
    AJ = torch.zeros_like(J)
    for a in range(3):
        o1, o2 = [k for k in range(3) if k != a]
        ja = torch.zeros(P, L, 2, dtype=torch.float64)
        aa = torch.zeros_like(ja)
        for i in range(2):
            for j in range(2):
                lo = (i << o1) | (j << o2)
                hi = lo | (1 << a)
                w = (W[:, :, o1, i] * W[:, :, o2, j])[..., None]
                ja = ja + w * (v[:, :, hi] - v[:, :, lo])
                aa = aa + w.abs() * (v[:, :, hi].abs() + v[:, :, lo].abs())
        J[:, a] = (s * ja).permute(1, 0, 2)
        AJ[:, a] = (s * aa).permute(1, 0, 2)
    return y.reshape(P, 2 * L), Ay.reshape(P, 2 * L), J, AJ


def grid_dx64(J: torch.Tensor, AJ: torch.Tensor, g: torch.Tensor):
    """d_x = sum_l J_l g_l and its absolute sum: J [L, 3, P, 2], g [P, 2 L] -> [P, 3]."""
    L, _, P, _ = J.shape
    gl = g.double().reshape(P, L, 2).permute(1, 0, 2)[:, None]          # [L, 1, P, 2]
    return (J * gl).sum((0, 3)).T.contiguous(), (AJ * gl.abs()).sum((0, 3)).T.contiguous()


def _ob_args(x: torch.Tensor, n: int):
    """u [P, D, n, 3] of the three images at the n left bin edges, and the magnitude M of what u was formed from."""
    xd = x.double()[:, :, None, None]
    b = (torch.arange(n, dtype=torch.float64) / n)[None, None, :, None]
    sh = torch.tensor([0.0, -1.0, 1.0], dtype=torch.float64)[None, None, None, :]
    u = (b - xd + sh) * n
    M = n * (b.abs() + xd.abs() + sh.abs())
    return u, torch.where(torch.isfinite(M), M, torch.zeros_like(M))


def _cdf(u):
    u2 = u * u
    return torch.clamp((15.0 / 16.0) * u * (1 - (2.0 / 3.0) * u2 + (1.0 / 5.0) * u2 * u2) + 0.5, 0.0, 1.0)   # keeps a NaN


def _pdf(u, n):
    u2 = u * u
    p = torch.where(u2 > 1.0, torch.zeros_like(u), (15.0 / 16.0) * n * (1 - u2) ** 2)
    return torch.where(torch.isfinite(u), p, torch.full_like(u, float("nan")))


def _cond(u, M, n, pdf: bool):
    """a(u) + M (|f'(u)| + max|f''| K_U 2^-24 M) per kernel evaluation (module docstring)."""
    near = u.abs() <= 1.001
    uh = u.abs().clamp(max=1.0)
    inside = (u.abs() < 1.0).double()
    if pdf:
        a = torch.where(near, (15.0 / 16.0) * n * (1 + uh * uh) ** 2, torch.zeros_like(u))
        slope = (15.0 / 16.0) * n * 4.0 * uh * (1 - uh * uh) * inside
        curv = 7.5 * n
    else:
        sat = (u > 0).double()
        a = torch.where(near, (15.0 / 16.0) * uh * (1 + (2.0 / 3.0) * uh ** 2 + (1.0 / 5.0) * uh ** 4) + 0.5, sat)
        slope = (15.0 / 16.0) * (1 - uh * uh) ** 2 * inside
        curv = 1.4434
    return a + M * (slope + curv * K_U * U * M)


def oneblob64(x: torch.Tensor, n: int):
    """tcnn kernel_one_blob: x [P, D] fp32 -> y, A [P, D n] float64; bin b = G(b + 1) - G(b), G(n) = G(0) + 1."""
    P, D = x.shape
    u, M = _ob_args(x, n)
    G = _cdf(u).sum(-1)
    E = _cond(u, M, n, False).sum(-1)
    y = torch.cat((G[..., 1:], G[..., :1] + 1.0), -1) - G
    A = torch.cat((E[..., 1:], E[..., :1] + 1.0), -1) + E
    return y.reshape(P, D * n), A.reshape(P, D * n)


def oneblob_dx64(x: torch.Tensor, n: int, g: torch.Tensor):
    """d/dx of oneblob64 contracted with g [P, D n] -> d_x, A [P, D]: d bin_b / dx = -(pdfG(b + 1) - pdfG(b)), pdfG(n) = pdfG(0)."""
    P, D = x.shape
    u, M = _ob_args(x, n)
    G = _pdf(u, n).sum(-1)
    E = _cond(u, M, n, True).sum(-1)
    gd = g.double().reshape(P, D, n)
    dx = -(gd * (torch.cat((G[..., 1:], G[..., :1]), -1) - G)).sum(-1)
    A = (gd.abs() * (torch.cat((E[..., 1:], E[..., :1]), -1) + E)).sum(-1)
    return dx, A


# ----------------------------------------------------------------------------- named inputs
def _uniform(P: int, seed: int) -> torch.Tensor:
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(seed)) * 1.2 - 0.1


def _f32(v) -> float:
    return float(np.float32(v))


def _pos(v: float, scale) -> np.float32:
    return np.float32(np.float32(np.float32(v) * np.float32(scale)) + np.float32(0.5))


def integer_pos_coordinate(scale) -> float:
    """The SMALLEST float32 coordinate whose pos = x * scale + 0.5 is exactly the integer k (fraction 0; its lower neighbour lies
    in cell k - 1), searched among the float32 neighbours of (k - 0.5) / scale for a k in the upper half of the level."""
    s = np.float32(scale)
    for k in range(max(int(s) // 2, 1), int(s) + 1):
        c = np.float32((k - 0.5) / float(s))
        for cand in (c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))):
            if float(_pos(cand, s)) == float(k):
                for _ in range(64):                     # (the + 0.5 may absorb a few neighbours into the same integer)
                    prev = np.nextafter(cand, np.float32(-1))
                    if float(_pos(prev, s)) != float(k):
                        return float(cand)
                    cand = prev
    raise AssertionError(f"no float32 coordinate with an integer pos at scale {scale}")


def _edges(meta: tr.GridMeta) -> torch.Tensor:
    P = 257                                             # two workgroups of 128 and a one-row tail
    x = _uniform(P, 41)
    one_up, zero_dn = _f32(np.nextafter(np.float32(1), np.float32(2))), _f32(np.nextafter(np.float32(0), np.float32(-1)))
    below4 = _f32(np.nextafter(np.float32(4), np.float32(0)))
    same = [0.0, 1.0, 0.5, one_up, zero_dn]             # rows with the value on all three axes
    single = []                                         # values dealt three to a row
    for lvl in meta.levels:
        v = integer_pos_coordinate(lvl.scale)
        lo, hi = _f32(np.nextafter(np.float32(v), np.float32(-1))), _f32(np.nextafter(np.float32(v), np.float32(2)))
        k = float(_pos(v, lvl.scale))
        assert k == math.floor(k)                                                            # fraction exactly 0
        assert math.floor(float(_pos(lo, lvl.scale))) == k - 1 and math.floor(float(_pos(hi, lvl.scale))) == k   # the cell changes at v
        same.append(v)
        single += [v, lo, hi]
        if not lvl.hashed:
            single.append(_f32(np.float32(-0.5) / lvl.scale))
    for n in N_BINS:                                    # every bin edge k / n as the kernel forms it, both sides of the interval
        single += [_f32(np.float32(k) / np.float32(n)) for k in range(-n, 2 * n + 1)]
    single += [below4, -below4, 4.0, -4.0, 4.25, -4.5, 4.75, 5.0, -5.0]
    assert below4 < 4.0 and all(4.0 <= abs(v) <= 5.0 for v in single[-7:])
    single = list(dict.fromkeys(single))
    single += [0.25] * (-len(single) % 3)
    hand = [(v, v, v) for v in same] + [tuple(single[i:i + 3]) for i in range(0, len(single), 3)]
    hand += [(-0.05, 0.01, 0.01), (0.31, 0.62, -0.05), (-0.07, -0.06, -0.05)]
    assert len(hand) < P - 64, len(hand)                # a fair share of the rows stays uniform
    x[:len(hand)] = torch.tensor(hand, dtype=torch.float32)
    rows, fr = tr.hashgrid_indices(x, meta)
    for l, lvl in enumerate(meta.levels):               # every level sees a fraction of exactly 0 on one axis and on all three
        assert bool((fr[:, l] == 0).any()) and bool((fr[:, l] == 0).all(-1).any()), l
        pos = x[len(hand) - 3:len(hand)] * torch.tensor(lvl.scale) + 0.5
        cell = torch.floor(pos).to(torch.int32).to(torch.int64) & 0xFFFFFFFF
        assert bool((cell[0, 0] >= 2 ** 31) and (cell[1, 2] >= 2 ** 31) and (cell[2] >= 2 ** 31).all())   # wraps through uint32
    assert int(rows.min()) >= 0 and int(rows.max()) < meta.total_rows
    return x


def _world(x: torch.Tensor) -> torch.Tensor:
    b = torch.tensor(BOUND, dtype=torch.float64)
    xw = (b[:, 0] + x.double() * (b[:, 1] - b[:, 0])).float()
    assert not torch.equal(normalise(xw), x)            # non-trivial: the normalisation does not simply undo the map
    return xw


def points(name: str, grid: str):
    """-> (src, x): what the encoder is given (world points for `world`, else x itself) and the fp32 normalised coordinates."""
    key = (name, grid if name in ("edges", "world") else None)
    if key not in _POINTS:
        if name == "edges":
            x = _edges(meta_of(grid))
            _POINTS[key] = (x, x)
        elif name == "world":
            xw = _world(points("edges", grid)[1])
            _POINTS[key] = (xw, normalise(xw))
        else:
            P = int(name[1:])
            x = _uniform(P, 50 + P)
            assert x.shape[0] == P and float(x.min()) >= -0.1 and float(x.max()) < 1.1
            _POINTS[key] = (x, x)
    return _POINTS[key]


def table(grid: str, kind: str = "uniform") -> torch.Tensor:
    """[rows, 2] fp32: uniform in [-1, 1), or `spread` -- magnitudes 10^[-6, 3] with random signs (sums that cancel: A >> |y|)."""
    key = (grid, kind)
    if key not in _TABLE:
        g = torch.Generator().manual_seed(1 if kind == "uniform" else 2)
        t = torch.rand(meta_of(grid).total_rows, 2, generator=g) * 2 - 1
        if kind == "spread":
            t = torch.sign(t) * 10.0 ** (torch.rand(t.shape, generator=g) * 9.0 - 6.0)
            assert float(t.abs().max()) > 100.0 and float(t.abs().min()) < 1e-5
        _TABLE[key] = t
    return _TABLE[key]


def grads(P: int, kind: str = "randn") -> torch.Tensor:
    """Upstream gradient [P, G_WIDTH] fp32: OneBlob columns are [:, :3 n], grid columns [:, 48:48 + 2 L]."""
    key = (P, kind)
    if key not in _GRAD:
        g = torch.Generator().manual_seed(60 + P + (1000 if kind == "spread" else 0))
        t = torch.randn(P, G_WIDTH, generator=g)
        if kind == "spread":
            t = t * 10.0 ** (torch.rand(P, 1, generator=g) * 9.0 - 6.0)
        _GRAD[key] = t
    return _GRAD[key]


def grad_cols(g: torch.Tensor, n_bins: int, L: int):
    return g[:, :3 * n_bins].contiguous(), g[:, 48:48 + 2 * L].contiguous()


# ----------------------------------------------------------------------------- cached references and bounds
def grid_reference(name: str, grid: str, kind: str = "uniform"):
    key = ("grid", name, grid, kind)
    if key not in _REF:
        _REF[key] = grid64(points(name, grid)[1], table(grid, kind), meta_of(grid))
    return _REF[key]


def oneblob_reference(name: str, grid: str, n_bins: int):
    key = ("ob", name, grid if name in ("edges", "world") else None, n_bins)
    if key not in _REF:
        _REF[key] = oneblob64(points(name, grid)[1], n_bins)
    return _REF[key]


def dx_reference(name: str, grid: str, n_bins: int, kind: str = "uniform", gkind: str = "randn", pe: bool = True, grd: bool = True,
                 bound: bool = False, saved: bool = True):
    """-> (d_x, tol) [P, 3] float64 of a form of the backward: OneBlob columns (pe), grid columns (grd), divided by the bound's
    extent (bound); the tolerance is made of the counts of the module docstring."""
    x = points(name, grid)[1]
    L = meta_of(grid).n_levels if grd else 0
    g_pe, g_grid = grad_cols(grads(x.shape[0], gkind), n_bins, meta_of(grid).n_levels)
    dx = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    tol = torch.zeros_like(dx)
    extra = 1 if bound else 0
    if pe:
        d, A = oneblob_dx64(x, n_bins, g_pe)
        dx, tol = dx + d, tol + (k_ob_dx(n_bins, L) + extra) * U * A
    if grd:
        _, _, J, AJ = grid_reference(name, grid, kind)
        d, A = grid_dx64(J, AJ, g_grid)
        dx, tol = dx + d, tol + ((k_dx_saved(L) if saved else k_dx_regather(L)) + extra) * U * A
    if bound:
        dx, tol = dx / bound_extent(), tol / bound_extent()
    return dx, tol + TINY


def worst_ratio(got: torch.Tensor, exp: torch.Tensor, tol: torch.Tensor):
    """max |got - exp| / tol over the entries whose reference is finite -> (ratio, flat index); an entry that equals its
    reference counts 0 whatever its tolerance."""
    got, exp, tol = got.detach().double().cpu(), exp.double(), tol.double()
    m = torch.isfinite(exp) & torch.isfinite(tol)
    d = torch.where(m, (got - exp).abs(), torch.zeros_like(exp))
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)          # a NaN where the reference is finite
    r = torch.where(d == 0, torch.zeros_like(d), d / tol.clamp_min(1e-300)).reshape(-1)
    if r.numel() == 0:
        return 0.0, 0
    i = int(torch.argmax(r))
    return float(r[i]), i
