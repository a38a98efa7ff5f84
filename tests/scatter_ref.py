"""Float64 reference of the hash-grid table-gradient scatter (tcnn kernel_grid_backward's d_table) and the seeded, RAY-SHAPED inputs
the scatter tests feed it: runs of consecutive samples in one coarse cell, points outside the unit cube, mostly-zero and widely
spread gradients, point counts around the kernels' tile sizes.  CPU only (tests/test_scatter_ref.py holds it to a plain per-corner
loop; tests/test_gpu_scatter.py holds every scatter form of csrc/scatter.hip to it).

The reference is oracle/tcnn_ref.hashgrid_forward with a float64 table leaf: the corner weights are the fp32 products the kernels
form, every weight * gradient product and every sum is float64.
"""
import numpy as np
import torch

from oracle import tcnn_ref as tr

N_FEAT = 32                      # 16 levels x 2 features
P_EDGES = (1, 255, 256, 257, 511, 513, 1023, 1025, 2047, 2049)   # transpose tile 256 x DG_TILES, sweep workgroup 1024, list tile 256 x 8

_META, _INPUT, _REF = {}, {}, {}


def meta_of(hash_size: int, res: int) -> tr.GridMeta:
    key = (hash_size, res)
    if key not in _META:
        _META[key] = tr.grid_meta(hash_size, res)
    return _META[key]


def _ray_points(P: int, seed: int) -> torch.Tensor:
    """ceil(P / 64) rays x 64 samples through the middle of the cube, in ray order (consecutive points = consecutive samples), the
    first P of them; every point inside [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    n = (P + 63) // 64
    o = torch.rand(n, 1, 3, generator=g) * 0.3 + 0.35
    d = torch.randn(n, 1, 3, generator=g) * 0.3
    t = torch.linspace(0, 1, 64)[None, :, None]
    return (o + d * t).reshape(-1, 3).clamp(0, 1)[:P].contiguous()


def _grad(P: int, seed: int) -> torch.Tensor:
    return torch.randn(P, N_FEAT, generator=torch.Generator().manual_seed(seed))


def _build(name: str, meta: tr.GridMeta):
    if name == "rays":
        return _ray_points(4096, 21), _grad(4096, 22)
    if name == "one_cell":                          # level-0 cell (7, 7, 7): pos = 15 x + 0.5 in [7, 8)
        g = torch.Generator().manual_seed(23)
        x = (6.5 + 0.02 + 0.96 * torch.rand(3000, 3, generator=g)) / 15.0
        return x, _grad(3000, 24)
    if name == "one_point":
        x = torch.tensor([0.4567, 0.4321, 0.4789]).expand(3000, 3).contiguous()
        return x, _grad(3000, 25)
    if name == "out_of_box":
        g = torch.Generator().manual_seed(26)
        x = torch.rand(4096, 3, generator=g) * 1.2 - 0.1
        one_up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
        hand = [(-0.05, 0.01, 0.01),                # level-0 cell (-1, 0, 0): the dense corner sum is 0xffffffff
                (0.31, 0.62, -0.05),                # negative on z only: the corner sum lands just below 2^32
                (-0.07, -0.06, -0.05),              # negative on all three axes
                (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.5), (one_up, one_up, one_up), (one_up, 0.5, 0.25)]
        for lvl in meta.levels:
            if not lvl.hashed:                      # exactly half a cell below the box: pos = x * scale + 0.5 rounds at 0
                v = float(np.float32(-0.5) / lvl.scale)
                hand += [(v, v, v), (v, 0.5, 0.5), (0.5, 0.5, v)]
        x[:len(hand)] = torch.tensor(hand, dtype=torch.float32)
        return x, _grad(4096, 27)
    if name == "sparse":                            # nine gradient rows in ten exactly zero: those points enter no bin, queue or list
        x, gy = _build("rays", meta)
        keep = torch.rand(gy.shape[0], generator=torch.Generator().manual_seed(28)) < 0.1
        return x, gy * keep[:, None]
    if name == "sparse_one":
        x, gy = _build("rays", meta)
        out = torch.zeros_like(gy)
        out[2077] = gy[2077]
        return x, out
    if name == "spread":                            # rows of very different magnitude: the fixed-point bins' quantum follows the largest
        x, gy = _build("rays", meta)
        e = torch.rand(gy.shape[0], 1, generator=torch.Generator().manual_seed(29)) * 9.0 - 6.0
        return x, (gy * 10.0 ** e).contiguous()
    if name.startswith("P"):
        P = int(name[1:])
        return _ray_points(P, 30 + P), _grad(P, 31 + P)
    raise KeyError(name)


INPUTS = ("rays", "one_cell", "one_point", "out_of_box", "sparse", "sparse_one", "spread") + tuple(f"P{p}" for p in P_EDGES)


def inputs(name: str, hash_size: int, res: int):
    """(x [P, 3], g [P, 32]) fp32 on the CPU, built once per session (out_of_box depends on the grid's dense levels)."""
    key = (hash_size, res, name) if name == "out_of_box" else name
    if key not in _INPUT:
        _INPUT[key] = _build(name, meta_of(hash_size, res))
    return _INPUT[key]


def table_gradient64(x: torch.Tensor, g: torch.Tensor, meta: tr.GridMeta):
    """-> (exp, A, n), each [total_rows, 2] float64: the scatter-add of (fp32 corner weight) x g, the same with |g|, and the number
    of non-zero contributions (non-zero weight, non-zero gradient) per table entry."""
    leaf = torch.zeros(meta.total_rows, meta.n_features, dtype=torch.float64, requires_grad=True)
    y = tr.hashgrid_forward(x, leaf, meta)
    exp = torch.autograd.grad(y, leaf, g, retain_graph=True)[0]
    A = torch.autograd.grad(y, leaf, g.abs())[0]
    rows, fr = tr.hashgrid_indices(x, meta)
    n = torch.zeros(meta.total_rows, meta.n_features, dtype=torch.float64)
    for l in range(meta.n_levels):
        f = fr[:, l]
        nzg = (g[:, 2 * l:2 * l + 2] != 0)
        for c in range(8):
            w = (f[:, 0] if c & 1 else 1 - f[:, 0]) * (f[:, 1] if c & 2 else 1 - f[:, 1]) * (f[:, 2] if c & 4 else 1 - f[:, 2])
            n.index_add_(0, rows[:, l, c], ((w != 0)[:, None] & nzg).double())
    return exp, A, n


def reference(name: str, hash_size: int, res: int):
    """table_gradient64 of a named input on a grid, computed once per session."""
    key = (hash_size, res, name)
    if key not in _REF:
        x, g = inputs(name, hash_size, res)
        _REF[key] = table_gradient64(x, g, meta_of(hash_size, res))
    return _REF[key]
