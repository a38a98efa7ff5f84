"""Every form of the hash-grid table-gradient scatter (csrc/scatter.hip, the per-corner atomics of csrc/encode.hip) against the float64
reference of tests/scatter_ref.py, entry by entry, on ray-shaped inputs: runs of samples in one coarse cell (the run-combining
sweep's register accumulators and flushes), points outside the unit cube (rows that wrap), mostly-zero and widely spread gradients,
point counts around the tile sizes.

Bound per table entry:  |got - exp| <= 1e-5 |exp| + c A + 1e-10 max|exp|,  A = the same scatter with |g| upstream.
  c = 1e-6 where the sums go through 64-bit bins (float64 or fixed point): the scatter-only bound tests/test_gpu_fullsize.py states;
  c = 1e-6 + n 2^-24 where contributions reach d_table as fp32 atomics (the ATOMIC form, the overflow fallback of 64-entry queues
      and lists): recursive fp32 summation of the entry's n contributions, n from the reference;
  for the `spread` input the last term is n 2^-39 max|g|: the fixed-point quantum of the queue and list bins per contribution.
"""
import pytest
import torch

import scatter_ref as sref
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from dns_slam_amd import ops
    return ops


def _form(ops, name):
    return {"auto": (ops.SCATTER_AUTO, 0), "binned": (ops.SCATTER_BINNED, 0), "queues": (ops.SCATTER_QUEUES, 0),
            "lists": (ops.SCATTER_AUTO | ops.SCATTER_LISTS, 0), "atomic": (ops.SCATTER_ATOMIC, 0),
            "replay": (ops.SCATTER_AUTO | ops.SCATTER_REPLAY, 0), "queues64": (ops.SCATTER_QUEUES, 64),
            "lists64": (ops.SCATTER_AUTO | ops.SCATTER_LISTS, 64)}[name]


FP32_ATOMICS = ("atomic", "queues64", "lists64")

_TABLES = {}


def _table(ops, hash_size, res):
    key = (hash_size, res)
    if key not in _TABLES:
        pm = ops.GridMeta(hash_size, res)
        t = torch.rand(pm.total_rows * 2, generator=torch.Generator().manual_seed(1)) * 2 - 1
        _TABLES[key] = (pm, t.to(DEV))
    return _TABLES[key]


def _run(name, form, hash_size, res, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "SCATTER_FORM", _form(ops, form))
    pm, table = _table(ops, hash_size, res)
    assert pm.total_rows == sref.meta_of(hash_size, res).total_rows
    x, g = sref.inputs(name, hash_size, res)
    t = table.clone().requires_grad_(True)
    ops.encode(x.to(DEV), t, pm, None, 16, False, True).backward(g.to(DEV))
    got = t.grad.reshape(-1, 2).cpu().double()
    exp, A, n = sref.reference(name, hash_size, res)
    c = 1e-6 + (n * 2.0 ** -24 if form in FP32_ATOMICS else 0.0)
    last = n * 2.0 ** -39 * float(g.abs().max()) if name == "spread" else 1e-10 * float(exp.abs().max())
    tol = 1e-5 * exp.abs() + c * A + last
    d = (got - exp).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / tol.clamp_min(1e-300))
    i = int(torch.argmax(ratio))
    worst = float(ratio.reshape(-1)[i])
    what = f"scatter64 grid ({hash_size}, {res}) {name} {form}"
    REPORT.append((what, float(d.max() / exp.abs().max()), worst, 1e-5))
    print(f"{what}: worst ratio {worst:.3f} at entry {i // 2} (got {float(got.reshape(-1)[i]):.9e}, want {float(exp.reshape(-1)[i]):.9e}, "
          f"tol {float(tol.reshape(-1)[i]):.3e}, n {int(n.reshape(-1)[i])}); entries over the bound: {int((ratio > 1).sum())}")
    assert bool(torch.isfinite(got).all()), what
    assert worst <= 1.0, f"{what}: worst ratio {worst:.2f}, {int((ratio > 1).sum())} entries over the bound"
    stray = (got != 0) & (n == 0)
    assert not bool(stray.any()), f"{what}: {int(stray.sum())} entries without a contribution are not zero"
    return got, exp, n


@pytest.mark.parametrize("form", ["auto", "binned", "queues", "lists", "atomic", "replay", "queues64", "lists64"])
@pytest.mark.parametrize("name", sref.INPUTS)
def test_scatter_16_592(name, form, monkeypatch):
    """T = 2^16: one dense level of one chunk, three of 2, 3 and 5 chunks (the run-combining sweep in AUTO, BINNED, LISTS and
    REPLAY), twelve hashed levels of 8 chunks."""
    got, exp, n = _run(name, form, 16, 592, monkeypatch)
    if name == "sparse_one":                        # one point: exactly its entries, each with its one contribution
        assert torch.equal(got != 0, (n > 0) & (exp.float() != 0))


@pytest.mark.parametrize("form", ["auto", "binned", "queues", "lists"])
@pytest.mark.parametrize("name", ["rays", "out_of_box", "sparse"])
def test_scatter_20_231(name, form, monkeypatch):
    """T = 2^20: dense levels large enough for the exact-size lists and the balanced jobs, up to 128 chunks per level."""
    _run(name, form, 20, 231, monkeypatch)


@pytest.mark.parametrize("hash_size,res", [(14, 200), (12, 64)])
@pytest.mark.parametrize("name", ["rays", "out_of_box"])
def test_scatter_small_tables(name, hash_size, res, monkeypatch):
    _run(name, "auto", hash_size, res, monkeypatch)
