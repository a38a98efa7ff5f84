"""tests/scatter_ref.py (the float64 reference of the table-gradient scatter) against a plain per-corner loop over the oracle's rows
and fractions -- on the inputs where rows wrap (points outside the cube) and where thousands of contributions meet in eight rows."""
import numpy as np
import pytest
import torch

import scatter_ref as sref
from oracle import tcnn_ref as tr


@pytest.mark.parametrize("hash_size,res", [(16, 592), (12, 64)])
@pytest.mark.parametrize("name", ["out_of_box", "one_cell"])
def test_reference_equals_a_per_corner_index_add_loop(name, hash_size, res):
    meta = sref.meta_of(hash_size, res)
    x, g = sref.inputs(name, hash_size, res)
    exp, A, n = sref.reference(name, hash_size, res)
    rows, fr = tr.hashgrid_indices(x, meta)
    assert int(rows.min()) >= 0 and int(rows.max()) < meta.total_rows
    e2 = np.zeros((meta.total_rows, 2))
    a2 = np.zeros((meta.total_rows, 2))
    n2 = np.zeros((meta.total_rows, 2))
    g64 = g.double().numpy()
    for l in range(meta.n_levels):
        f = fr[:, l]
        for c in range(8):
            w = (f[:, 0] if c & 1 else 1 - f[:, 0]) * (f[:, 1] if c & 2 else 1 - f[:, 1]) * (f[:, 2] if c & 4 else 1 - f[:, 2])
            assert w.dtype == torch.float32
            w = w.double().numpy()[:, None]
            r = rows[:, l, c].numpy()
            gl = g64[:, 2 * l:2 * l + 2]
            np.add.at(e2, r, w * gl)
            np.add.at(a2, r, w * np.abs(gl))
            np.add.at(n2, r, ((w != 0) & (gl != 0)).astype(np.float64))
    # float64 sums of the same float64 terms in another order
    assert np.all(np.abs(exp.numpy() - e2) <= 1e-13 * a2 + 1e-300)
    assert np.all(np.abs(A.numpy() - a2) <= 1e-13 * a2)
    assert np.array_equal(n.numpy(), n2)
    assert np.all((n2 == 0) == (a2 == 0))


def test_inputs_have_the_shapes_they_are_named_for():
    meta = sref.meta_of(16, 592)
    x, _ = sref.inputs("rays", 16, 592)
    rows, _ = tr.hashgrid_indices(x, meta)
    same = (rows[1:, 0, 0] == rows[:-1, 0, 0]).float().mean()
    assert same > 0.5, "consecutive ray samples share their level-0 cell more often than not"
    x, _ = sref.inputs("one_cell", 16, 592)
    rows, _ = tr.hashgrid_indices(x, meta)
    assert len(torch.unique(rows[:, 0, 0])) == 1
    x, _ = sref.inputs("out_of_box", 16, 592)
    g0 = torch.floor(x[0] * torch.tensor(meta.levels[0].scale) + 0.5)
    assert g0.tolist() == [-1.0, 0.0, 0.0]
    assert bool((x < 0).any()) and bool((x > 1).any())
    for name in sref.INPUTS:
        if name != "out_of_box":
            xi, gi = sref.inputs(name, 16, 592)
            assert bool((xi >= 0).all() and (xi <= 1).all()) and xi.shape[0] == gi.shape[0] <= 4096
    _, g = sref.inputs("sparse", 16, 592)
    assert 0.05 < float((g != 0).any(1).float().mean()) < 0.15
    _, g = sref.inputs("sparse_one", 16, 592)
    assert int((g != 0).any(1).sum()) == 1
