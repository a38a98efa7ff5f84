"""The float64 loss reference and its cases, checked on the host (no GPU): the reference reproduces the recorded
get_opacity_loss fixture and oracle/render_math.py, the two formulations in tests/losses_ref.py agree, every edge case is
SENSITIVE (its mutant lies at least 100x the GPU test's tolerance away from the truth), and no case but the dedicated one
puts a sample on a band edge."""
import numpy as np
import pytest
import torch

import losses_ref as R
from oracle import render_math as rm

ALL = list(R.CASES) + list(R.BIG_CASES)


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_reference_reproduces_the_recorded_opacity_fixture(ci):
    """fs, op and d(3 fs + 7 op)/d occ of tests/golden/get_opacity_loss.npz to 1e-6 of the recorded fp32 numbers, and the
    same from oracle/render_math.py evaluated in fp32."""
    case, ref, _ = R.solved(f"golden_c{ci}")
    rec = case.recorded
    for t in ("fs", "op"):
        assert abs(float(ref["terms"][t]) - rec[t]) <= 1e-6 * abs(rec[t]) or rec[t] == float(ref["terms"][t]), t
    occ = case.fine.reshape(-1).clone().requires_grad_(True)
    fs, op = rm.opacity_loss(case.z, case.gt_depth, occ, case.lam[6])
    for t, v in (("fs", fs), ("op", op)):
        v = float(v.detach())
        assert abs(float(ref["terms"][t]) - v) <= 1e-6 * abs(v) or v == float(ref["terms"][t]), t
    if rec["grad_occ"] is not None:
        (3.0 * fs + 7.0 * op).backward()
        got = ref["grads"]["d_fine"]
        scale = float(rec["grad_occ"].abs().max())
        assert float((got - rec["grad_occ"].double()).abs().max()) <= 1e-6 * scale
        assert float((got - occ.grad.reshape(-1, 1).double()).abs().max()) <= 1e-6 * scale
    else:
        assert float(ref["terms"]["fs"]) == 0.0 and float(ref["terms"]["op"]) == 0.0          # the flag-off branch
        assert not bool(ref["grads"]["d_fine"].any())


@pytest.mark.parametrize("name", [n for n in ALL if not n.endswith("all_invalid")])      # the oracle takes no empty batch
def test_reference_agrees_with_render_math_in_fp32(name):
    """Every term of the float64 reference against the oracle's own functions evaluated in fp32 on the kept rays: the
    reference adds nothing to those formulas but precision (and the fp32 comparisons, which the oracle makes in fp32 too)."""
    case, ref, _ = R.solved(name)
    c = case
    keep = torch.arange(c.N) if c.valid is None else torch.nonzero(c.valid).reshape(-1)
    want = {}
    if c.tracker:
        m = torch.ones(keep.numel(), dtype=torch.bool)
        want["p"] = rm.track_photometric_loss(c.gt_color[keep], c.pred_color[keep], m)
        want["d"] = rm.track_depth_loss(c.gt_depth[keep], c.pred_depth[keep], c.pred_var[keep], m)
        if c.C:
            want["l"] = rm.track_label_loss(c.gt_label[keep], c.logits[keep], m)
    else:
        want["p"] = rm.photometric_loss(c.gt_color[keep], c.pred_color[keep])
        want["d"] = rm.depth_loss(c.gt_depth[keep], c.pred_depth[keep])
        if c.C:
            want["l"] = rm.label_loss(c.gt_label[keep], c.logits[keep])
        f3, c3 = c.fine.reshape(c.N, c.S, c.L)[keep], c.coarse.reshape(c.N, c.S, c.L)[keep]
        want["lt"] = rm.latent_loss(c3, f3)
        want["fs"], want["op"] = rm.opacity_loss(c.z[keep], c.gt_depth[keep], f3[..., -1], c.lam[6], c.lam[7])
    for t, v in want.items():
        assert R.scalar_err(v, ref["terms"][t]) <= 2e-5, (t, float(v), float(ref["terms"][t]))


@pytest.mark.parametrize("name", ALL)
def test_the_two_formulations_agree(name):
    """Dropping the invalid rays (the reference) and weighting them by zero over the flat arrays (what the mutants are
    cut from) give the same seven terms in float64, NaN in the same places."""
    case, ref, _ = R.solved(name)
    got = R.masked_terms(case)
    for t in R.TERMS:
        assert R.scalar_err(got[t], ref["terms"][t]) <= 1e-11, (t, float(got[t]), float(ref["terms"][t]))


EDGES = [(n, m) for n in ALL for m in (R.CASES.get(n) or R.BIG_CASES[n])().edges]


@pytest.mark.parametrize("name,mut", EDGES)
def test_cases_are_sensitive_to_their_mutants(name, mut):
    """The quantity an edge moves differs, between the mutant and the truth, by >= 100x the bound the GPU test applies."""
    case, ref, bnd = R.solved(name)
    sep = R.separation(case, mut, ref, bnd)
    assert sep and all(v >= 100.0 for v in sep.values()), sep


def test_every_mutant_and_every_path_has_a_case():
    have = {m for _, m in EDGES}
    assert have == set(R.MUTANTS), set(R.MUTANTS) - have
    small = {n: R.CASES[n]() for n in R.MAPPER_CASES}
    assert {c.E % 4 for c in small.values() if "tail_dropped" in c.edges} == {1, 2, 3}
    for L in (1, 2, 3):                                      # the narrow latents: several points per quad, straddling rays
        assert any("quad_first_point" in c.edges and c.L == L for c in small.values()), L
        assert any("straddle_validity" in c.edges and c.L == L for c in small.values()), L
    big = {n: f() for n, f in R.BIG_CASES.items()}
    assert big["trip2_fwd"].E > R.FWD_TRIP and big["trip2_fwd"].E % 4 == 1
    assert big["trip2_bwd"].E > R.BWD_TRIP


@pytest.mark.parametrize("name", ALL)
def test_no_sample_sits_on_a_band_edge(name):
    """Apart from the dedicated boundary case no z lies within 1e-4 of d +- trunc: a mask flip there is no rounding
    difference for the tolerance to absorb.  The boundary case has samples EXACTLY on both edges, and they are in the band."""
    case = (R.CASES.get(name) or R.BIG_CASES[name])()
    if case.tracker:
        return
    t32 = torch.tensor(case.lam[6], dtype=torch.float32)
    d = case.gt_depth[:, None]
    lo, hi = (case.z - (d - t32)).abs(), (case.z - (d + t32)).abs()
    if case.boundary:
        front, back, dm = R.band_masks(case.z, case.gt_depth, case.lam[6])
        on = ((lo == 0) | (hi == 0)) & dm
        assert int(on.sum()) >= 2 and not bool((front | back)[on].any())
        lo, hi = lo[~on], hi[~on]
    if name.startswith("golden_"):
        # recorded data, not ours to move: case 1 has one sample 3.55e-5 (about 150 fp32 ulps of z) off its edge.  The
        # comparison is made on the same fp32 values by the reference and by the kernel, so it cannot flip; what is held here
        # is that the recorded samples stay two orders of magnitude clear of a rounding difference.
        assert float(torch.minimum(lo, hi).min()) > 1e-5
        return
    assert float(torch.minimum(lo, hi).min()) > 1e-4


@pytest.mark.parametrize("name", ALL)
def test_yardstick_and_bounds(name):
    """The fp32-CPU-vs-float64 error of every term and gradient tensor is finite, and the bound cut from it lies in
    [1e-5, 1e-4]."""
    case, ref, bnd = R.solved(name)
    err = R.yardstick(case, ref)
    assert set(err) == set(R.TERMS) | set(case.grad_names())
    for k, v in err.items():
        assert np.isfinite(v), (k, v)
        assert R.FLOOR <= bnd[k] <= R.RTOL and bnd[k] == R.bound_from(v)
