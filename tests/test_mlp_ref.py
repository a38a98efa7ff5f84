"""tests/mlp_ref.py on the CPU: the float64 reference against autograd and a hand-computed network; the derived bound against a
torch emulation of the stated operand format (it holds the format as stated, and rejects a lost lo plane and a tile-wide scale
by more than 100x: neither vacuous nor unreachable); and the seeds of tests/test_gpu_mlp_range.py (near-kink share <= 2 %)."""
import pytest
import torch

import mlp_ref as mr
from oracle import tcnn_ref as tr

D = torch.float64
SEED = 5                                                   # the seed of the GPU range tests


@pytest.mark.parametrize("shape", mr.NETS)
def test_reference_equals_float64_autograd(shape):
    n_in, n_out, nn, nl = shape
    x, params, dy = mr.base_inputs(shape, 1, P=37)
    xd, pd = x.to(D).requires_grad_(True), params.to(D).requires_grad_(True)
    y = tr.mlp_forward(xd, pd, n_in, n_out, nn, nl)
    y.backward(dy.to(D))
    r = mr.backward64(x, params, dy, shape)
    y64, pres = mr.forward64(x, params, shape)
    assert torch.equal(y64, r["y"]) and len(pres) == nl and pres[0].shape == (37, nn)
    tol = lambda t: 1e-12 * float(t.abs().max())
    assert float((r["y"] - y.detach()).abs().max()) <= tol(y.detach())
    assert float((r["dx"] - xd.grad).abs().max()) <= tol(xd.grad)
    used = mr.used_count(shape)
    mats = tr.mlp_split(pd.grad, n_in, n_out, nn, nl)
    want = mr.flat_used(list(mats[:-1]) + [mats[-1][:n_out]])
    assert r["dparams"].numel() == used and float((r["dparams"] - want).abs().max()) <= tol(want)
    # two segments and a group index: the same numbers, split / gathered
    n1 = 16 if n_in > 16 else 8
    r2 = mr.backward64(x[:, :n1], params, dy, shape, x2=x[:, n1:])
    assert torch.equal(r2["y"], r["y"]) and torch.equal(r2["dx1"], r["dx"][:, :n1]) and torch.equal(r2["dx2"], r["dx"][:, n1:])
    grp = torch.arange(37) % 2
    grp[5] = -1
    pool = torch.stack((params, params * 0.5))
    rg = mr.backward64(x, pool, dy, shape, group=grp)
    even = (grp == 0).nonzero().reshape(-1)
    re = mr.backward64(x[even], params, dy[even], shape)
    assert torch.equal(rg["y"][even], re["y"]) and torch.equal(rg["dx"][even], re["dx"]) and torch.equal(rg["dparams"][0], re["dparams"])
    assert float(rg["y"][5].abs().max()) == 0.0 and float(rg["dx"][5].abs().max()) == 0.0


def test_reference_hand_computed_two_layer_network():
    """n_in 2, 2 hidden units, 1 output: W_in = [[1, -2], [3, 1]], W_out = [[2, -1]] (15 padded rows), x = (1, 2), (-1, 1)."""
    shape = (2, 1, 2, 1)
    params = torch.zeros(tr.mlp_param_count(*shape))
    params[:4] = torch.tensor([1.0, -2.0, 3.0, 1.0])
    params[4:6] = torch.tensor([2.0, -1.0])
    x = torch.tensor([[1.0, 2.0], [-1.0, 1.0]])
    dy = torch.tensor([[1.0], [10.0]])
    r = mr.backward64(x, params, dy, shape)
    # point 0: pre = (-3, 5), h = (0, 5), y = -5; point 1: pre = (-3, -2), h = 0, y = 0
    assert r["pre"][0].tolist() == [[-3.0, 5.0], [-3.0, -2.0]]
    assert r["y"].tolist() == [[-5.0], [0.0]]
    # dh = dy W_out masked: point 0 (0, -1), point 1 (0, 0); dx = dh W_in = (-3, -1), (0, 0)
    assert r["dx"].tolist() == [[-3.0, -1.0], [0.0, 0.0]]
    # dW_in = dh^T x = [[0, 0], [-1, -2]]; dW_out = dy^T h = [[0, 5]]
    assert r["dparams"].tolist() == [0.0, 0.0, -1.0, -2.0, 0.0, 5.0]


def test_operand_error_is_the_stated_format():
    v = torch.tensor([1.0, 2.0 ** -20, 0.0], dtype=D)
    # group maximum 1: k = 13
    e = mr.operand_error(v, torch.tensor(1.0), "f16x2")
    assert e.tolist() == [2.0 ** -22, 2.0 ** -38, 2.0 ** -38]
    assert mr.operand_error(v, torch.tensor(1.0), "f16").tolist() == [2.0 ** -11, 2.0 ** -31, 2.0 ** -38]
    assert mr.operand_error(v, None, "bf16x3").tolist() == [2.0 ** -23, 2.0 ** -43, 0.0]
    # the clamp: a maximum of 2^-120 asks for k = 134 and gets 110
    assert float(mr.scale_exp(torch.tensor(2.0 ** -120))) == 110.0 and float(mr.scale_exp(torch.tensor(2.0 ** 125))) == -110.0
    assert float(mr.scale_exp(torch.tensor(0.0))) == 0.0 and float(mr.scale_exp(torch.tensor(float("inf")))) == 0.0
    assert float(mr.operand_error(torch.tensor([0.0], dtype=D), torch.tensor(2.0 ** -120), "f16x2")) == 2.0 ** -135
    # and the format really is that good: representation error of random values within the bound, attained to within 4x
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 80, generator=g) * torch.exp2(torch.randint(-30, 1, (64, 80), generator=g).float())).to(D)
    m = x.abs().amax(dim=1, keepdim=True)
    err = (mr._represent(x, mr.scale_exp(m)) - x).abs()
    bound = mr.operand_error(x, m, "f16x2")
    assert bool((err <= bound).all()) and float((err / bound).max()) > 0.25


def _emulation_ratios(x, params, dy, shape, mode="exact", name=None, bound_mode=None, **variant):
    """the emulated format against the bound, by the procedure of the GPU tests: near-kink points lose their dy where
    mr.kinks_zeroed says so, else they keep it and the bound carries the undetermined-unit term"""
    ref = mr.analyse(x, params, dy, shape, bound_mode or mode)
    zero = mr.kinks_zeroed(bound_mode or mode, name)
    dy, kinks = mr.mask_kinks(dy, ref["pre"], ref["e_pre"], zero)
    if zero:
        ref = mr.analyse(x, params, dy, shape, bound_mode or mode)
    y, dx, dp = mr.emulate(x, params, dy, shape, **dict({"lo": mode == "exact"}, **variant))
    return {"y": mr.ratio(y, ref["y"], ref["e_y"]), "dx": mr.ratio(dx, ref["dx"], ref["e_dx"]),
            "dparams": mr.ratio(dp, ref["dparams"], ref["e_dparams"])}, kinks, ref


@pytest.mark.parametrize("shape", mr.NETS)
@pytest.mark.parametrize("name", mr.FINITE)
def test_emulated_format_is_inside_the_bound(name, shape):
    """... and the seed's near-kink share is at most 2 % (asserted again on the GPU) wherever the format allows that"""
    x, params, dy = mr.finite_case(name, shape, SEED)
    r, kinks, _ = _emulation_ratios(x, params, dy, shape, name=name)
    if mr.kinks_zeroed("exact", name):
        assert int(kinks.sum()) <= 0.02 * x.shape[0], f"{int(kinks.sum())} near-kink points"
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("shape", mr.NETS)
@pytest.mark.parametrize("name", mr.FINITE)
def test_emulated_f16_format_is_inside_its_bound_with_every_point_kept(name, shape):
    """The f16 mode flags most points (its pre-activation bound is 2^-11 of sum |W||x|), so no point is dropped: the bound carries
    the undetermined-unit term instead.  The hi-only emulation stays inside it; a backward that ignores the ReLU mask, one that
    skips a layer's transpose product and a sign error do not -- the bound still tells a wrong backward from a right one."""
    x, params, dy = mr.finite_case(name, shape, SEED)
    r, kinks, ref = _emulation_ratios(x, params, dy, shape, mode="fp16", name=name)
    assert max(r.values()) <= 1.0, r
    if name == "inrow-30w":                                 # operands 2^-30 below their row carry the result: in f16 under the
        return                                              # row's scale they keep no bits, and every unit is undetermined
    Ws = mr.mats64(params, shape)
    g = dy.to(D)
    for W in reversed(Ws):                                  # no ReLU mask at all
        g = g @ W
    assert mr.ratio(g, ref["dx"], ref["e_dx"]) > 1.0
    assert mr.ratio(-ref["dx"], ref["dx"], ref["e_dx"]) > 1.0
    assert mr.ratio(-ref["dparams"], ref["dparams"], ref["e_dparams"]) > 1.0
    assert mr.ratio(torch.zeros_like(ref["dx"]), ref["dx"], ref["e_dx"]) > 1.0


@pytest.mark.parametrize("shape", mr.NETS)
def test_emulated_two_segment_and_group_cases_are_inside_the_bound(shape):
    n_in = shape[0]
    n1 = mr.N1[n_in]
    x1, x2, params, dy = mr.two_segment_case(shape, n1, SEED)
    # one scale per row of the concatenation (the fp32 two-segment entry points)
    r, kinks, _ = _emulation_ratios(torch.cat((x1, x2), 1), params, dy, shape)
    assert int(kinks.sum()) <= 0.02 * x1.shape[0] and max(r.values()) <= 1.0, (r, int(kinks.sum()))
    x, pool, dy, slot = mr.group_case(shape, SEED)
    ref = mr.analyse(x, pool, dy, shape, group=slot)
    assert int(mr.near_kink(ref["pre"], ref["e_pre"]).sum()) <= 0.02 * x.shape[0]
    for gi in range(3):
        idx = (slot == gi).nonzero().reshape(-1)
        y, dx, dp = mr.emulate(x[idx], pool[gi], dy[idx], shape)
        assert mr.ratio(y, ref["y"][idx], ref["e_y"][idx]) <= 1.0 and mr.ratio(dx, ref["dx"][idx], ref["e_dx"][idx]) <= 1.0
        assert mr.ratio(dp, ref["dparams"][gi], ref["e_dparams"][gi]) <= 1.0
    assert float(ref["y"][11].abs().max()) == 0.0 and float(ref["y"][50].abs().max()) == 0.0


@pytest.mark.parametrize("shape", mr.NETS)
def test_a_lost_lo_plane_exceeds_the_bound(shape):
    x, params, dy = mr.finite_case("rows", shape, SEED)
    r, _, _ = _emulation_ratios(x, params, dy, shape, lo=False)
    assert min(r.values()) > 1.0 and max(r.values()) > 100.0, r


@pytest.mark.parametrize("shape", mr.NETS)
def test_a_tile_wide_scale_exceeds_the_bound_on_mixed_magnitudes(shape):
    x, params, dy = mr.finite_case("rows", shape, SEED)
    r, _, _ = _emulation_ratios(x, params, dy, shape, tile_scale=True)
    assert min(r["y"], r["dx"]) > 100.0, r


@pytest.mark.parametrize("shape", [s for s in mr.NETS if mr.N1[s[0]] % 16 == 0])
def test_two_segment_alignment_is_modelled(shape):
    """Split rows with their own exponents: what xs_align's max(e - e_k, -24) leaves in the operand is inside input_error -- the
    bound names the clamp's cost (a segment 2^-30 below the other is carried 2^6 too large) -- and a clamp set wrong (-12) is
    not, by more than 100x.  Without any clamp the multiplier underflows to 0 and the small segment is dropped: a SMALLER error,
    which no bound can object to."""
    n1 = mr.N1[shape[0]]
    x1, x2, _, _ = mr.two_segment_case(shape, n1, SEED)
    X = torch.cat((x1, x2), 1).to(D)
    bound = mr.input_error(X, "exact", n1, own_exps=True)
    r = mr.ratio(mr.emulate_aligned(x1, x2), X, bound)
    assert 0.5 < r <= 1.0, r                                # reached: the 2^-30 rows sit on the modelled term
    assert mr.ratio(mr.emulate_aligned(x1, x2, clamp=-12), X, bound) > 100.0
    assert mr.ratio(mr.emulate_aligned(x1, x2, clamp=-40), X, bound) <= 1.0
