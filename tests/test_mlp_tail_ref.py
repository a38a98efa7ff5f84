"""The inputs of tests/test_gpu_mlp_tail.py on the CPU: at the seed the GPU tests use, the float64 reference alone flags at most
2 % of the points of every case as near-kink (tests/mlp_ref.py's procedure zeroes their dy; the share is a condition on the
inputs), and the 80-input network that stands for DNS_MLP_LIVE_IN(80) on a 112-wide W_in is the zero-padded 112-input one."""
import pytest
import torch

import mlp_ref as mr
import mlp_tail_cases as tc


@pytest.mark.parametrize("kind,shape,P", tc.all_cases())
def test_tail_case_near_kink_share(kind, shape, P):
    assert tc.case_share(kind, shape, P, tc.SEED) <= 0.02


def test_tail_cases_cover_both_forms():
    tail = lambda n_out: n_out <= 33 and n_out % 32 == 1     # csrc/mlp_split.hpp tail_shape
    assert all(tail(s[1]) for s in tc.TAIL_NETS + tc.LIVE_NETS) and not any(tail(s[1]) for s in tc.OLD_NETS)
    assert {s[1] for s in tc.TAIL_NETS} == {1, 33} and {s[2:] for s in tc.TAIL_NETS} == {(64, 2), (32, 1)}


@pytest.mark.parametrize("shape", tc.LIVE_NETS)
def test_live_reference_is_the_zero_padded_network(shape):
    x1, x2, params, dy, live = tc.live_case(shape, tc.SEED)
    P = x1.shape[0]
    xp = torch.cat((x1, x2, torch.zeros(P, tc.N_IN_WIDE - tc.LIVE)), 1)
    a = mr.backward64(xp, params, dy, shape)
    b = mr.backward64(x1, live, dy, tc.live_shape(shape), x2=x2)
    # two float64 evaluations of the same sums in another blocking: 1e-12 of the largest entry (as tests/test_mlp_ref.py compares
    # the reference with float64 autograd)
    same = lambda u, v: float((u - v).abs().max()) <= 1e-12 * float(v.abs().max())
    assert same(a["y"], b["y"]) and same(a["dx"][:, :tc.LIVE], b["dx"])
    nn = shape[2]
    wa = a["dparams"][:nn * tc.N_IN_WIDE].reshape(nn, tc.N_IN_WIDE)
    assert same(wa[:, :tc.LIVE].reshape(-1), b["dparams"][:nn * tc.LIVE]) and float(wa[:, tc.LIVE:].abs().max()) == 0.0
    assert same(a["dparams"][nn * tc.N_IN_WIDE:], b["dparams"][nn * tc.LIVE:])
