"""Inputs of tests/test_gpu_mlp_tail.py (the tail-column form of the split-operand MLP kernels, csrc/mlp_split.hpp) and the seed
they run at.  The near-kink procedure of tests/mlp_ref.py holds the share of flagged points to 2 % -- a condition on the inputs,
not a measurement of the kernels -- so the seed is one for which the float64 reference alone meets it;
tests/test_mlp_tail_ref.py checks that on the CPU."""
import torch

import mlp_ref as mr

TAIL_NETS = [(80, 1, 64, 2), (80, 33, 64, 2), (80, 33, 32, 1), (32, 1, 32, 1)]      # n_out = 32 MT + 1: the tail form
OLD_NETS = [(80, 32, 64, 2), (80, 34, 64, 2), (80, 3, 64, 2)]                      # neighbours that keep the matrix-only path
POINTS = [1, 32, 33, 101, 517]        # one lane, a full wave tile, a one-point tail, mlp_ref's size, > one 128-slot block + 5
P_VAR = 101                           # the variants' size
LIVE, N1_LIVE, N_IN_WIDE = 80, 48, 112    # DNS_MLP_LIVE_IN(80) on a 112-wide W_in: segments of 48 and 32 live columns
LIVE_NETS = [(N_IN_WIDE, 1, 64, 2), (N_IN_WIDE, 33, 64, 2)]
MIN_COUNT = 2


def plain_case(shape, P, seed):
    return mr.base_inputs(shape, seed, P)


def group_case(shape, seed, P=P_VAR, G=4):
    """4 weight sets: set 1 has exactly MIN_COUNT points, set 2 none, two points have no set (padding slots in every tile)"""
    x, _, dy = mr.base_inputs(shape, seed, P)
    pool = torch.stack([mr.base_inputs(shape, seed + 1 + gi, P)[1] for gi in range(G)])
    slot = torch.where(torch.arange(P) % 3 == 0, 0, 3)
    slot[[5, 60]] = 1
    slot[[17, 90]] = -1
    return x, pool, dy, slot


def live_case(shape, seed, P=P_VAR):
    """x1 [P, 48], x2 [P, 32] (the live columns of a 112-wide input), the 112-input parameters, dy, and the parameters of the
    80-input network the kernels run (W_in's first 80 columns): the reference"""
    n_in, n_out, nn, nl = shape
    assert n_in == N_IN_WIDE
    x, params, dy = mr.base_inputs(shape, seed, P)
    w_in = params[:nn * n_in].reshape(nn, n_in)
    live = torch.cat((w_in[:, :LIVE].reshape(-1), params[nn * n_in:]))
    return x[:, :N1_LIVE].contiguous(), x[:, N1_LIVE:LIVE].contiguous(), params, dy, live


def live_shape(shape):
    return (LIVE,) + tuple(shape[1:])


def share(x, params, dy, shape, **kw):
    """share of near-kink points of the float64 reference"""
    ref = mr.analyse(x, params, dy, shape, "exact", **kw)
    return float(mr.near_kink(ref["pre"], ref["e_pre"]).float().mean())


def case_share(kind, shape, P, seed):
    if kind == "plain":
        return share(*plain_case(shape, P, seed), shape)
    if kind == "group":
        x, pool, dy, slot = group_case(shape, seed, P)
        return share(x, pool, dy, shape, group=slot, min_count=MIN_COUNT)
    x1, x2, _, dy, live = live_case(shape, seed, P)
    return share(x1, live, dy, live_shape(shape), x2=x2)


SEED = 1                              # every case below meets the condition at this seed (tests/test_mlp_tail_ref.py)


def all_cases():
    out = [("plain", s, P) for s in TAIL_NETS + OLD_NETS for P in POINTS]
    out += [("group", s, P_VAR) for s in TAIL_NETS]
    out += [("live", s, P_VAR) for s in LIVE_NETS]
    return out
