"""csrc/adam.hip (FusedAdam, dns_adam_step) against a float64 Adam written out here, torch's definition: bias corrections from
double-precision beta ** t, denom = sqrt(v) / sqrt(bc2) + eps, p -= lr / bc1 * m / denom.

Two comparisons.  (i) PER STEP: the update p_t - p_{t-1} and both moments against one reference step restarted from the
kernel's own fp32 state at t - 1, so the step's error is measured, not an accumulated one.  Parameters are kept at the
magnitude of a few hundred steps' worth of lr, so that the rounding of the stored parameter (2^-24 |p|) is small against
1e-4 of the update and nothing dilutes the comparison.  (ii) ACCUMULATED: the parameters after the run against an
uninterrupted float64 run.  The bound on the update and the moments is tests/util.py RTOL = 1e-4 (the kernel's
1 - 0.999f differs from 1e-3 by 4.7e-5; at t = 1 that cancels against its own bias correction)."""
import ctypes as C
import math

import pytest
import torch

from util import REPORT, RTOL, assert_close, elem_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-8
SENTINEL = 7.0


def ref_step(p, g, m, v, t, lr):
    """One float64 Adam step (torch.optim.Adam, no weight decay, no amsgrad) -> (p, m, v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    denom = v.sqrt() / math.sqrt(bc2) + EPS
    return p - (lr / bc1) * (m / denom), m, v


def _compare(got, want, what, rtol=RTOL, atol=None):
    got, want = got.detach().cpu(), want.detach().cpu()
    if torch.isfinite(want).all():
        assert_close(got, want, rtol=rtol, what=what, atol=atol)
        return
    r = elem_err(got, want, rtol=rtol, atol=atol)
    REPORT.append((what, float("nan"), r, rtol))
    assert r <= 1.0, f"{what}: non-finite entries differ, or worst ratio {r:.2f}"


def check_step(before, after, grads, lrs, t, what, merge_by_lr=False):
    """before / after: lists of (p, m, v) fp32 CPU tensors around kernel step t.  -> worst scale-relative update error.
    merge_by_lr: the tensors of one learning rate are compared as ONE vector.  Late in a run a one-element tensor's update
    can be a small fraction of lr by chance, and is then no longer resolved by the rounding of its stored parameter
    (2^-24 |p|, |p| ~ tens of lr); the group's vector keeps the scale of the comparison at the group's typical update, where
    that rounding is ~1e-6 of it, and a tensor stepped with another group's lr (10x) still stands out."""
    idx = {}
    for i, lr in enumerate(lrs):
        idx.setdefault(lr if merge_by_lr else i, []).append(i)
    worst = 0.0
    for key, ii in idx.items():
        steps = [ref_step(before[i][0], grads[i], before[i][1], before[i][2], t, lrs[i]) for i in ii]
        cat = lambda ts: torch.cat([x.reshape(-1).double() for x in ts])
        p0 = cat([before[i][0] for i in ii])
        upd, upd_ref = cat([after[i][0] for i in ii]) - p0, cat([s[0] for s in steps]) - p0
        if torch.isfinite(upd_ref).all():
            worst = max(worst, rel_err(upd, upd_ref))
        name = f"adam/{what} t={t} " + (f"lr={key:g}" if merge_by_lr else f"tensor {key} (n={before[key][0].numel()})")
        _compare(upd, upd_ref, f"{name}: update")
        _compare(cat([after[i][1] for i in ii]), cat([s[1] for s in steps]), f"{name}: exp_avg")
        _compare(cat([after[i][2] for i in ii]), cat([s[2] for s in steps]), f"{name}: exp_avg_sq")
    return worst


def _snap(opt, params):
    return [(p.detach().cpu().clone(), opt.state[p][0].cpu().clone(), opt.state[p][1].cpu().clone()) for p in params]


def _params(sizes, lrs, seed):
    """Parameters of the magnitude of their OWN learning rate (so the stored value resolves the update)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * lr).to(DEV).requires_grad_(True) for n, lr in zip(sizes, lrs)]


def _groups(params, lrs):
    by = {}
    for p, lr in zip(params, lrs):
        by.setdefault(lr, []).append(p)
    return [{"params": ps, "lr": lr} for lr, ps in by.items()]


SIZES = [1, 2, 3, 5, 7, 1023, 1024, 1025, 2048, 4097]      # one workgroup (1024 elements) exactly, and one either side


def test_sizes_per_step_and_accumulated_over_1000_steps():
    """Sizes around the float4 width and the workgroup; steps 1, 2, 10 and 1000 measured per step; the parameters after
    1000 steps against an uninterrupted float64 run."""
    from dns_slam_amd.optim import FusedAdam
    lrs = [(1e-2, 1e-3, 1e-4)[i % 3] for i in range(len(SIZES))]
    params = _params(SIZES, lrs, 1)
    opt = FusedAdam(_groups(params, lrs))
    gen = torch.Generator().manual_seed(2)
    base = [[torch.randn(n, generator=gen) for n in SIZES] for _ in range(8)]       # gradients cycle, magnitudes 1e-3 .. 10
    grad = lambda t, i: base[t % 8][i] * (10.0 ** ((t % 5) - 3))
    dev_grads = {(k, s): [(base[k][i] * (10.0 ** (s - 3))).to(DEV) for i in range(len(SIZES))] for k in range(8) for s in range(5)}
    p64 = [p.detach().cpu().double() for p in params]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    total_update = [torch.zeros_like(p) for p in p64]
    marks, snaps = (1, 2, 10, 1000), {}
    for t in range(1, 1001):
        for i, p in enumerate(params):
            p.grad = dev_grads[(t % 8, t % 5)][i]
        if t in marks:
            snaps[t] = [_snap(opt, params)]
        opt.step()
        if t in marks:
            snaps[t].append(_snap(opt, params))
        for i in range(len(SIZES)):
            new, m64[i], v64[i] = ref_step(p64[i], grad(t, i), m64[i], v64[i], t, lrs[i])
            total_update[i] += (new - p64[i]).abs()
            p64[i] = new
    assert float(opt._dev_state[0]) == 1000.0
    for t in marks:
        w = check_step(snaps[t][0], snaps[t][1], [grad(t, i) for i in range(len(SIZES))], lrs, t, "sizes", merge_by_lr=t > 2)
        print(f"adam sizes: worst scale-relative update error at t={t}: {w:.3e}")
        REPORT.append((f"adam/sizes t={t}: worst update error over tensors", w, w / RTOL, RTOL))
    # accumulated: the gradients do not depend on p, so the final error is at most the sum of the per-step ones:
    # RTOL * sum |update_t| for the arithmetic, plus one rounding of the stored parameter (2^-24 |p|) per step
    for i, p in enumerate(params):
        atol = RTOL * total_update[i] + 1000 * 2.0 ** -24 * p64[i].abs().clamp_min(lrs[i])
        _compare(p, p64[i], f"adam/sizes accumulated 1000 steps tensor {i} (n={SIZES[i]})", atol=atol)


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_unaligned_buffers_take_the_guarded_path_and_stay_inside(which):
    """Parameter, gradient and each moment in turn as a view 4 bytes into a larger buffer (dns_adam_step directly: the
    moments are FusedAdam's own).  Three steps against the reference; the enclosing buffer is bit-unchanged on both sides."""
    from dns_slam_amd import ops
    from dns_slam_amd._lib import DnsAdamTensor, check, ptr, stream_ptr
    sizes, lrs = [1029, 6, 2048], [1e-2, 1e-3, 1e-4]
    gen = torch.Generator().manual_seed(3)
    bufs, views = {}, {}
    for k in "pgmv":
        for i, n in enumerate(sizes):
            off = 1 if k == which else 4
            b = torch.full((n + 12,), SENTINEL, device=DEV)
            v = b[off:off + n]
            init = torch.randn(n, generator=gen) * (lrs[i] if k == "p" else 1.0) if k in "pg" else torch.zeros(n)
            v.copy_(init)
            assert v.data_ptr() % 16 == (4 if k == which else 0)
            bufs[k, i], views[k, i] = (b, off), v
    state = torch.zeros(3, device=DEV)
    arr = (DnsAdamTensor * len(sizes))()
    for i, n in enumerate(sizes):
        arr[i].p, arr[i].g, arr[i].m, arr[i].v = (views[k, i].data_ptr() for k in "pgmv")
        arr[i].n, arr[i].lr = n, lrs[i]
    snap = lambda: [tuple(views[k, i].cpu().clone() for k in "pmv") for i in range(len(sizes))]
    for t in (1, 2, 3):
        for i, n in enumerate(sizes):
            views["g", i].copy_(torch.randn(n, generator=gen) * 10.0 ** (t - 2))
        before = snap()
        check(ops.lib.dns_adam_step(arr, len(sizes), B1, B2, EPS, ptr(state), stream_ptr()), "dns_adam_step")
        torch.cuda.synchronize()
        check_step(before, snap(), [views["g", i].cpu() for i in range(len(sizes))], lrs, t, f"unaligned {which}")
    for (k, i), (b, off) in bufs.items():
        n = sizes[i]
        assert bool((b[:off] == SENTINEL).all()) and bool((b[off + n:] == SENTINEL).all()), (k, i)


@pytest.mark.parametrize("mode", ["optim", "direct"])
def test_block_end_walk_with_frozen_tensors_and_per_group_lr(mode):
    """32 tensors of mixed sizes in three groups whose lr are a factor 10 apart (a tensor stepped with its neighbour's lr is
    off by 10x); the first, the last, two adjacent ones and two more have no gradient.  'optim': FusedAdam drops them before
    the call; 'direct': dns_adam_step gets all 32 entries, the frozen ones with g = NULL.  Frozen tensors and their moments
    are bit-unchanged."""
    from dns_slam_amd import ops
    from dns_slam_amd._lib import DnsAdamTensor, check, ptr, stream_ptr
    from dns_slam_amd.optim import FusedAdam
    sizes = [5, 1024, 3, 1025, 7, 2049, 1, 4, 1023, 2, 6, 4097, 9, 2048, 11, 3, 1500, 8, 13, 1024, 5, 3000, 2, 17, 1, 999, 4, 6, 33,
             1026, 10, 7]
    assert len(sizes) == 32
    lrs = [1e-2] * 11 + [1e-3] * 11 + [1e-4] * 10
    frozen = {0, 31, 10, 11, 5, 20}
    params = _params(sizes, lrs, 4)
    opt = FusedAdam(_groups(params, lrs))
    gen = torch.Generator().manual_seed(5)
    if mode == "direct":
        state = torch.zeros(3, device=DEV)
        grads_dev = [torch.zeros(n, device=DEV) for n in sizes]
        arr = (DnsAdamTensor * 32)()
        for i, p in enumerate(params):
            m, v = opt.state[p]
            arr[i].p, arr[i].m, arr[i].v, arr[i].n, arr[i].lr = p.data_ptr(), m.data_ptr(), v.data_ptr(), sizes[i], lrs[i]
            arr[i].g = None if i in frozen else grads_dev[i].data_ptr()
    with torch.no_grad():
        for i in frozen:                                     # moments that are not zero, so that "unchanged" says something
            opt.state[params[i]][0].fill_(0.25)
            opt.state[params[i]][1].fill_(0.5)
    start = _snap(opt, params)
    for t in (1, 2, 3):
        grads = [torch.randn(n, generator=gen) * 10.0 ** (t - 2) for n in sizes]
        before = _snap(opt, params)
        if mode == "optim":
            for i, p in enumerate(params):
                p.grad = None if i in frozen else grads[i].to(DEV)
            opt.step()
        else:
            for i in range(32):
                grads_dev[i].copy_(grads[i])
            check(ops.lib.dns_adam_step(arr, 32, B1, B2, EPS, ptr(state), stream_ptr()), "dns_adam_step")
        torch.cuda.synchronize()
        after = _snap(opt, params)
        live = [i for i in range(32) if i not in frozen]
        check_step([before[i] for i in live], [after[i] for i in live], [grads[i] for i in live], [lrs[i] for i in live], t,
                   f"block_end {mode}")
    end = _snap(opt, params)
    for i in frozen:
        for a, b in zip(start[i], end[i]):
            assert torch.equal(a, b), i


def test_gradient_magnitudes_and_zero_gradient():
    """1e-20, 1e-8, 1 and 1e8 (and an exact 0) in ONE tensor, each class held to ITS OWN magnitude: the update to
    RTOL |update| + 2^-24 |p| (the rounding of the stored parameter), exp_avg to RTOL of itself, exp_avg_sq to RTOL of itself
    above 1e-37 (below that fp32 is subnormal and carries no 1e-4).  A zero gradient moves nothing: 0 / eps, no NaN."""
    from dns_slam_amd.optim import FusedAdam
    n, lr = 1030, 1e-3
    mags = torch.tensor([1e-20, 1e-8, 1.0, 1e8, 0.0])
    gen = torch.Generator().manual_seed(6)
    sign = (torch.rand(n, generator=gen) > 0.5).float() * 2 - 1
    g = mags[torch.arange(n) % 5] * sign * (0.5 + torch.rand(n, generator=gen))
    (p,) = _params([n], [lr], 7)
    opt = FusedAdam([{"params": [p], "lr": lr}])
    for t in (1, 2, 3):
        before = _snap(opt, [p])
        p.grad = g.to(DEV)
        opt.step()
        torch.cuda.synchronize()
        after = _snap(opt, [p])
        (p0, m0, v0), (p1, m1, v1) = before[0], after[0]
        pr, mr, vr = ref_step(p0, g, m0, v0, t, lr)
        upd, upd_ref = p1.double() - p0.double(), pr - p0.double()
        _compare(upd, upd_ref, f"adam/magnitudes t={t}: update", atol=2.0 ** -24 * p0.double().abs())
        _compare(m1, mr, f"adam/magnitudes t={t}: exp_avg", atol=1e-37)
        _compare(v1, vr, f"adam/magnitudes t={t}: exp_avg_sq", atol=1e-37)
        z = g == 0
        assert torch.equal(p1[z], p0[z]) and not bool(m1[z].any()) and not bool(v1[z].any())
        assert bool(torch.isfinite(p1).all())


def test_non_finite_gradients_poison_only_their_own_element():
    from dns_slam_amd.optim import FusedAdam
    sizes, lrs = [2048, 7], [1e-3, 1e-3]
    params = _params(sizes, lrs, 8)
    opt = FusedAdam(_groups(params, lrs))
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(n, generator=gen) for n in sizes]
    grads[0][5], grads[0][1026], grads[1][6] = float("nan"), float("inf"), float("-inf")
    before = _snap(opt, params)
    for p, g in zip(params, grads):
        p.grad = g.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    after = _snap(opt, params)
    check_step(before, after, grads, lrs, 1, "non-finite")          # NaN / Inf must sit where the reference has them
    bad = torch.zeros(2048, dtype=torch.bool)
    bad[5] = bad[1026] = True
    assert bool(torch.isnan(after[0][0][bad]).all()) and bool(torch.isfinite(after[0][0][~bad]).all())
    assert bool(torch.isnan(after[1][0][6])) and bool(torch.isfinite(after[1][0][:6]).all())


def test_33_tensors_are_refused_before_anything_is_launched():
    """More than 32 tensors with a gradient: ValueError, and parameters, both moments of every tensor and the device step
    count are bit-unchanged.  A following step over exactly 32 tensors is step 1."""
    from dns_slam_amd.optim import FusedAdam
    sizes = [3 + (i * 37) % 1100 for i in range(33)]
    lrs = [(1e-2, 1e-3, 1e-4)[i % 3] for i in range(33)]
    params = _params(sizes, lrs, 10)
    opt = FusedAdam(_groups(params, lrs))
    order = [p for g in opt.param_groups for p in g["params"]]                # the order FusedAdam walks them in
    lr_of = {id(p): lr for p, lr in zip(params, lrs)}
    gen = torch.Generator().manual_seed(11)
    grads = {id(p): torch.randn(p.numel(), generator=gen) for p in order}
    for p in order:
        p.grad = grads[id(p)].to(DEV)
    before = _snap(opt, order)
    with pytest.raises(ValueError, match="more than 32 parameter tensors"):
        opt.step()
    torch.cuda.synchronize()
    after = _snap(opt, order)
    for i, (a, b) in enumerate(zip(before, after)):
        for x, y, name in zip(a, b, ("parameter", "exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), f"tensor {i}: {name} changed by the refused step"
    assert torch.equal(opt._dev_state.cpu(), torch.zeros(3)), "the refused step ticked the device step count"
    order[-1].grad = None                                                     # 32 left: the full batch of one launch
    opt.step()
    torch.cuda.synchronize()
    assert float(opt._dev_state[0]) == 1.0
    end = _snap(opt, order)
    live = order[:-1]
    check_step(before[:-1], end[:-1], [grads[id(p)] for p in live], [lr_of[id(p)] for p in live], 1, "after the refusal")
    for x, y in zip(before[-1], end[-1]):
        assert torch.equal(x, y)
