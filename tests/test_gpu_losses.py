"""csrc/losses.hip against the float64 host reference of tests/losses_ref.py, at the edges: narrow latents (L < 4), the
E % 4 tail, unaligned buffers, second trips of the grid-stride loops, rays of different validity inside one float4, the
flag-off branch, 0/0 denominators, d_occ with ldd_fine > L, the ray kernels around their workgroup sizes, cross-entropy
extremes.  Every case goes through BOTH routes:

* ``ops.mapping_losses`` / ``ops.tracking_losses``: dns_loss_sums -> dns_loss_finalize -> dns_loss_bwd;
* the raw entry points: dns_loss_rays, dns_loss_sums + dns_loss_finalize_bwd, and dns_loss_bwd_points with d_occ
  (ld_occ = 2) and ldd_fine = L + 3.

The bound of each quantity is max(1e-5, 4 x the fp32-CPU-vs-float64 error of that quantity on that case), capped at 1e-4
(tests/losses_ref.py bounds()); none is taken from the kernel's output.  tests/test_losses_ref.py shows on the host that
each edge case's mutant lies >= 100x that bound away."""
import ctypes as C

import pytest
import torch

import losses_ref as R
from util import REPORT, assert_close, elem_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0


def _lib():
    from dns_slam_amd import ops
    from dns_slam_amd._lib import check, ptr, stream_ptr
    return ops, ops.lib, check, ptr, stream_ptr


def _dev(t, offset=False):
    """Device copy; offset: a contiguous view that starts 4 bytes into a larger buffer (not 16-byte aligned)."""
    if t is None:
        return None
    if not offset:
        return t.to(DEV)
    buf = torch.full((t.numel() + 8,), SENTINEL, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _compare(got, want, bound, what, groups=None):
    """assert_close where the reference is finite; where it holds NaN / Inf they must match in place (elem_err)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if want.dim() == 0:
        got, want = got.reshape(1), want.reshape(1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.isfinite(want).all():
        assert_close(got, want, rtol=bound, what=what, groups=groups)
        return
    r = elem_err(got, want, rtol=bound, groups=groups)
    REPORT.append((what, float("nan"), r, bound))
    assert r <= 1.0, f"{what}: non-finite entries differ, or worst ratio {r:.2f}"


def _check(case, ref, bnd, got, path, grads=None):
    for t in R.TERMS:
        print(f"{path} {case.name} {t}: got {float(got['terms'][t])!r} want {float(ref['terms'][t])!r} bound {bnd[t]:.1e}")
    for t in R.TERMS:
        _compare(got["terms"][t], ref["terms"][t], bnd[t], f"losses/{path} {case.name}: {t}")
    for g in (grads if grads is not None else case.grad_names()):
        _compare(got["grads"][g], ref["grads"][g], bnd[g], f"losses/{path} {case.name}: {g}", R.grad_groups(g))


def _valid_u8(case):
    return None if case.valid is None else case.valid.to(torch.uint8).to(DEV)


def run_ops(case):
    """ops.mapping_losses / ops.tracking_losses and autograd with the upstream scalar g_total."""
    ops = _lib()[0]
    c = case
    leaf = lambda t, off=False: None if t is None else _dev(t, off).requires_grad_(True)
    pc, pd, lg = leaf(c.pred_color), leaf(c.pred_depth), leaf(c.logits if c.C else None)
    gc, gd, lab = _dev(c.gt_color), _dev(c.gt_depth), _dev(c.gt_label)
    if c.tracker:
        pv = leaf(c.pred_var)
        mask = torch.ones(c.N, dtype=torch.bool, device=DEV) if c.valid is None else c.valid.to(DEV)
        total, terms = ops.tracking_losses(pc, pd, pv, lg, gc, gd, lab, mask, c.lam[:3])
    else:
        fine, coarse = leaf(c.fine, "fine" in c.unaligned), leaf(c.coarse, "coarse" in c.unaligned)
        total, terms = ops.mapping_losses(pc, pd, lg, fine, coarse, gc, gd, lab, _dev(c.z), c.lam, valid=_valid_u8(c))
    total.backward(torch.tensor(float(c.g_total), device=DEV))
    torch.cuda.synchronize()
    t = dict(zip(R.TERMS, list(terms.detach().cpu()) + [total.detach().cpu()]))
    g = {"d_color": pc.grad, "d_depth": pd.grad}
    if c.C:
        g["d_logits"] = lg.grad
    if c.tracker:
        g["d_var"] = pv.grad
    else:
        g["d_fine"], g["d_coarse"] = fine.grad, coarse.grad
    return {"terms": t, "grads": g}


def run_raw(case, points=True):
    """-> (dns_loss_rays result, dns_loss_sums + dns_loss_finalize_bwd result); the first also carries d_fine / d_coarse of
    dns_loss_bwd_points (d_occ at ld_occ = 2, destination of leading dimension L + 3) when ``points``."""
    ops, lib, check, ptr, stream_ptr = _lib()
    c = case
    N, S, L, Cn, trk = c.N, c.S, c.L, c.C, int(c.tracker)
    lam = (C.c_float * 8)(*[float(v) for v in c.lam])
    f = lambda *s: torch.full(s, float("nan"), device=DEV)
    pc, pd, gc, gd, lab = _dev(c.pred_color), _dev(c.pred_depth), _dev(c.gt_color), _dev(c.gt_depth), _dev(c.gt_label)
    lg = _dev(c.logits) if Cn else None
    pv = _dev(c.pred_var) if trk else None
    valid = _valid_u8(c)
    fine = coarse = z = None
    if not trk:
        fine, coarse, z = _dev(c.fine, "fine" in c.unaligned), _dev(c.coarse, "coarse" in c.unaligned), _dev(c.z)
    g1 = torch.full((1,), float(c.g_total), device=DEV)
    res = []
    for fused in (True, False):
        sums, out = f(ops.LOSS_SUMS_FLOATS), f(16)
        dcol, ddep, dvar, dlog = f(N, 3), f(N), (f(N) if trk else None), (f(N, Cn) if Cn else None)
        if fused:
            check(lib.dns_loss_rays(lam, N, S, Cn, L, trk, ptr(pc), ptr(pd), ptr(pv), ptr(lg), ptr(gc), ptr(gd), ptr(lab), ptr(valid),
                                    ptr(fine), ptr(coarse), ptr(z), ptr(sums), ptr(out), ptr(g1), ptr(dcol), ptr(ddep), ptr(dvar),
                                    ptr(dlog), stream_ptr()), "dns_loss_rays")
        else:
            check(lib.dns_loss_sums(lam, N, S, Cn, L, trk, ptr(pc), ptr(pd), ptr(pv), ptr(lg), ptr(gc), ptr(gd), ptr(lab), ptr(valid),
                                    ptr(fine), ptr(coarse), ptr(z), ptr(sums), stream_ptr()), "dns_loss_sums")
            check(lib.dns_loss_finalize_bwd(lam, N, S, Cn, L, trk, ptr(sums), ptr(out), ptr(g1), ptr(pc), ptr(pd), ptr(pv), ptr(lg),
                                            ptr(gc), ptr(gd), ptr(lab), ptr(valid), ptr(dcol), ptr(ddep), ptr(dvar), ptr(dlog),
                                            stream_ptr()), "dns_loss_finalize_bwd")
        g = {"d_color": dcol, "d_depth": ddep}
        if Cn:
            g["d_logits"] = dlog
        if trk:
            g["d_var"] = dvar
        if fused and not trk and points:
            ldf = L + 3
            wide = torch.full((c.P, ldf), SENTINEL, device=DEV)
            dco_buf = torch.full((c.E + 8,), SENTINEL, device=DEV)
            o = 1 if "d_coarse" in c.unaligned else 4
            dco = dco_buf[o:o + c.E].view(c.P, L)
            docc = None
            if c.d_occ is not None:
                docc = torch.full((c.P, 2), SENTINEL, device=DEV)
                docc[:, 0] = c.d_occ.to(DEV)
            check(lib.dns_loss_bwd_points(lam, N, S, Cn, L, ptr(out), ptr(g1), ptr(gd), ptr(valid), ptr(fine), ptr(coarse), ptr(z),
                                          ptr(wide), ptr(dco), ldf, ptr(docc), 2, stream_ptr()), "dns_loss_bwd_points")
            torch.cuda.synchronize()
            assert bool((wide[:, L:] == SENTINEL).all()), "dns_loss_bwd_points wrote past column L of the wide destination"
            assert bool((dco_buf[:o] == SENTINEL).all()) and bool((dco_buf[o + c.E:] == SENTINEL).all()), "d_coarse: out of bounds"
            g["d_fine"], g["d_coarse"] = wide[:, :L], dco
        torch.cuda.synchronize()
        o16 = out.cpu()
        res.append({"terms": dict(zip(R.TERMS, list(o16[:7]))), "grads": g})
    return res


# ------------------------------------------------------------------------------------------------------------ mapper
@pytest.mark.parametrize("name", R.MAPPER_CASES)
def test_mapper_losses_ops_route_against_float64(name):
    case, ref, bnd = R.solved(name)
    _check(case, R.without_d_occ(case, ref), bnd, run_ops(case), "ops")


@pytest.mark.parametrize("name", R.MAPPER_CASES)
def test_mapper_losses_raw_entry_points_against_float64(name):
    case, ref, bnd = R.solved(name)
    rays, fin = run_raw(case)
    _check(case, ref, bnd, rays, "rays+points")
    _check(case, ref, bnd, fin, "sums+finalize_bwd", grads=[g for g in case.grad_names() if g not in ("d_fine", "d_coarse")])


# ----------------------------------------------------------------------------------------------------------- tracker
@pytest.mark.parametrize("name", R.TRACKER_CASES)
def test_tracker_losses_ops_route_against_float64(name):
    case, ref, bnd = R.solved(name)
    _check(case, ref, bnd, run_ops(case), "ops tracker")


@pytest.mark.parametrize("name", R.TRACKER_CASES)
def test_tracker_losses_raw_entry_points_against_float64(name):
    case, ref, bnd = R.solved(name)
    rays, fin = run_raw(case)
    _check(case, ref, bnd, rays, "rays tracker")
    _check(case, ref, bnd, fin, "sums+finalize_bwd tracker")


# ----------------------------------------------------------------------------------------------- the recorded fixture
@pytest.mark.parametrize("route", ["ops", "raw"])
@pytest.mark.parametrize("ci", [0, 1, 2])
def test_recorded_opacity_fixture_against_the_kernel(ci, route):
    """tests/golden/get_opacity_loss.npz (an L = 1 problem, recorded from get_opacity_loss of the modelled project with
    weights 3 and 7): fs, op and d(3 fs + 7 op)/d occ from the KERNEL against the recorded numbers.  Case 2 (all depths
    zero) is the flag-off branch: fs = op = 0 exactly and no gradient from them."""
    case, ref, bnd = R.solved(f"golden_c{ci}")
    got = run_ops(case) if route == "ops" else run_raw(case)[0]
    rec = case.recorded
    for t in ("fs", "op"):
        print(f"{route} golden_c{ci} {t}: got {float(got['terms'][t])!r} recorded {rec[t]!r}")
        _compare(got["terms"][t], torch.tensor(rec[t], dtype=torch.float64), bnd[t], f"losses/{route} fixture c{ci}: {t}")
    if rec["grad_occ"] is not None:
        _compare(got["grads"]["d_fine"], rec["grad_occ"].double(), bnd["d_fine"], f"losses/{route} fixture c{ci}: grad_occ", 1)
    else:
        assert float(got["terms"]["fs"]) == 0.0 and float(got["terms"]["op"]) == 0.0
        assert not bool(got["grads"]["d_fine"].any())


# ------------------------------------------------------------------------------- second trips of the grid-stride loops
def test_forward_point_loop_second_trip():
    """(2731, 47, 33): E = 4 235 781 > 1024 workgroups x 256 threads x 4 quads x 4 elements, E % 4 = 1.  The sums through
    dns_loss_rays (and the rays' gradients, which carry the coefficients cut from them)."""
    case, ref, bnd = R.solved("trip2_fwd")
    assert case.E > R.FWD_TRIP and case.E % 4 == 1
    rays, _ = run_raw(case, points=False)
    _check(case, ref, bnd, rays, "rays second trip", grads=["d_color", "d_depth", "d_logits"])


def test_point_backward_loop_second_trip():
    """(5479, 47, 33): E = 8 497 929 > 4096 workgroups x 256 threads x 2 quads x 4 elements.  ops.mapping_losses, i.e.
    dns_loss_bwd's point pass, every element of d_fine and d_coarse."""
    case, ref, bnd = R.solved("trip2_bwd")
    assert case.E > R.BWD_TRIP
    _check(case, R.without_d_occ(case, ref), bnd, run_ops(case), "ops second trip")
