"""Ray generation, depth-guided sampling and the pose gradient (csrc/sample.hip, csrc/dev_sample.hpp, the frame-begin kernel of
csrc/track_fused.inc) against tests/raygen_ref.py at their edges.

Forward: bit for bit against the fp32 reference spelled in the kernels' own association -- no tolerance, no second branch; NaN must
sit where the reference has NaN.  All three widths of the per-ray sort (1, 2 and 4 keys per lane: up to 64, 128, 256 samples), one
and many rays, a last workgroup that is partly full, a cropped window, shared and per-frame jitter, a computed and a given depth
maximum, frames without any positive depth, a ray origin on a face of the box (far = NaN), rays that leave the box before their
depth, quaternions of norm 0.5 and 3, camera constants that are not fp32 numbers.
Backward: dns_raygen_bwd through the C entry against float64 autograd, inside the error bound derived from the kernels' operation
order (raygen_ref.pose_grad_bound): ratio <= 1, nothing added; the measured ratios go to the parity report.
The maximum drawn depth is computed by four kernels and the forced mid sample by two: they are held to each other and to the CPU."""
import ctypes as C

import pytest
import torch

import raygen_ref as rr
from oracle import render_math as rm
from util import REPORT

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = rr.H, rr.W
NAN = float("nan")


def _ops():
    from dns_slam_amd import ops
    return ops


def _d(t):
    return None if t is None else t.to(DEV)


def _camv(cam):
    return (C.c_double * 4)(*[float(v) for v in cam])


def _forward(sc, requires_grad=False):
    """ops.raygen_sample on a case of raygen_ref -> the eight outputs (device), q and T (device leaves if requires_grad)."""
    q, T = _d(sc["q"]).requires_grad_(requires_grad), _d(sc["T"]).requires_grad_(requires_grad)
    outs = _ops().raygen_sample(q, T, _d(sc["idx"]), _d(sc["color"]), _d(sc["depth"]), _d(sc["label"]), sc["cam"], sc["bound"],
                                sc["window"], sc["npf"], _d(sc["t_uniform"]), _d(sc["t_surf"]), _d(sc["t_zero"]),
                                depth_max=_d(sc["depth_max"]))
    return dict(zip(("rays_o", "rays_d", "pts", "gt_color", "gt_depth", "gt_label", "inside", "z"), outs)), q, T


def _raw_forward(sc, f, idx, ws, given):
    """dns_raygen_sample through the C entry on ONE frame f of a scene with the draw ``idx`` [n]: -> z; ws [1] int32 is the
    depth-maximum word (written unless ``given``)."""
    ops = _ops()
    p, n, S = ops.ptr, idx.numel(), sc["nu"] + sc["ns"]
    H0, H1, W0, W1 = sc["window"]
    new = lambda *s, dt=torch.float32: torch.empty(*s, device=DEV, dtype=dt)
    ro, rd, gc, gd, gl, ins = new(n, 3), new(n, 3), new(n, 3), new(n), new(n, dt=torch.int64), new(n, dt=torch.uint8)
    z, pts = torch.full((n, S), NAN, device=DEV), new(n, S, 3)
    args = [_d(sc[k][f:f + 1].contiguous()) for k in ("color", "depth", "label", "q", "T")]
    tu, t, t0, ix = _d(sc["t_uniform"]), _d(sc["t_surf"]), _d(sc["t_zero"]), _d(idx)
    ops.check(ops.lib.dns_raygen_sample(p(ix), p(args[0]), p(args[1]), p(args[2]), p(args[3]), p(args[4]), _camv(sc["cam"]),
                                        ops._bound6(sc["bound"]), H, W, H0, H1, W0, W1, 1, n, p(tu), p(t), p(t0), sc["nu"], sc["ns"], 0,
                                        p(ws), 1 if given else 0, p(ro), p(rd), p(gc), p(gd), p(gl), p(ins), p(z), p(pts),
                                        ops.stream_ptr()), "dns_raygen_sample")
    torch.cuda.synchronize()
    return z.cpu()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("ci", range(len(rr.FORWARD_CASES)), ids=[rr.forward_id(c) for c in rr.FORWARD_CASES])
def test_raygen_sample_bit_exact_vs_ordered_reference(ci):
    sc = rr.forward_case(ci)
    ref = rr.forward_ref(sc)
    got = {k: v.detach().cpu() for k, v in _forward(sc)[0].items()}
    got["inside"] = got["inside"].bool()
    for k in ("gt_color", "gt_depth", "gt_label", "rays_o", "rays_d", "inside", "z", "pts"):
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        bad = ~((got[k] == ref[k]) | ((got[k] != got[k]) & (ref[k] != ref[k])))
        assert rr.same_bits(got[k], ref[k]), f"{k}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:3].tolist()}"
    assert rr.ascending(got["z"])


# ------------------------------------------------------------------------------------------------ stand-alone entry points
@pytest.mark.parametrize("nu,ns", [(1, 128), (136, 64), (200, 56)])
@pytest.mark.parametrize("rays", ["one", "five", "five_zero"])
def test_sample_along_rays_four_keys_per_lane(nu, ns, rays):
    """S = 129, 200, 256 (the widest sort) with far_bb NaN, +-inf and negative, and with every depth zero."""
    ops = _ops()
    g = torch.Generator().manual_seed(nu + ns)
    t, t0 = torch.rand(ns, generator=g), torch.rand(ns, generator=g)
    t[ns // 2] = 0.5
    if rays == "one":
        depth, far = torch.tensor([1.75]), torch.tensor([[2.2]], dtype=torch.float64)
    else:
        depth = torch.tensor([1.5, 0.0, 2.5, 0.7, 3.1]) * (0.0 if rays == "five_zero" else 1.0)
        far = torch.tensor([[NAN], [float("inf")], [float("-inf")], [-2.0], [3.7]], dtype=torch.float64)
    z = ops.sample_along_rays(_d(depth), _d(far), _d(torch.linspace(0.0, 1.0, steps=nu)), _d(t), _d(t0)).cpu()
    zo = rm.sample_along_rays(depth, nu, ns, far, t, t0)
    assert rr.same_bits(z, zo) and rr.ascending(z)
    if rays != "one" and nu >= 2:
        assert torch.isnan(z[0]).sum() == nu and not torch.isnan(z[1:]).any()          # NaN far: every uniform sample, sorted last


@pytest.mark.parametrize("n_rays", [1, 65, 300])
def test_sample_along_rays_maximum_in_the_last_ray(n_rays):
    """depth_max_flat_kernel: the only positive depth sits in the last ray (last lane of a wave, second wave, second workgroup);
    every other ray's samples are built from that maximum."""
    ops = _ops()
    nu, ns = 4, 3
    g = torch.Generator().manual_seed(n_rays)
    depth = torch.zeros(n_rays)
    depth[-1] = 3.25
    far = torch.rand(n_rays, 1, generator=g, dtype=torch.float64) * 6
    t, t0 = torch.rand(ns, generator=g), torch.rand(ns, generator=g)
    z = ops.sample_along_rays(_d(depth), _d(far), _d(torch.linspace(0.0, 1.0, steps=nu)), _d(t), _d(t0)).cpu()
    assert rr.same_bits(z, rm.sample_along_rays(depth, nu, ns, far, t, t0))
    assert float(z.max()) > 1.0


def test_rays_from_pixels_cropped_window():
    """dns_rays_from_pixels on the cropped window: drawn pixels through ops, and pixel r = ray r for n smaller than the window
    through the C entry; rays, the gathered image rows (C = 5) and the (col, row) output."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    H0, H1, W0, W1 = rr.CROP
    nwin = (H1 - H0) * (W1 - W0)
    image = torch.rand(H, W, 5, generator=g)
    q = torch.randn(4, generator=g)
    R, T = rr.rotation_ordered(q), torch.randn(3, generator=g)
    idx = rr.draw_indices(1, 300, rr.CROP, g)

    def want(ix):
        row, col = rr.pixels(ix, rr.CROP)
        ro, rd = rr.rays_ordered(ix, rr.CROP, R, T, rr.CAM_INEXACT)
        return ro, rd, image[row, col], torch.stack((col.float(), row.float()), -1)

    got = ops.rays_from_pixels(_d(R), _d(T), _d(idx), _d(image), rr.CAM_INEXACT, (H, W), rr.CROP)
    for a, b, k in zip(got, want(idx), ("rays_o", "rays_d", "sample", "ij")):
        assert torch.equal(a.cpu(), b), k
    n = 777                                                     # 14 rows of 53 and 35 pixels of the next: not the whole window
    assert n < nwin
    ro, rd, smp, ij = [torch.full(s, NAN, device=DEV) for s in ((n + 1, 3), (n + 1, 3), (n + 1, 5), (n + 1, 2))]
    p = ops.ptr
    Rd, Td, imd = _d(R.contiguous()), _d(T), _d(image)
    ops.check(ops.lib.dns_rays_from_pixels(None, p(imd), 5, p(Rd), p(Td), _camv(rr.CAM_INEXACT), H, W, H0, H1, W0, W1, n, p(ro), p(rd),
                                           p(smp), p(ij), ops.stream_ptr()), "dns_rays_from_pixels")
    torch.cuda.synchronize()
    for a, b, k in zip((ro, rd, smp, ij), want(torch.arange(n)), ("rays_o", "rays_d", "sample", "ij")):
        assert torch.equal(a.cpu()[:n], b), k
        assert torch.isnan(a.cpu()[n]).all(), k + ": written past n"


# ------------------------------------------------------------------------------------------------ backward
def _raw_bwd(sc, z, gp, gd, go, dq0=None, dT0=None, null_out=None):
    """dns_raygen_bwd through the C entry.  The workspace is NaN before the call (every slot that is read must have been written;
    the slots come back too); d_quat / d_trans start from dq0 / dT0 (zeros by default) or are NULL."""
    ops = _ops()
    p = ops.ptr
    K, npf = sc["K"], sc["npf"]
    H0, H1, W0, W1 = sc["window"]
    n_ws = int(ops.lib.dns_raygen_bwd_ws_floats(K, npf))
    assert n_ws == 12 * K * ((npf + 7) // 8)
    ws = torch.full((n_ws + 12,), NAN, device=DEV)
    dq = None if null_out == "quat" else (torch.zeros(K, 4, device=DEV) if dq0 is None else _d(dq0).clone())
    dT = None if null_out == "trans" else (torch.zeros(K, 3, device=DEV) if dT0 is None else _d(dT0).clone())
    idx, q, zd, gpd, gdd, god = _d(sc["idx"]), _d(sc["q"]), _d(z), _d(gp), _d(gd), _d(go)
    ops.check(ops.lib.dns_raygen_bwd(p(idx), p(q), _camv(sc["cam"]), H0, H1, W0, W1, K, npf, z.shape[1], p(zd), p(gpd), p(god), p(gdd),
                                     p(ws), p(dq), p(dT), ops.stream_ptr()), "dns_raygen_bwd")
    torch.cuda.synchronize()
    ws = ws.cpu()
    assert torch.isnan(ws[n_ws:]).all(), "workspace written past dns_raygen_bwd_ws_floats"
    return (None if dq is None else dq.cpu()), (None if dT is None else dT.cpu()), ws[:n_ws]


def _reference(sc, z, gp, gd, go):
    args = (sc["idx"], sc["window"], rr.cam32(sc["cam"]), z, gp, gd, go)
    return rr.pose_grad_f64(sc["q"], sc["T"], *args) + rr.pose_grad_bound(sc["q"], *args)


@pytest.mark.parametrize("ci", range(len(rr.BACKWARD_CASES)), ids=[rr.backward_id(c) for c in rr.BACKWARD_CASES])
def test_raygen_bwd_within_derived_bound(ci):
    sc = rr.backward_case(ci)
    z = _forward(sc)[0]["z"].cpu()
    dq, dT, ws = _raw_bwd(sc, z, sc["gp"], sc["gd"], sc["go"], null_out=sc["null_out"])
    assert torch.isfinite(ws).all()                            # every partial slot was written: no zero fill is needed
    dq_ref, dT_ref, Bq, BT = _reference(sc, z, sc["gp"], sc["gd"], sc["go"])
    assert (dq is None) == (sc["null_out"] == "quat") and (dT is None) == (sc["null_out"] == "trans")
    rq = 0.0 if dq is None else rr.bound_ratio(dq, dq_ref, Bq)
    rT = 0.0 if dT is None else rr.bound_ratio(dT, dT_ref, BT)
    REPORT.append((f"dns_raygen_bwd vs float64, {rr.backward_id(rr.BACKWARD_CASES[ci])}: |error| / derived bound of d_quat, d_trans",
                   rq, rT, 1.0))
    print(f"{rr.backward_id(rr.BACKWARD_CASES[ci])}: ratio d_quat {rq:.4f} d_trans {rT:.4f}")
    assert rq <= 1.0 and rT <= 1.0, (rq, rT)


def test_raygen_bwd_accumulates_into_the_outputs():
    sc = rr.backward_case(9)                                   # K 3, npf 515: 65 partial sums per frame
    z = _forward(sc)[0]["z"].cpu()
    g = torch.Generator().manual_seed(1)
    dq0, dT0 = torch.randn(3, 4, generator=g), torch.randn(3, 3, generator=g) * 100
    dq_z, dT_z, _ = _raw_bwd(sc, z, sc["gp"], sc["gd"], sc["go"])
    dq_a, dT_a, _ = _raw_bwd(sc, z, sc["gp"], sc["gd"], sc["go"], dq0=dq0, dT0=dT0)
    assert dq_z.abs().min() > 0 and dT_z.abs().min() > 0
    assert torch.equal(dq_a, dq0 + dq_z) and torch.equal(dT_a, dT0 + dT_z)


def test_raygen_bwd_nan_stays_in_its_frame():
    sc = rr.backward_case(6)                                   # K 2, npf 9, S 65, cropped, all three gradients
    z = _forward(sc)[0]["z"].cpu()
    dq_c, dT_c, _ = _raw_bwd(sc, z, sc["gp"], sc["gd"], sc["go"])
    gp = sc["gp"].clone()
    gp[sc["npf"] + 3, 64, 1] = NAN                             # frame 1, the sample of the lane-strided loop's second trip, y
    dq, dT, _ = _raw_bwd(sc, z, gp, sc["gd"], sc["go"])
    assert torch.isnan(dq[1]).all() and torch.isnan(dT[1, 1])
    assert torch.equal(dT[1, 0::2], dT_c[1, 0::2])              # d_trans x and z of frame 1 never see the y component
    assert torch.equal(dq[0], dq_c[0]) and torch.equal(dT[0], dT_c[0])


def test_raygen_autograd_node_on_cropped_window():
    """ops.raygen_sample's backward (its argument order into dns_raygen_bwd) on the cropped window."""
    sc = rr.backward_case(6)
    outs, q, T = _forward(sc, requires_grad=True)
    torch.autograd.backward([outs["pts"], outs["rays_d"], outs["rays_o"]], [_d(sc["gp"]), _d(sc["gd"]), _d(sc["go"])])
    dq_ref, dT_ref, Bq, BT = _reference(sc, outs["z"].cpu(), sc["gp"], sc["gd"], sc["go"])
    rq, rT = rr.bound_ratio(q.grad, dq_ref, Bq), rr.bound_ratio(T.grad, dT_ref, BT)
    REPORT.append(("ops.raygen_sample backward vs float64, cropped window: |error| / derived bound of d_quat, d_trans", rq, rT, 1.0))
    assert rq <= 1.0 and rT <= 1.0, (rq, rT)


# ------------------------------------------------------------------------------------------------ the maxima and the forced 0.5
@pytest.mark.parametrize("N,ns", [(1, 3), (255, 15), (257, 65), (700, 130)])
def test_track_begin_maximum_and_forced_half(N, ns):
    """dns_track_fused_begin on the cropped window, three iterations (the second draws pixels of depth 0 only): its maximum equals
    the CPU's and the word dns_raygen_sample computes for the same draw, bit for bit; a given maximum samples like a computed one;
    its jitter rows equal dns_force_half row by row (0.5 already at index 0 / only at an index past the first 64 / absent)."""
    ops = _ops()
    p = ops.ptr
    n_it = 3
    H0, H1, W0, W1 = rr.CROP
    nwin = (H1 - H0) * (W1 - W0)
    sc = rr.make_scene("plain", 1, rr.CROP, N, 7000 + N, rr.CAM_INEXACT)
    g = torch.Generator().manual_seed(N)
    rows, cols = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sc["depth"][0][(rows + cols) % 3 == 1] = 0.0               # a third of the pixels; the window's last pixel stays positive
    pix = torch.stack([rr.draw_indices(1, N, rr.CROP, g) for _ in range(n_it)])
    r, c = rr.pixels(torch.arange(nwin), rr.CROP)
    zero_idx = torch.nonzero(sc["depth"][0][r, c] == 0).reshape(-1)
    pix[1] = zero_idx[torch.randint(zero_idx.numel(), (N,), generator=g)]
    t = torch.rand(n_it, ns, generator=g)
    t[t == 0.5] = 0.25
    t[0, 0] = 0.5
    t[1, 64 if ns > 64 else ns - 1] = 0.5
    t_dev, dmax = _d(t), torch.full((n_it,), -1, device=DEV, dtype=torch.int32)
    depth_dev, pix_dev = _d(sc["depth"][0].contiguous()), _d(pix)
    ops.check(ops.lib.dns_track_fused_begin(p(pix_dev), N, n_it, p(depth_dev), W, H0, W0, W1, p(t_dev), ns, p(dmax), ops.stream_ptr()),
              "dns_track_fused_begin")
    torch.cuda.synchronize()
    # the forced mid sample
    want_rows = t.clone()
    want_rows[2, ns // 2 + 1] = 0.5
    for it in range(n_it):
        row = _d(t[it].clone())
        ops.check(ops.lib.dns_force_half(p(row), ns, ns // 2 + 1, ops.stream_ptr()), "dns_force_half")
        assert torch.equal(t_dev[it], row) and torch.equal(row.cpu(), want_rows[it]), it
    # the maxima
    pr, pc = rr.pixels(pix, rr.CROP)
    want = sc["depth"][0][pr, pc].max(1).values.clamp_min(0.0)
    dmax_f = dmax.view(torch.float32)
    assert torch.equal(dmax_f.cpu(), want) and float(want[1]) == 0.0 and float(want[0]) > 0.0
    sc.update(nu=5, ns=ns, K=1, npf=N, window=rr.CROP, cam=rr.CAM_INEXACT, bound=rr.BOUND, t_uniform=torch.linspace(0.0, 1.0, steps=5),
              t_zero=torch.rand(ns, generator=g))
    for it in range(n_it):
        sc["t_surf"] = want_rows[it]
        ws = torch.full((1,), -1, device=DEV, dtype=torch.int32)
        z_computed = _raw_forward(sc, 0, pix[it], ws, given=False)
        assert torch.equal(ws, dmax[it:it + 1]), it
        sc["idx"], sc["depth_max"] = pix[it], ws.view(torch.float32)
        z_given = _forward(sc)[0]["z"].cpu()
        sc["depth_max"] = None
        z_none = _forward(sc)[0]["z"].cpu()
        assert rr.same_bits(z_given, z_computed) and rr.same_bits(z_none, z_computed), it
        gd = sc["depth"][0][pr[it], pc[it]]
        far = rr.box_far(*rr.rays_ordered(pix[it], rr.CROP, rr.rotation_ordered(sc["q"][0]), sc["T"][0], sc["cam"]), gd, rr.BOUND)[0]
        assert rr.same_bits(z_computed, rr.z_values(gd, 5, ns, far, want_rows[it], sc["t_zero"])), it
