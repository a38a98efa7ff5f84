"""tests/raygen_ref.py against the oracle and against itself, on the CPU: the ordered fp32 reference of ray generation agrees
with oracle/render_math.py on every forward case of the GPU table (bit for bit on most frames: the count is reported), the float64
pose gradient equals a central difference, the coefficient tables behind the error bound reproduce autograd, and an fp32 autograd
evaluation of the same loss lies inside the bound on every backward case."""
import pytest
import torch

import raygen_ref as rr
from oracle import render_math as rm
from util import REPORT, assert_close


def _oracle_frame(sc, f):
    """oracle/render_math.py on frame f of a forward case, as test_raygen_sample_bit_exact_vs_oracle calls it."""
    npf, window = sc["npf"], sc["window"]
    idx = sc["idx"][f * npf:(f + 1) * npf]
    img5 = torch.cat((sc["color"][f], sc["depth"][f][..., None], sc["label"][f][..., None]), -1)
    i, j = rm.uv_from_indices(idx, *window)
    px = rm.gather_pixels(idx, img5, *window)
    ro, rd = rm.rays_from_uv(i, j, rm.rotation_from_quad(sc["q"][f]), sc["T"][f], *sc["cam"])
    far, ins = rm.box_far(ro, rd, px[:, 3], sc["bound"])
    return px, ro.contiguous(), rd, far, ins


def test_ordered_reference_agrees_with_oracle():
    frames = equal_R = equal_d = equal_all = 0
    some_outside = some_nan = False
    for ci in range(len(rr.FORWARD_CASES)):
        sc = rr.forward_case(ci)
        ref = rr.forward_ref(sc)
        npf = sc["npf"]
        for f in range(sc["K"]):
            sl = slice(f * npf, (f + 1) * npf)
            what = f"ordered reference vs oracle, {rr.forward_id(rr.FORWARD_CASES[ci])} frame {f}"
            px, ro, rd, far, ins = _oracle_frame(sc, f)
            assert torch.equal(ref["gt_color"][sl], px[:, :3]) and torch.equal(ref["gt_depth"][sl], px[:, 3])
            assert torch.equal(ref["gt_label"][sl], px[:, 4].long())
            assert torch.equal(ref["rays_o"][sl], ro)
            frames += 1
            eq_R = torch.equal(rr.rotation_ordered(sc["q"][f]), rm.rotation_from_quad(sc["q"][f]))
            eq_d = torch.equal(ref["rays_d"][sl], rd)
            equal_R += eq_R
            equal_d += eq_d
            zo = rr.z_values(px[:, 3], sc["nu"], sc["ns"], far, sc["t_surf"][f] if sc["t_surf"].dim() == 2 else sc["t_surf"],
                             sc["t_zero"][f] if sc["t_zero"].dim() == 2 else sc["t_zero"],
                             None if sc["depth_max"] is None else sc["depth_max"][f])
            if eq_d:
                # same rays: the fp64 clip, the samples and the points have no freedom left
                assert rr.same_bits(ref["far"][sl], far) and torch.equal(ref["inside"][sl], ins), what
                assert rr.same_bits(ref["z"][sl], zo), what
                assert rr.same_bits(ref["pts"][sl], rm.points_from_rays(ro, rd, zo)), what
                equal_all += 1
            else:
                assert_close(ref["rays_d"][sl], rd, rtol=1e-6, what=what + " rays_d")
                assert_close(ref["z"][sl], zo, rtol=1e-6, what=what + " z")
            assert rr.ascending(ref["z"][sl])
            some_outside |= bool((~ref["inside"][sl] & torch.isfinite(ref["far"][sl][:, 0])).any())
            some_nan |= bool(torch.isnan(ref["far"][sl]).any() and torch.isnan(ref["z"][sl]).any())
    REPORT.append((f"ordered fp32 reference vs oracle: frames with bit-equal rotation {equal_R}, rays_d {equal_d}, everything "
                   f"{equal_all}, of {frames}", 0.0, 0.0, 0.0))
    print(f"bit-equal frames: R {equal_R}, rays_d {equal_d}, all {equal_all} of {frames}")
    assert some_outside and some_nan              # the table holds a finite ray that leaves the box early, and a NaN far with NaN z


def test_ordered_reference_on_the_existing_tests_frames():
    """The 15 frames of test_raygen_sample_bit_exact_vs_oracle (5 sample counts x 3 frames): how many the oracle (torch's association,
    which may depend on the host's vector width) and the ordered reference agree on bit for bit is reported -- 15 of 15 where this
    was written --; the rest must agree to the rtol that test grants."""
    from test_gpu_kernels import _scene_small
    n_eq = 0
    for nu, ns in [(32, 15), (48, 16), (96, 32), (0, 15), (22, 10)]:
        _, _, _, q, T = _scene_small(nu + ns)
        cam = (50.0, 52.0, 31.5, 23.5)
        idx = torch.randint(48 * 64, (3 * 200,), generator=torch.Generator().manual_seed(9))
        for f in range(3):
            sl = idx[f * 200:(f + 1) * 200]
            i, j = rm.uv_from_indices(sl, *rr.FULL)
            _, rd = rm.rays_from_uv(i, j, rm.rotation_from_quad(q[f]), T[f], *cam)
            rd_ord = rr.rays_ordered(sl, rr.FULL, rr.rotation_ordered(q[f]), T[f], cam)[1]
            if torch.equal(rd_ord, rd):
                n_eq += 1
            else:
                assert_close(rd_ord, rd, rtol=1e-6, what=f"ordered reference vs oracle, existing test {nu}+{ns} frame {f} rays_d")
    REPORT.append((f"ordered fp32 reference vs oracle on the existing forward test's frames: bit-equal {n_eq} of 15", 0.0, 0.0, 0.0))
    print(f"existing forward test's frames: bit-equal {n_eq} of 15")


def test_every_sort_width_sees_both_kinds_of_ray():
    seen = {}
    for ci, c in enumerate(rr.FORWARD_CASES):
        E = 1 if c[0] + c[1] <= 64 else 2 if c[0] + c[1] <= 128 else 4
        gd = rr.forward_ref(rr.forward_case(ci))["gt_depth"]
        s = seen.setdefault(E, {"pos": False, "zero": False, "windows": set(), "shapes": set()})
        s["pos"] |= bool((gd > 0).any())
        s["zero"] |= bool((gd == 0).any())
        s["windows"].add(c[4])
        s["shapes"].add((c[2], c[3]))
    for E in (1, 2, 4):
        assert seen[E]["pos"] and seen[E]["zero"] and len(seen[E]["windows"]) == 2 and len(seen[E]["shapes"]) >= 2, (E, seen[E])


def _z_of(sc):
    return rr.forward_ref(sc)["z"]


def test_pose_grad_f64_equals_central_difference():
    sc = rr.backward_case(2)                                   # K 1, npf 7, S 5, cropped window, all three gradients
    z = _z_of(sc)
    c32 = rr.cam32(sc["cam"])
    args = (sc["idx"], sc["window"], c32, z, sc["gp"], sc["gd"], sc["go"])
    dq, dT = rr.pose_grad_f64(sc["q"], sc["T"], *args)
    q0, T0 = sc["q"].double(), sc["T"].double()
    h = 1e-6
    for f in range(sc["K"]):
        for c in range(4):
            e = torch.zeros_like(q0)
            e[f, c] = h
            fd = (rr.pose_loss(q0 + e, T0, *args) - rr.pose_loss(q0 - e, T0, *args)) / (2 * h)
            assert abs(float(fd) - float(dq[f, c])) <= 1e-7 * float(dq[f].norm()), (f, c, float(fd), float(dq[f, c]))
        for c in range(3):
            e = torch.zeros_like(T0)
            e[f, c] = h
            fd = (rr.pose_loss(q0, T0 + e, *args) - rr.pose_loss(q0, T0 - e, *args)) / (2 * h)
            assert abs(float(fd) - float(dT[f, c])) <= 1e-7 * float(dT[f].norm()), (f, c, float(fd), float(dT[f, c]))


@pytest.mark.parametrize("ci", range(len(rr.BACKWARD_CASES)), ids=[rr.backward_id(c) for c in rr.BACKWARD_CASES])
def test_bound_holds_an_fp32_evaluation(ci):
    sc = rr.backward_case(ci)
    z = _z_of(sc)
    c32 = rr.cam32(sc["cam"])
    args = (sc["idx"], sc["window"], c32, z, sc["gp"], sc["gd"], sc["go"])
    dq, dT = rr.pose_grad_f64(sc["q"], sc["T"], *args)
    # the chain rule the bound is pushed through is the one autograd differentiates
    G, _ = rr.pose_sums_f64(sc["idx"], sc["window"], c32, sc["K"], z, sc["gp"], sc["gd"], sc["go"])
    dq_s, dT_s = rr.pose_grad_from_sums(sc["q"], G)
    scale = max(float(dq.abs().max()), float(G.abs().max()), 1e-30)
    assert float((dq_s - dq).abs().max()) <= 1e-11 * scale and float((dT_s - dT).abs().max()) <= 1e-11 * scale
    Bq, BT = rr.pose_grad_bound(sc["q"], *args)
    assert torch.isfinite(Bq).all() and torch.isfinite(BT).all()
    # non-zero wherever a term reaches the sum; exactly zero where none does (d_rays_o alone moves no rotation, d_rays_d alone no
    # translation: the kernels then add up zeros, exactly)
    assert (Bq > 0).all() if (sc["gp"] is not None or sc["gd"] is not None) else (Bq == 0).all()
    assert (BT > 0).all() if (sc["gp"] is not None or sc["go"] is not None) else (BT == 0).all()
    q32, T32 = sc["q"].clone().requires_grad_(True), sc["T"].clone().requires_grad_(True)
    rr.pose_loss(q32, T32, *args).backward()
    gq = torch.zeros_like(q32) if q32.grad is None else q32.grad
    gT = torch.zeros_like(T32) if T32.grad is None else T32.grad
    rq, rT = rr.bound_ratio(gq, dq, Bq), rr.bound_ratio(gT, dT, BT)
    REPORT.append((f"pose gradient bound, CPU fp32 autograd, {rr.backward_id(rr.BACKWARD_CASES[ci])}: ratio d_quat, d_trans",
                   rq, rT, 1.0))
    assert rq <= 1.0 and rT <= 1.0, (rq, rT)
