"""References for ray generation, depth-guided sampling and the pose gradient (csrc/sample.hip, csrc/dev_sample.hpp), plain torch
on the CPU; imports nothing of the product.

FORWARD.  ``rotation_ordered``, ``rays_ordered``, ``box_far`` and ``points`` spell the kernels' arithmetic operation by
operation: fp32 elementwise torch ops on the CPU are correctly rounded and never fused, so with the association of
``quat_to_R`` (|q|^2 = ((rr + ii) + jj) + kk), ``pixel_dir`` ((col - cx) / fx with the camera constants rounded to fp32 first) and
``raygen_sample_kernel`` (d = (x + y) + z, the box clip in fp64, pts = o + d z) these functions ARE the specification, bit for bit;
there is no summation order left to excuse.  The z values reuse ``oracle.render_math.sample_along_rays`` (it sorts in fp64 and then
rounds; rounding is monotone, so that equals the kernel's round-then-sort).

BACKWARD.  ``pose_grad_f64`` is float64 autograd of  sum pts . gp + sum rays_d . gd + sum rays_o . go  at the fp32 inputs promoted;
``pose_grad_bound`` is the a-priori fp32 error bound of ``raygen_bwd_reduce_kernel`` + ``raygen_bwd_pose_kernel`` derived from their
operation order: nothing is fitted to what the kernels return.

The case tables of tests/test_raygen_ref.py (CPU) and tests/test_gpu_raygen.py (GPU) live here, so both files run the same inputs.
"""
import math

import torch

from oracle import render_math as rm

H, W = 48, 64
FULL = (0, 48, 0, 64)
CROP = (5, 41, 7, 60)
BOUND = torch.tensor([[-3.0, 3.5], [-2.5, 4.0], [-2.0, 2.2]], dtype=torch.float64)
CAM_EXACT = (50.0, 52.0, 31.5, 23.5)            # exact in fp32
CAM_INT = (50.0, 52.0, 32.0, 24.0)              # integer principal point: pixel (cx, cy) has dir = (0, -0, -1)
CAM_INEXACT = (517.3, 516.5, 31.7, 23.9)        # none of the four is an fp32 number


# ------------------------------------------------------------------------------------------------ forward, in the kernels' order
def cam32(cam):
    """The camera constants as the entry points round them (make_cam): four fp32 numbers."""
    return torch.tensor([float(v) for v in cam], dtype=torch.float64).float()


def rotation_ordered(q):
    """quat_to_R (dev_sample.hpp): q [..., 4] fp32 (r, i, j, k) -> R [..., 3, 3], two_s = 2 / (((rr + ii) + jj) + kk)."""
    q = q.float()
    qr, qi, qj, qk = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    nrm = ((qr * qr + qi * qi) + qj * qj) + qk * qk
    two_s = 2.0 / nrm
    jj, kk, ii = qj * qj, qk * qk, qi * qi
    ij, kr, ik, jr, jk, ir = qi * qj, qk * qr, qi * qk, qj * qr, qj * qk, qi * qr
    rows = [1.0 - two_s * (jj + kk), two_s * (ij - kr), two_s * (ik + jr),
            two_s * (ij + kr), 1.0 - two_s * (ii + kk), two_s * (jk - ir),
            two_s * (ik - jr), two_s * (jk + ir), 1.0 - two_s * (ii + jj)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def pixels(idx, window):
    """Window-flat index -> (row, col) of the image, int64 (pixel_dir's first two lines)."""
    H0, _, W0, W1 = window
    w = W1 - W0
    return H0 + torch.div(idx, w, rounding_mode="floor"), W0 + idx % w


def dirs_ordered(idx, window, cam):
    """pixel_dir: ((col - cx) / fx, -((row - cy) / fy), -1) in fp32 on the fp32 camera."""
    c = cam32(cam)
    row, col = pixels(idx, window)
    d0 = (col.float() - c[2]) / c[0]
    d1 = -((row.float() - c[3]) / c[1])
    return torch.stack((d0, d1, -torch.ones_like(d0)), -1)


def rays_ordered(idx, window, R, T, cam):
    """The ray lines of raygen_sample_kernel / rays_from_pixels_kernel for ONE frame: R [3, 3], T [3] fp32 ->
    rays_o, rays_d [n, 3] with d[a] = (dir0 R[a,0] + dir1 R[a,1]) + dir2 R[a,2]."""
    dr = dirs_ordered(idx, window, cam)
    R = R.float()
    d = [(dr[:, 0] * R[a, 0] + dr[:, 1] * R[a, 1]) + dr[:, 2] * R[a, 2] for a in range(3)]
    rays_d = torch.stack(d, -1)
    return T.float().expand(rays_d.shape).contiguous(), rays_d


def box_far(rays_o, rays_d, gt_depth, bound):
    """The fp64 box clip of raygen_sample_kernel: far = min over axes of max(t0, t1), NaN propagating (0 / 0 on a face);
    inside = far >= depth BEFORE the + 0.01.  -> (far + 0.01 [n, 1] fp64, inside [n] bool)."""
    o, d = rays_o.double(), rays_d.double()
    m = [torch.maximum((bound[a, 0] - o[:, a]) / d[:, a], (bound[a, 1] - o[:, a]) / d[:, a]) for a in range(3)]
    far = torch.minimum(torch.minimum(m[0], m[1]), m[2])
    return (far + 0.01)[:, None], far >= gt_depth.double()


def z_values(gt_depth, nu, ns, far_bb, t_surf, t_zero, depth_max=None):
    """oracle sample_along_rays on one frame's rays.  depth_max (a float >= the rays' own maximum: the all-ranks maximum of a
    multi-GPU step) replaces the rays' maximum: a phantom ray of that depth is appended for the call and its row dropped."""
    if depth_max is None:
        return rm.sample_along_rays(gt_depth, nu, ns, far_bb, t_surf, t_zero)
    assert float(depth_max) >= max(float(gt_depth.max()), 0.0)
    d = torch.cat((gt_depth.reshape(-1), torch.tensor([float(depth_max)])))
    f = torch.cat((far_bb.reshape(-1, 1), torch.ones(1, 1, dtype=torch.float64)))
    return rm.sample_along_rays(d, nu, ns, f, t_surf, t_zero)[:-1]


def points(rays_o, rays_d, z):
    """pts = o + d z, product and sum rounded separately."""
    return rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]


def same_bits(a, b):
    """NaN in the same places, everything else torch.equal (payloads of NaN are not compared)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros((), dtype=a.dtype)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


def ascending(z):
    """Every row ascending, NaN last."""
    a, b = z[:, :-1], z[:, 1:]
    return bool(((b >= a) | torch.isnan(b)).all())


# ------------------------------------------------------------------------------------------------ scenes and the forward table
def draw_indices(K, npf, window, g):
    """[K * npf] window-flat indices; every frame draws index 0 first and the window's last index last (npf == 1: even frames
    the last index, odd frames 0)."""
    nwin = (window[1] - window[0]) * (window[3] - window[2])
    idx = torch.randint(nwin, (K, npf), generator=g)
    idx[:, 0] = 0
    idx[:, -1] = nwin - 1
    if npf == 1:
        idx[1::2, 0] = 0
    return idx.reshape(-1)


def make_scene(kind, K, window, npf, seed, cam, norm_shift=0):
    """color [K,H,W,3], depth, label [K,H,W], q [K,4], T [K,3], idx [K*npf] in the style of test_gpu_kernels._scene_small.
    Every frame: depth 0 at the window's first pixel and > 0 at its last (both are always drawn).  Quaternion norms cycle through
    (about 1, 0.5, 3) from ``norm_shift``.  kind:
      plain    nothing more
      zero     frame 0 has depth 0 everywhere; frame 1 (if any) is positive at the window's last pixel only
      last     frame 0 is positive at the window's last pixel only; frame 1 (if any) has depth 0 everywhere
      nanfar   frame 0: identity quaternion, translation on the x = bound[0,0] face, pixel (cx, cy) drawn second (cam must have
               an integer principal point inside the window; npf >= 3): column cx has d_x = 0 -> 0/0 -> far = NaN, row cy has
               d_y = -0 (axis-aligned, +-inf)
    """
    g = torch.Generator().manual_seed(seed)
    H0, H1, W0, W1 = window
    color = torch.rand(K, H, W, 3, generator=g)
    depth = torch.rand(K, H, W, generator=g) * 4 + 0.3
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    label = torch.randint(0, 6, (K, H, W), generator=g).float()
    q = torch.randn(K, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * (1 + 0.1 * torch.rand(K, 1, generator=g))
    q = q * torch.tensor([(1.0, 0.5, 3.0)[(f + norm_shift) % 3] for f in range(K)])[:, None]
    T = torch.randn(K, 3, generator=g) * 0.5
    idx = draw_indices(K, npf, window, g)
    depth[:, H0, W0] = 0.0
    depth[:, H1 - 1, W1 - 1] = 1.0 + torch.rand(K, generator=g) * 3
    if kind in ("zero", "last"):
        only_last = torch.zeros(H, W)
        only_last[H1 - 1, W1 - 1] = 2.75
        pair = (torch.zeros(H, W), only_last) if kind == "zero" else (only_last, torch.zeros(H, W))
        for f in range(min(K, 2)):
            depth[f] = pair[f]
    elif kind == "nanfar":
        cx, cy = int(cam[2]), int(cam[3])
        assert float(cam[2]) == cx and float(cam[3]) == cy and H0 <= cy < H1 and W0 <= cx < W1 and npf >= 3
        q[0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        T[0] = torch.tensor([float(BOUND[0, 0]), 0.25, -0.5])
        idx[1] = (cy - H0) * (W1 - W0) + (cx - W0)
    elif kind != "plain":
        raise ValueError(kind)
    return {"color": color, "depth": depth, "label": label, "q": q, "T": T, "idx": idx}


# (nu, ns, K, npf, window, per-frame jitter, depth_max given, scene kind, camera)
FORWARD_CASES = [
    (0, 1, 1, 1, FULL, False, False, "plain", CAM_EXACT),            # E = 1
    (0, 1, 3, 64, CROP, True, True, "plain", CAM_INEXACT),
    (0, 3, 1, 3, CROP, False, False, "zero", CAM_INEXACT),
    (0, 3, 2, 67, FULL, True, False, "zero", CAM_EXACT),
    (63, 1, 3, 200, FULL, False, True, "nanfar", CAM_INT),
    (63, 1, 1, 3, CROP, True, False, "last", CAM_INEXACT),
    (64, 1, 2, 67, CROP, False, False, "nanfar", CAM_INT),           # E = 2
    (64, 1, 1, 1, FULL, True, True, "plain", CAM_INEXACT),
    (96, 32, 3, 64, FULL, True, False, "zero", CAM_INEXACT),
    (96, 32, 1, 3, CROP, False, True, "plain", CAM_EXACT),
    (128, 1, 3, 200, CROP, False, False, "plain", CAM_INEXACT),      # E = 4
    (128, 1, 1, 1, FULL, True, True, "plain", CAM_EXACT),
    (129, 71, 2, 67, FULL, False, False, "nanfar", CAM_INT),
    (129, 71, 3, 64, CROP, True, True, "last", CAM_INEXACT),
    (192, 64, 1, 3, FULL, True, False, "zero", CAM_INEXACT),
    (192, 64, 3, 200, CROP, False, True, "zero", CAM_EXACT),
    (0, 130, 2, 67, CROP, True, False, "plain", CAM_INEXACT),
    (0, 130, 3, 64, FULL, False, True, "nanfar", CAM_INT),
]


def forward_id(c):
    return f"{c[0]}+{c[1]}-K{c[2]}x{c[3]}-{'crop' if c[4] == CROP else 'full'}-{'pf' if c[5] else 'sh'}-{'dm' if c[6] else 'nodm'}-{c[7]}"


def forward_case(ci):
    """Inputs of FORWARD_CASES[ci]: the scene plus jitter (t_surf, t_zero: [ns] shared or [K, ns] per frame), t_uniform and, where
    given, depth_max [K] (>= each frame's own maximum over its draw, equal to it on frame 2)."""
    nu, ns, K, npf, window, per_frame, dm_given, kind, cam = FORWARD_CASES[ci]
    sc = make_scene(kind, K, window, npf, 1000 + ci, cam, norm_shift=ci)
    g = torch.Generator().manual_seed(2000 + ci)
    shape = (K, ns) if per_frame else (ns,)
    t, t0 = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if ns > 1:
        t[..., ns // 2] = 0.5
    sc.update(nu=nu, ns=ns, K=K, npf=npf, window=window, cam=cam, bound=BOUND, t_surf=t, t_zero=t0,
              t_uniform=torch.linspace(0.0, 1.0, steps=nu) if nu else None, depth_max=None)
    if dm_given:
        row, col = pixels(sc["idx"], window)
        own = sc["depth"][torch.arange(K).repeat_interleave(npf), row, col].reshape(K, npf).max(1).values.clamp_min(0.0)
        dm = own * 1.5 + 0.25
        dm[2:3] = own[2:3]
        sc["depth_max"] = dm
    return sc


def forward_ref(sc):
    """The ordered fp32 reference of dns_raygen_sample on a case of ``forward_case``: dict of the eight outputs (+ far)."""
    K, npf, nu, ns, window = sc["K"], sc["npf"], sc["nu"], sc["ns"], sc["window"]
    out = {k: [] for k in ("rays_o", "rays_d", "pts", "gt_color", "gt_depth", "gt_label", "inside", "z", "far")}
    for f in range(K):
        idx = sc["idx"][f * npf:(f + 1) * npf]
        row, col = pixels(idx, window)
        ro, rd = rays_ordered(idx, window, rotation_ordered(sc["q"][f]), sc["T"][f], sc["cam"])
        gd = sc["depth"][f, row, col]
        far, ins = box_far(ro, rd, gd, sc["bound"])
        t = sc["t_surf"][f] if sc["t_surf"].dim() == 2 else sc["t_surf"]
        t0 = sc["t_zero"][f] if sc["t_zero"].dim() == 2 else sc["t_zero"]
        z = z_values(gd, nu, ns, far, t, t0, None if sc["depth_max"] is None else sc["depth_max"][f])
        for k, v in (("rays_o", ro), ("rays_d", rd), ("pts", points(ro, rd, z)), ("gt_color", sc["color"][f, row, col]),
                     ("gt_depth", gd), ("gt_label", sc["label"][f, row, col].long()), ("inside", ins), ("z", z), ("far", far)):
            out[k].append(v)
    return {k: torch.cat(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ pose gradient
def _rotation_f64(q):
    qr, qi, qj, qk = q[0], q[1], q[2], q[3]
    two_s = 2.0 / (q * q).sum()
    return torch.stack([1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                        two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)]).reshape(3, 3)


def _dirs_f64(idx, window, cam_f32):
    """The EXACT direction of the fp32 camera: (col - cx) / fx in float64 (the kernel's two roundings are part of its error)."""
    c = cam_f32.double()
    row, col = pixels(idx, window)
    d0 = (col.double() - c[2]) / c[0]
    d1 = -((row.double() - c[3]) / c[1])
    return torch.stack((d0, d1, -torch.ones_like(d0)), -1)


def pose_loss(q, T, idx, window, cam_f32, z, gp, gd, go):
    """sum pts . gp + sum rays_d . gd + sum rays_o . go in the dtype of q (float64 for the reference); gp / gd / go may be None."""
    K = q.shape[0]
    npf = idx.numel() // K
    dt = q.dtype
    loss = torch.zeros((), dtype=dt)
    for f in range(K):
        sl = slice(f * npf, (f + 1) * npf)
        dirs = _dirs_f64(idx[sl], window, cam_f32).to(dt)
        rd = dirs @ _rotation_f64(q[f]).t()
        ro = T[f].expand(npf, 3)
        if gp is not None:
            loss = loss + ((ro[:, None, :] + rd[:, None, :] * z[sl].to(dt)[:, :, None]) * gp[sl].to(dt)).sum()
        if gd is not None:
            loss = loss + (rd * gd[sl].to(dt)).sum()
        if go is not None:
            loss = loss + (ro * go[sl].to(dt)).sum()
    return loss


def pose_grad_f64(q, T, idx, window, cam_f32, z, gp, gd, go):
    """float64 autograd of ``pose_loss`` at the fp32 inputs promoted -> (d_quat [K, 4], d_trans [K, 3]) float64."""
    qd, Td = q.double().clone().requires_grad_(True), T.double().clone().requires_grad_(True)
    pose_loss(qd, Td, idx, window, cam_f32, z, gp, gd, go).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return zero(qd), zero(Td)


def pose_sums_f64(idx, window, cam_f32, K, z, gp, gd, go):
    """The 12 per-frame sums the reduce kernel forms, exact terms in float64: G [K, 12] (dL/dR row-major, then dL/dT) and the
    sums of the terms' absolute values A [K, 12]."""
    npf = idx.numel() // K
    G, A = torch.zeros(K, 12, dtype=torch.float64), torch.zeros(K, 12, dtype=torch.float64)
    for f in range(K):
        sl = slice(f * npf, (f + 1) * npf)
        dirs = _dirs_f64(idx[sl], window, cam_f32)
        gdv, gdv_abs = torch.zeros(npf, 3, dtype=torch.float64), torch.zeros(npf, 3, dtype=torch.float64)
        gov, gov_abs = torch.zeros(npf, 3, dtype=torch.float64), torch.zeros(npf, 3, dtype=torch.float64)
        if gp is not None:
            gz = gp[sl].double() * z[sl].double()[:, :, None]
            gdv, gdv_abs = gdv + gz.sum(1), gdv_abs + gz.abs().sum(1)
            gov, gov_abs = gov + gp[sl].double().sum(1), gov_abs + gp[sl].double().abs().sum(1)
        if gd is not None:
            gdv, gdv_abs = gdv + gd[sl].double(), gdv_abs + gd[sl].double().abs()
        if go is not None:
            gov, gov_abs = gov + go[sl].double(), gov_abs + go[sl].double().abs()
        G[f, :9] = (gdv[:, :, None] * dirs[:, None, :]).sum(0).reshape(9)
        A[f, :9] = (gdv_abs[:, :, None] * dirs.abs()[:, None, :]).sum(0).reshape(9)
        G[f, 9:] = gov.sum(0)
        A[f, 9:] = gov_abs.sum(0)
    return G, A


def _quat_tables(q):
    """|coefficient| of G[e] in (dr, di, dj, dk) of raygen_bwd_pose_kernel [4, 9], the signed coefficients [4, 9], M [9] of
    R = I + two_s M and the sums of the absolute values of M's two products [9]; q float64 [4]."""
    r, i, j, k = [float(v) for v in q]
    Cs = torch.tensor([[0, -k, j, k, 0, -i, -j, i, 0],
                       [0, j, k, j, -2 * i, -r, k, r, -2 * i],
                       [-2 * j, i, r, i, 0, k, -r, k, -2 * j],
                       [-2 * k, -r, i, r, -2 * k, j, i, j, 0]], dtype=torch.float64)
    M = torch.tensor([-(j * j + k * k), i * j - k * r, i * k + j * r, i * j + k * r, -(i * i + k * k), j * k - i * r,
                      i * k - j * r, j * k + i * r, -(i * i + j * j)], dtype=torch.float64)
    a = abs
    Ma = torch.tensor([j * j + k * k, a(i * j) + a(k * r), a(i * k) + a(j * r), a(i * j) + a(k * r), i * i + k * k,
                       a(j * k) + a(i * r), a(i * k) + a(j * r), a(j * k) + a(i * r), i * i + j * j], dtype=torch.float64)
    return Cs.abs(), Cs, M, Ma


def pose_grad_from_sums(q, G):
    """The quaternion chain rule of raygen_bwd_pose_kernel evaluated in float64 on G [K, 12] -> (d_quat, d_trans): ties the
    coefficient tables the bound uses to autograd (tests/test_raygen_ref.py)."""
    K = q.shape[0]
    dq = torch.zeros(K, 4, dtype=torch.float64)
    for f in range(K):
        qf = q[f].double()
        _, Cs, M, _ = _quat_tables(qf)
        two_s = 2.0 / float((qf * qf).sum())
        dq[f] = two_s * (Cs @ G[f, :9]) - two_s * two_s * float(M @ G[f, :9]) * qf
    return dq, G[:, 9:].clone()


U32 = 2.0 ** -24          # unit roundoff of fp32, round to nearest


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def chain_lengths(npf, S):
    """Longest chains of roundings a term of the 12 sums passes through: (n_T, n_R)."""
    n_part = (npf + 7) // 8
    strided_s = (S + 63) // 64            # the lane-strided loop over a ray's samples
    strided_p = (n_part + 63) // 64       # the lane-strided loop over a frame's workgroups
    n_t = strided_s + 6 + 1 + 2 + 3 + strided_p + 6      # + butterfly + d_rays_o + acc (2 rays) + 4 waves + ... + butterfly
    n_r = n_t + 4                                        # g z, gdv dir, and pixel_dir's subtraction and division
    return n_t, n_r


N_POSE = 27               # longest chain of roundings of a term inside raygen_bwd_pose_kernel (the c q_c path)


def pose_grad_bound(q, idx, window, cam_f32, z, gp, gd, go):
    """|kernel - exact| <= (Bq [K, 4], BT [K, 3]), float64.  With E = gamma(n) A the bound of the 12 sums,
    S_c(X) = two_s sum_e |coef_ce| X_e + two_s^2 |q_c| sum_e Mabs_e X_e:   Bq_c = gamma(N_POSE) S_c(|G| + E) + S_c(E),
    BT_a = gamma(n_T + 1) A_a (the + 1: the += into the output)."""
    K = q.shape[0]
    npf = idx.numel() // K
    S = z.shape[1] if z is not None else 1
    n_t, n_r = chain_lengths(npf, S)
    G, A = pose_sums_f64(idx, window, cam_f32, K, z, gp, gd, go)
    E = torch.cat((gamma(n_r) * A[:, :9], gamma(n_t) * A[:, 9:]), 1)
    Bq = torch.zeros(K, 4, dtype=torch.float64)
    for f in range(K):
        qf = q[f].double()
        Ca, _, _, Ma = _quat_tables(qf)
        two_s = 2.0 / float((qf * qf).sum())
        s_of = lambda X: two_s * (Ca @ X) + two_s * two_s * qf.abs() * float(Ma @ X)
        Bq[f] = gamma(N_POSE) * s_of(G[f, :9].abs() + E[f, :9]) + s_of(E[f, :9])
    return Bq, gamma(n_t + 1) * A[:, 9:]


def bound_ratio(got, want, bound):
    """max |got - want| / bound over the elements; 0 / 0 counts as 0, x / 0 as inf, a non-finite ``got`` as inf."""
    got, want, bound = got.double().cpu(), want.double().cpu(), bound.double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    d = (got - want).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(r.max())


# (K, npf, S, window, which gradients, NULL output, cancel)
BACKWARD_CASES = [
    (1, 1, 1, FULL, "pdo", None, False),
    (1, 1, 1, CROP, "p", None, False),
    (1, 7, 5, CROP, "pdo", None, False),
    (1, 7, 5, FULL, "o", None, False),
    (2, 9, 65, FULL, "p", None, False),
    (2, 9, 65, CROP, "d", None, False),
    (2, 9, 65, CROP, "pdo", "quat", False),
    (1, 64, 47, FULL, "pdo", "trans", False),
    (1, 64, 47, CROP, "p", None, True),
    (3, 515, 3, CROP, "pdo", None, False),
    (3, 515, 3, FULL, "p", None, True),
]


def backward_id(c):
    return f"K{c[0]}x{c[1]}xS{c[2]}-{'crop' if c[3] == CROP else 'full'}-{c[4]}" + (f"-no_{c[5]}" if c[5] else "") + ("-cancel" if c[6] else "")


def backward_case(ci):
    """Inputs of BACKWARD_CASES[ci]: a plain scene on the inexact camera (quaternion norms cycling through 1, 0.5, 3 from the
    case's number), samples nu + ns = S, and the output gradients gp [n, S, 3], gd, go [n, 3] (None where the case leaves one out;
    cancel: gp has zero mean per frame and component)."""
    K, npf, S, window, which, null_out, cancel = BACKWARD_CASES[ci]
    sc = make_scene("plain", K, window, npf, 3000 + ci, CAM_INEXACT, norm_shift=ci)
    g = torch.Generator().manual_seed(4000 + ci)
    nu = S // 2
    ns = S - nu
    n = K * npf
    gp = torch.randn(n, S, 3, generator=g)
    if cancel:
        gp = (gp.reshape(K, npf * S, 3) - gp.reshape(K, npf * S, 3).mean(1, keepdim=True)).reshape(n, S, 3).contiguous()
    gd, go = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    sc.update(nu=nu, ns=ns, K=K, npf=npf, S=S, window=window, cam=CAM_INEXACT, bound=BOUND, depth_max=None,
              t_surf=torch.rand(ns, generator=g), t_zero=torch.rand(ns, generator=g),
              t_uniform=torch.linspace(0.0, 1.0, steps=nu) if nu else None,
              gp=gp if "p" in which else None, gd=gd if "d" in which else None, go=go if "o" in which else None,
              null_out=null_out)
    return sc
