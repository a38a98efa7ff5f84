"""numpy restatement of ops.keyframe_overlap (include/dns_hip.h, "keyframe overlap"): the float64 arithmetic of csrc/keyframes.hip,
operation for operation, so the kernel's counts are EQUAL to it -- and, beside it, the rule of the reference's
keyframe_selection_overlap (slams/mapping.py:208-226) spelled the reference's way (float32 inverse and camera coordinates, K in
float64), which the restatement is held to away from the image borders (tests/test_keyframe_overlap_ref.py).

Every numpy operation below is one IEEE operation per element (numpy fuses nothing across ufunc calls), which is what the kernel
computes under -ffp-contract=off.  ``strict`` / ``flip`` / ``use_eps`` switch single parts of the rule off: the tests use them to
show that the comparison against the reference rule notices a wrong rule."""
import numpy as np


def inverse_rows(m):
    """m [4,4] (any float dtype) -> (rows 0-2 of inverse(m) as float64 [12], ok): the adjugate from the twelve 2 x 2 minors of rows
    0-1 (s0..s5) and rows 2-3 (c0..c5), every entry divided by the determinant.  ok is False for a non-finite entry or a determinant
    that is 0 or non-finite."""
    a = np.asarray(m, dtype=np.float64)
    ok = bool(np.isfinite(a).all())
    (a00, a01, a02, a03), (a10, a11, a12, a13), (a20, a21, a22, a23), (a30, a31, a32, a33) = a
    with np.errstate(all="ignore"):
        s0, s1, s2 = a00 * a11 - a10 * a01, a00 * a12 - a10 * a02, a00 * a13 - a10 * a03
        s3, s4, s5 = a01 * a12 - a11 * a02, a01 * a13 - a11 * a03, a02 * a13 - a12 * a03
        c0, c1, c2 = a20 * a31 - a30 * a21, a20 * a32 - a30 * a22, a20 * a33 - a30 * a23
        c3, c4, c5 = a21 * a32 - a31 * a22, a21 * a33 - a31 * a23, a22 * a33 - a32 * a23
        det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
        ok = ok and bool(np.isfinite(det)) and det != 0.0
        w = np.array([
            ((a11 * c5 - a12 * c4) + a13 * c3) / det,
            ((a02 * c4 - a01 * c5) - a03 * c3) / det,
            ((a31 * s5 - a32 * s4) + a33 * s3) / det,
            ((a22 * s4 - a21 * s5) - a23 * s3) / det,
            ((a12 * c2 - a10 * c5) - a13 * c1) / det,
            ((a00 * c5 - a02 * c2) + a03 * c1) / det,
            ((a32 * s2 - a30 * s5) - a33 * s1) / det,
            ((a20 * s5 - a22 * s2) + a23 * s1) / det,
            ((a10 * c4 - a11 * c2) + a13 * c0) / det,
            ((a01 * c2 - a00 * c4) - a03 * c0) / det,
            ((a30 * s4 - a31 * s2) + a33 * s0) / det,
            ((a21 * s2 - a20 * s4) - a23 * s0) / det], dtype=np.float64)
    return w, ok


def project(points, c2w, fx, fy, cx, cy, eps=1e-5, flip=True, use_eps=True):
    """One keyframe: points fp32 [P,3], c2w fp32 [4,4] -> (u, v float64 [P] before the fp32 rounding, ze float64 [P], ok)."""
    w, ok = inverse_rows(c2w)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    fx, fy, cx, cy, eps = (np.float64(t) for t in (fx, fy, cx, cy, eps))
    with np.errstate(all="ignore"):
        xc = ((w[0] * x + w[1] * y) + w[2] * z) + w[3]
        if flip:
            xc = -xc
        yc = ((w[4] * x + w[5] * y) + w[6] * z) + w[7]
        zc = ((w[8] * x + w[9] * y) + w[10] * z) + w[11]
        ze = zc + eps if use_eps else zc
        u = (fx * xc + cx * zc) / ze
        v = (fy * yc + cy * zc) / ze
    return u, v, ze, ok


def overlap_counts(points, c2w, H, W, fx, fy, cx, cy, edge=10, eps=1e-5, strict=True, flip=True, use_eps=True):
    """points fp32 [P,3], c2w fp32 [n,4,4] -> int32 [n]: what ops.keyframe_overlap returns."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    c2w = np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4)
    out = np.zeros(len(c2w), dtype=np.int32)
    if len(points) == 0:
        return out
    finite = np.isfinite(points).all(axis=1)
    lo, u_hi, v_hi = np.float32(edge), np.float32(W - edge), np.float32(H - edge)
    for k, m in enumerate(c2w):
        u, v, ze, ok = project(points, m, fx, fy, cx, cy, eps, flip, use_eps)
        if not ok:
            continue
        with np.errstate(all="ignore"):
            u, v = u.astype(np.float32), v.astype(np.float32)
            if strict:
                inside = (u < u_hi) & (u > lo) & (v < v_hi) & (v > lo) & (ze < 0.0)
            else:
                inside = (u <= u_hi) & (u >= lo) & (v <= v_hi) & (v >= lo) & (ze < 0.0)
        out[k] = int((inside & finite).sum())
    return out


def reference_rule(points, c2w, H, W, fx, fy, cx, cy, edge=10):
    """The reference's rule in its own number formats (slams/mapping.py:208-226): float32 inverse of the float32 pose, float32 camera
    coordinates, K applied in float64, + 1e-5, the quotient rounded to fp32, five strict comparisons.
    -> (counts int64 [n], u float64 [n,P], v float64 [n,P]) with u, v as they stand before the fp32 rounding."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    c2w = np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4)
    homo = np.concatenate([points, np.ones((len(points), 1), dtype=np.float32)], axis=1)[:, :, None]      # [P,4,1] fp32
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    counts, us, vs = [], [], []
    for m in c2w:
        cam = (np.linalg.inv(m) @ homo)[:, :3]                    # fp32 [P,3,1]
        cam[:, 0] *= -1
        uvz = K @ cam                                             # float64
        z = uvz[:, 2:] + 1e-5
        uv = uvz[:, :2] / z
        uv32 = uv.astype(np.float32)
        inside = (uv32[:, 0] < W - edge) & (uv32[:, 0] > edge) & (uv32[:, 1] < H - edge) & (uv32[:, 1] > edge) & (z[:, 0] < 0)
        counts.append(int(inside.sum()))
        us.append(uv[:, 0, 0]), vs.append(uv[:, 1, 0])
    return np.array(counts, dtype=np.int64), np.array(us), np.array(vs)


def near_border(u, v, H, W, edge=10, margin=0.01):
    """u, v [n,P] -> bool [P]: the point projects within ``margin`` pixels of one of the four borders in some keyframe."""
    with np.errstate(all="ignore"):
        near = (np.abs(u - edge) < margin) | (np.abs(u - (W - edge)) < margin) | (np.abs(v - edge) < margin) | \
               (np.abs(v - (H - edge)) < margin)
    return near.any(axis=0)


def margin_filter(points, c2w, H, W, fx, fy, cx, cy, edge=10, margin=0.01):
    """Removes the points that EITHER spelling projects within ``margin`` px of a border (in any keyframe) -> (kept points, number
    removed).  Away from the borders the float32 and float64 spellings must count the same points."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    _, u32, v32 = reference_rule(points, c2w, H, W, fx, fy, cx, cy, edge)
    uv64 = [project(points, m, fx, fy, cx, cy)[:2] for m in np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4)]
    u64, v64 = np.array([t[0] for t in uv64]), np.array([t[1] for t in uv64])
    drop = near_border(u32, v32, H, W, edge, margin) | near_border(u64, v64, H, W, edge, margin)
    return points[~drop], int(drop.sum())


def circle_poses(n, centre=(0.0, 0.0, 0.0), radius=1.0, phase=0.3):
    """n camera-to-world poses fp32 [n,4,4] on a horizontal circle, looking outward along -z of the camera, y up (world z up)."""
    out = np.zeros((n, 4, 4), dtype=np.float64)
    for i in range(n):
        th = 2.0 * np.pi * i / n + phase
        look = np.array([np.cos(th), np.sin(th), 0.0])
        x = np.cross(look, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        z = -look
        y = np.cross(z, x)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2] = x, y, z
        out[i, :3, 3] = np.asarray(centre) + radius * look
        out[i, 3, 3] = 1.0
    return out.astype(np.float32)


def box_points(P, seed, half=4.0, centre=(0.0, 0.0, 0.0)):
    """P points fp32 uniform in the cube of half side ``half`` around ``centre``."""
    rng = np.random.default_rng(seed)
    return (np.asarray(centre) + rng.uniform(-half, half, size=(P, 3))).astype(np.float32)


CAM = dict(H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5)       # the issue's test camera
