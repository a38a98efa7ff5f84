"""numpy restatement of the keyframe TSDF fusion behind Mesher.get_bound_from_frames (the reference's slams/meshing.py:380-445,
i.e. Open3D >= 0.13's ScalableTSDFVolume with the reference's parameters): what csrc/tsdf.hip must compute, bit for bit.

Everything is written element-wise in the kernels' operation order -- no ``@``, no BLAS -- so float32 and float64 results are
reproducible.  Stated departures from Open3D (none could be pinned to an Open3D run):
  * Open3D walks z by repeated float additions of a scaled column; every voxel is evaluated directly here.
  * colour is not fused; only vertices are extracted, never faces.
  * the reference negates the pose columns in place on a view that can alias the keyframe's tensor; the keyframes stay unmodified.

``dtype=np.float64`` evaluates the integration in float64 and the ``near`` flags say where float32 may legitimately differ.
"""
import numpy as np

UNIT = 16


def poses(est_c2w):
    """est_c2w [K,4,4] (the keyframes' float32 values) -> (extrinsic E [K,4,4] f64, pose = inv(E) [K,4,4] f64, centres [K,3] f64).
    Columns 1 and 2 of the rotation are negated on a copy (this project's cameras look along -z, Open3D's along +z)."""
    c = np.array(est_c2w, dtype=np.float32).astype(np.float64).reshape(-1, 4, 4).copy()
    c[:, :3, 1] *= -1.0
    c[:, :3, 2] *= -1.0
    K = c.shape[0]
    E = np.stack([np.linalg.inv(c[k]) for k in range(K)]) if K else np.zeros((0, 4, 4))
    P = np.stack([np.linalg.inv(E[k]) for k in range(K)]) if K else np.zeros((0, 4, 4))
    return E, P, c[:, :3, 3].copy()


def multiplier_table(H, W, cam):
    """m [H,W] f32: the camera-distance multiplier sqrt(((u-cx)/fx)^2 + ((v-cy)/fy)^2 + 1), float64 rounded to float32."""
    u = (np.arange(W, dtype=np.float64) - float(cam["cx"])) / float(cam["fx"])
    v = (np.arange(H, dtype=np.float64) - float(cam["cy"])) / float(cam["fy"])
    return np.sqrt((u * u)[None, :] + (v * v)[:, None] + 1.0).astype(np.float32)


def touch(depths, pose, cam, voxel_length, sdf_trunc, stride=4, depth_trunc=1000.0):
    """-> keys [n,4] int64 (ux, uy, uz, frame), sorted lexicographically and unique: the (unit, frame) pairs."""
    depths = np.asarray(depths, np.float32)
    K = depths.shape[0]
    L, tr = UNIT * float(voxel_length), float(sdf_trunc)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    out = []
    for k in range(K):
        d = depths[k, ::stride, ::stride]
        i, j = np.meshgrid(np.arange(0, depths.shape[1], stride), np.arange(0, depths.shape[2], stride), indexing="ij")
        ok = (d > 0) & (d < np.float32(depth_trunc))
        z = d[ok].astype(np.float64)
        x = ((j[ok].astype(np.float64) - cx) * z) / fx
        y = ((i[ok].astype(np.float64) - cy) * z) / fy
        P = pose[k]
        p = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
        lo = [np.floor((p[a] - tr) / L).astype(np.int64) for a in range(3)]
        hi = [np.floor((p[a] + tr) / L).astype(np.int64) for a in range(3)]
        for cxn in range(8):
            sel = [hi[a] if (cxn >> a) & 1 else lo[a] for a in range(3)]
            out.append(np.stack(sel + [np.full_like(sel[0], k)], 1))
    if not out:
        return np.zeros((0, 4), np.int64)
    return np.unique(np.concatenate(out), axis=0)


def fuse(depths, extrinsic, pose, cam, voxel_length, sdf_trunc, stride=4, dtype=np.float32):
    """-> dict(units [B,3] int32 sorted, tsdf [B,16,16,16], weight [B,16,16,16], pairs [n,4], near [B,16,16,16] bool, updates int).
    Frame k is integrated only into the units it touched, in ascending k."""
    ft = dtype
    depths = np.asarray(depths, np.float32)
    K, H, W = depths.shape
    keys = touch(depths, pose, cam, voxel_length, sdf_trunc, stride)
    units, inv = (np.unique(keys[:, :3], axis=0, return_inverse=True) if len(keys) else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64)))
    inv = np.asarray(inv).reshape(-1)
    B = units.shape[0]
    tsdf = np.zeros((B, UNIT, UNIT, UNIT), ft)
    wgt = np.zeros((B, UNIT, UNIT, UNIT), ft)
    near = np.zeros((B, UNIT, UNIT, UNIT), bool)
    vl, L = float(voxel_length), UNIT * float(voxel_length)
    tr = ft(sdf_trunc)
    fx, fy, cx, cy = (ft(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    m = multiplier_table(H, W, cam).astype(ft)
    eps_px = ft(np.float32(1e-4))
    u_hi, v_hi = ft(np.float32(W) - np.float32(1e-4)), ft(np.float32(H) - np.float32(1e-4))
    ax = (np.arange(UNIT, dtype=np.float64) + 0.5) * vl
    one, half = ft(1), ft(0.5)
    n_updates = 0
    for k in range(K):
        ub = inv[keys[:, 3] == k]                                  # ascending unit index
        if ub.size == 0:
            continue
        E = np.asarray(extrinsic[k], np.float64).astype(ft)
        org = units[ub].astype(np.float64) * L                      # [n,3]
        c = [(ax[None, :] + org[:, a:a + 1]).astype(ft) for a in range(3)]
        X, Y, Z = c[0][:, :, None, None], c[1][:, None, :, None], c[2][:, None, None, :]
        cam_p = [((E[a, 0] * X + E[a, 1] * Y) + E[a, 2] * Z) + E[a, 3] for a in range(3)]
        xc, yc, zc = cam_p
        front = zc > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = ((xc * fx) / zc + cx) + half
            v = ((yc * fy) / zc + cy) + half
        inside = front & (u >= eps_px) & (u < u_hi) & (v >= eps_px) & (v < v_hi)
        iu = np.where(inside, u, 0).astype(np.int64)
        iv = np.where(inside, v, 0).astype(np.int64)
        d = depths[k][iv, iu].astype(ft)
        sdf = (d - zc) * m[iv, iu]
        upd = inside & (d > 0) & (sdf > -tr)
        t = np.minimum(one, sdf / tr)
        T, Wt = tsdf[ub], wgt[ub]
        T2 = (T * Wt + t) / (Wt + one)
        tsdf[ub] = np.where(upd, T2, T)
        wgt[ub] = np.where(upd, Wt + one, Wt)
        n_updates += int(upd.sum())
        # where float32 may legitimately decide differently: a projection within 1e-3 px of an integer (the image edges are
        # 1e-4 px from one), an sdf within 1e-4 trunc of -trunc, z_cam within 1e-6 of 0
        with np.errstate(invalid="ignore"):
            nr = (np.abs(zc) < 1e-6) | (front & ((np.abs(u - np.rint(u)) < 1e-3) | (np.abs(v - np.rint(v)) < 1e-3))
                                         & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1))
            nr |= inside & (d > 0) & (np.abs(sdf + tr) < 1e-4 * tr)
        near[ub] |= nr
    return {"units": units.astype(np.int32), "tsdf": tsdf, "weight": wgt, "pairs": keys, "near": near, "updates": n_updates}


def tiles(units, tsdf, weight, sel=None):
    """[n,18,18,18]: the units ``sel`` (default: all) plus one voxel on each side (from the neighbouring units); unobserved or
    missing = NaN."""
    sel = np.arange(units.shape[0]) if sel is None else np.asarray(sel)
    ul = units.tolist()
    index = {tuple(u): b for b, u in enumerate(ul)}
    T = np.full((len(sel), UNIT + 2, UNIT + 2, UNIT + 2), np.nan, tsdf.dtype)
    rng = {-1: ([0], [UNIT - 1]), 0: (list(range(1, UNIT + 1)), list(range(UNIT))), 1: ([UNIT + 1], [0])}   # tile cells, source voxels
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                nb = np.array([index.get((ul[b][0] + dx, ul[b][1] + dy, ul[b][2] + dz), -1) for b in sel], np.int64)
                have = nb >= 0
                if not have.any():
                    continue
                (tx, sx), (ty, sy), (tz, sz) = rng[dx], rng[dy], rng[dz]
                src = nb[have]
                T[np.ix_(np.nonzero(have)[0], tx, ty, tz)] = np.where(weight[np.ix_(src, sx, sy, sz)] > 0, tsdf[np.ix_(src, sx, sy, sz)], np.nan)
    return T


def vertices(units, tsdf, weight, voxel_length, with_cubes=False, block=4096):
    """-> [V,3] f64, ordered by unit, voxel ((x 16 + y) 16 + z), axis.  Voxel a and axis e emit a vertex when a and a+e are
    observed with different ``tsdf < 0`` and one of the four cubes around that edge has eight observed corners.  Evaluated in
    blocks of ``block`` units (memory); ``with_cubes`` also returns the complete-cube flags [B,17,17,17] by base tile position."""
    out, cubes = [np.zeros((0, 3))], []
    for b0 in range(0, units.shape[0], block):
        sel = np.arange(b0, min(b0 + block, units.shape[0]))
        pos, cube = _block_vertices(units, tsdf, weight, float(voxel_length), sel)
        out.append(pos)
        if with_cubes:
            cubes.append(cube)
    pos = np.concatenate(out)
    if with_cubes:
        return pos, (np.concatenate(cubes) if cubes else np.zeros((0, UNIT + 1, UNIT + 1, UNIT + 1), bool))
    return pos


def _block_vertices(units, tsdf, weight, vl, sel):
    B = len(sel)
    T = tiles(units, tsdf, weight, sel)
    ob = ~np.isnan(T)
    n = UNIT + 1
    cube = np.ones((B, n, n, n), bool)                              # base tile position q: corners q + {0,1}^3
    for o in range(8):
        cube &= ob[:, (o & 1):(o & 1) + n, ((o >> 1) & 1):((o >> 1) & 1) + n, ((o >> 2) & 1):((o >> 2) & 1) + n]
    S = slice(1, UNIT + 1)
    A = T[:, S, S, S]
    emit = np.zeros((B, UNIT, UNIT, UNIT, 3), bool)
    frac = np.zeros((B, UNIT, UNIT, UNIT, 3), np.float64)
    for e in range(3):
        sh = [slice(2, UNIT + 2) if a == e else S for a in range(3)]
        Bn = T[:, sh[0], sh[1], sh[2]]
        with np.errstate(invalid="ignore"):
            cross = ob[:, S, S, S] & ob[:, sh[0], sh[1], sh[2]] & ((A < 0) != (Bn < 0))
        e1, e2 = [a for a in range(3) if a != e]
        anyc = np.zeros((B, UNIT, UNIT, UNIT), bool)
        for o1 in (0, 1):
            for o2 in (0, 1):
                off = [0, 0, 0]
                off[e1], off[e2] = o1, o2
                q = [slice(1 - off[a], 1 - off[a] + UNIT) for a in range(3)]   # tile position p - offsets, p = a + 1
                anyc |= cube[:, q[0], q[1], q[2]]
        emit[..., e] = cross & anyc
        fa, fb = np.abs(A.astype(np.float64)), np.abs(Bn.astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            frac[..., e] = (fa * vl) / (fa + fb)
    b, x, y, z, e = np.nonzero(emit)
    loc = np.stack((x, y, z), 1)
    idx = units[sel[b]].astype(np.int64) * UNIT + loc
    pos = 0.5 * vl + vl * idx.astype(np.float64)
    pos[np.arange(len(e)), e] = pos[np.arange(len(e)), e] + frac[b, x, y, z, e]
    return pos, cube


def scene_keyframes(frames, idx, shift=(0.01, 0.0, 0.0)):
    """(est_c2w [K+1,4,4] f32, depths [K+1,H,W] f32) of frames ``idx`` plus keyframe idx[0] a second time with its translation
    shifted: at stride 4 no unit of the synthetic scene is touched by two frames otherwise."""
    c = np.stack([np.asarray(frames["est_c2w"][i], np.float32) for i in idx] + [np.asarray(frames["est_c2w"][idx[0]], np.float32)])
    c = c.copy()
    c[-1, :3, 3] += np.asarray(shift, np.float32)
    d = np.stack([np.asarray(frames["gt_depth"][i], np.float32) for i in idx] + [np.asarray(frames["gt_depth"][idx[0]], np.float32)])
    return c, d
