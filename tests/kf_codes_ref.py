"""Torch restatement of the reference's get_2d_feature (slams/meshing.py:311-377), statement by statement: the loop over the
keyframes, the projection, the rounded pixel, the truncation mask against the keyframe's depth, the stem map up-sampled to full
resolution with F.interpolate(align_corners=True) and indexed at the pixel, Merge on one view, the masked accumulation and the
final division.  Runs on whatever device the points live on.  Besides the reference's two results it returns the count, the
dense [K, P] mask of the (keyframe, point) pairs that contribute, and a flag of the points whose membership in that mask hangs
on a rounding of the projection."""
import torch
import torch.nn.functional as F


def get_2d_feature(points, keyframe_dict, cam, encoder, merge_fn, hidden_dim):
    """points [P,3]; keyframe_dict: list of {'est_c2w' [4,4], 'gt_color' [H,W,3], 'gt_label' [H,W], 'gt_depth' [H,W]};
    cam {'H','W','fx','fy','cx','cy'}; encoder(images [1,1,H,W,3]) -> [1,1,C,h,w]; merge_fn(refer_p [1,n,3], refer_o [1,3],
    ft [1,n,C]) -> [n, hidden_dim].
    -> (pixel_pts [P, hidden_dim], label_pts [P], count_pts [P], mask [K,P] bool, near [P] bool).

    near: for some keyframe with z < 0 the point projects within 1e-3 px of a rounding boundary (u or v at .5) or of an image
    edge, or its depth lies within 1e-5 * depth of one of the two truncation limits."""
    dev = points.device
    H, W = int(cam["H"]), int(cam["W"])
    K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]], device=dev)
    P = points.shape[0]
    pixel_pts = torch.zeros(P, hidden_dim, device=dev)
    label_pts = torch.zeros(P, device=dev)
    count_pts = torch.zeros(P, device=dev)
    mask = torch.zeros(len(keyframe_dict), P, dtype=torch.bool, device=dev)
    near = torch.zeros(P, dtype=torch.bool, device=dev)
    for k, keyframe in enumerate(keyframe_dict):
        c2w = torch.as_tensor(keyframe["est_c2w"]).to(dev)
        color = torch.as_tensor(keyframe["gt_color"]).to(dev)
        label = torch.as_tensor(keyframe["gt_label"]).to(dev)
        depth = torch.as_tensor(keyframe["gt_depth"]).to(dev)
        w2c = torch.inverse(c2w).float()
        ones = torch.ones_like(points[:, 0]).reshape(-1, 1)
        homo_points = torch.cat([points, ones], dim=1).reshape(-1, 4, 1).float()
        cam_cord = (w2c @ homo_points)[:, :3]
        cam_cord[:, 0] *= -1
        uv = K.float() @ cam_cord.float()
        z = uv[:, -1:] + 1e-8
        uv = (uv[:, :2] / z).float()
        cur_mask_seen = (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
        cur_mask_seen = (cur_mask_seen & (z[:, :, 0] < 0)).reshape(-1)

        # ---- the flag (not part of the reference): every point in front of this keyframe, at its own rounded pixel
        u, v, zz = uv[:, 0, 0], uv[:, 1, 0], z[:, 0, 0]
        fin = torch.isfinite(u) & torch.isfinite(v)
        iu = torch.round(torch.where(fin, u, torch.zeros_like(u))).to(torch.int64).clamp(0, W - 1)
        iv = torch.round(torch.where(fin, v, torch.zeros_like(v))).to(torch.int64).clamp(0, H - 1)
        d_all = depth.float()[iv, iu]
        dp_all = -zz
        near |= (zz < 0) & (((u - u.floor() - 0.5).abs() < 1e-3) | ((v - v.floor() - 0.5).abs() < 1e-3) |
                            (u.abs() < 1e-3) | ((u - W).abs() < 1e-3) | (v.abs() < 1e-3) | ((v - H).abs() < 1e-3) |
                            ((dp_all - d_all * 0.95).abs() < 1e-5 * d_all) | ((dp_all - d_all * 1.05).abs() < 1e-5 * d_all))

        uv_ = uv[cur_mask_seen, :, 0]
        p = points[cur_mask_seen, :]
        if uv_.numel() != 0:
            uv_ = torch.round(uv_).to(torch.int64)
            uv_[:, 0] = uv_[:, 0].clamp(0, W - 1)
            uv_[:, 1] = uv_[:, 1].clamp(0, H - 1)
            label_seen = label[uv_[:, 1], uv_[:, 0]]
            depth_seen = depth[uv_[:, 1], uv_[:, 0]]
            depth_proj = -z[cur_mask_seen].reshape(-1)
            front_mask = torch.where(depth_proj < (depth_seen * 0.95), torch.ones_like(depth_seen), torch.zeros_like(depth_seen))
            back_mask = torch.where(depth_proj > (depth_seen * 1.05), torch.ones_like(depth_seen), torch.zeros_like(depth_seen))
            trunc_mask = (1.0 - front_mask) * (1.0 - back_mask)

            features = encoder(color.unsqueeze(0).unsqueeze(0))
            features = F.interpolate(features[0], size=[H, W], mode="bilinear", align_corners=True)
            ft = features[0, :, uv_[:, 1], uv_[:, 0]].permute(1, 0).unsqueeze(0)

            refer_o = c2w[:3, 3].unsqueeze(0).float()
            refer_p = p[None, :, :].clone() - refer_o[:, None, :]
            code_pts = merge_fn(refer_p, refer_o, ft)
            code_pts = code_pts * trunc_mask[..., None]
            count_ = torch.ones_like(trunc_mask) * trunc_mask

            count_pts[cur_mask_seen] += count_
            pixel_pts[cur_mask_seen, :] += code_pts.float()
            label_pts[cur_mask_seen] = label_seen.float()
            mask[k, cur_mask_seen] = trunc_mask > 0
    pixel_pts[count_pts > 0, :] = pixel_pts[count_pts > 0, :] / count_pts[count_pts > 0, None]
    return pixel_pts, label_pts, count_pts, mask, near


def pair_count_loops(points, keyframe_dict, cam):
    """The number of contributing keyframes of every point ([P] int64) by a plain double loop over numpy fp32 scalars, one
    rounding per operation: a check of the restatement's mask that shares none of its indexing."""
    import numpy as np
    f = np.float32
    H, W = int(cam["H"]), int(cam["W"])
    fx, fy, cx, cy = (f(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    pts = points.cpu().numpy().astype(np.float32)
    total = np.zeros(len(pts), np.int64)
    for keyframe in keyframe_dict:
        w2c = torch.inverse(torch.as_tensor(keyframe["est_c2w"])).float().numpy()
        depth = torch.as_tensor(keyframe["gt_depth"]).float().numpy()
        for i_p, (x, y, zc) in enumerate(pts):
            c = [f(f(f(w2c[i, 0] * x + w2c[i, 1] * y) + w2c[i, 2] * zc) + w2c[i, 3]) for i in range(3)]
            c[0] = -c[0]
            z = f(c[2] + f(1e-8))
            if not z < 0:
                continue
            u = f(f(fx * c[0] + cx * c[2]) / z)
            v = f(f(fy * c[1] + cy * c[2]) / z)
            if not (0 < u < W and 0 < v < H):
                continue
            iu = min(max(int(np.rint(u)), 0), W - 1)
            iv = min(max(int(np.rint(v)), 0), H - 1)
            d = depth[iv, iu]
            dp = -z
            if dp < f(d * f(0.95)) or dp > f(d * f(1.05)):
                continue
            total[i_p] += 1
    return torch.from_numpy(total)


def mixed_points(n, keyframe_dict, cam, bound, generator, pad=0.05, jitter=0.1):
    """n points inside the bound padded by ``pad`` of its extent: half drawn uniformly, half near the surfaces the keyframes
    see -- a random pixel of a random keyframe (sub-pixel position uniform in the pixel) back-projected at its depth times
    1 + U(-jitter, jitter), replaced by a uniform draw where it falls outside the padded bound.  Uniform points alone rarely
    fall into a keyframe's +-5 % truncation band; mesh vertices, which the codes are computed for, lie on the surfaces."""
    b = bound.float()
    ext = b[:, 1] - b[:, 0]
    n_u = n // 2
    uni = (torch.rand(n_u, 3, generator=generator) * (1 + 2 * pad) - pad) * ext + b[:, 0]
    H, W = int(cam["H"]), int(cam["W"])
    m = n - n_u
    k = torch.randint(0, len(keyframe_dict), (m,), generator=generator)
    iv = torch.randint(0, H, (m,), generator=generator)
    iu = torch.randint(0, W, (m,), generator=generator)
    sub = torch.rand(m, 2, generator=generator) - 0.5
    scale = 1 + (torch.rand(m, generator=generator) * 2 - 1) * jitter
    depth = torch.stack([torch.as_tensor(kf["gt_depth"]).float() for kf in keyframe_dict])[k, iv, iu]
    depth = torch.where(depth > 0, depth, torch.ones_like(depth)) * scale
    c2w = torch.stack([torch.as_tensor(kf["est_c2w"]).float() for kf in keyframe_dict])[k]
    Z = -depth
    X = (iu + sub[:, 0] - cam["cx"]) * Z / cam["fx"]              # the flipped camera x of the reference's projection
    Y = (iv + sub[:, 1] - cam["cy"]) * Z / cam["fy"]
    local = torch.stack((-X, Y, Z, torch.ones_like(Z)), 1)
    world = (c2w @ local[:, :, None])[:, :3, 0]
    lo, hi = b[:, 0] - pad * ext, b[:, 1] + pad * ext
    outside = ((world < lo) | (world > hi)).any(1)                # (a surface seen beyond the padded bound: a uniform draw instead)
    world[outside] = ((torch.rand(m, 3, generator=generator) * (1 + 2 * pad) - pad) * ext + b[:, 0])[outside]
    return torch.cat((uni, world))[torch.randperm(n, generator=generator)].contiguous()
