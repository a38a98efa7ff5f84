"""Torch restatement of the reference's ``Mesher.point_masks`` (slams/meshing.py:124-291), line by line: the per-chunk loop, the
per-keyframe matmuls, the in-place x flip and normalisation, ``F.grid_sample`` and the chunk's ``torch.max``.  Runs on any device
and in float32 (the reference's arithmetic) or float64.

Besides the three masks it returns ``near``: the points some keyframe puts within rounding distance of one of its decisions --
  within 1e-3 px of an image edge, or within 1e-2 px of an edge of the image widened by 1000 px (both with z < 0);
  inside the widened image, within 1e-4 * limit of the depth limit (1.2 max depth, or the chunk's maximum sample);
  inside the image, within 1e-4 * (1 + ds) of either threshold of the depth test.
A kernel that evaluates the same formulas in another order may differ from this file at those points and at no others.
"""
import math

import torch
import torch.nn.functional as F


def point_masks_ref(points, w2c, cam, H, W, *, max_depth=None, depths=None, chunk=None, dtype=torch.float32):
    """points [P,3], w2c [K,4,4] (the world->camera matrices the reference forms per keyframe / frame), cam {'fx','fy','cx','cy'}.
    Mode as in ``ops.point_masks``: neither option = the get_mask_use_all_frames branch (:164-201); ``max_depth`` [K] (the maximum
    of each keyframe's gt_depth) = :257-271; ``depths`` [K,H,W] with ``chunk`` (points_batch_size) = the depth test (:229-255).
    -> (seen, forecast, unseen, near), bool [P]."""
    device = points.device
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    Kmat = torch.tensor([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]], dtype=torch.float64, device=device).to(dtype)
    P = points.shape[0]
    batch = P if chunk is None else int(chunk)
    seen_l, fore_l, unseen_l, near_l = [], [], [], []
    for i in range(math.ceil(P / batch) if P else 0):
        pts = points[i * batch:min((i + 1) * batch, P), :].to(dtype)
        seen_mask = torch.zeros(pts.shape[0], dtype=torch.bool, device=device)
        forecast_mask = torch.zeros(pts.shape[0], dtype=torch.bool, device=device)
        near = torch.zeros(pts.shape[0], dtype=torch.bool, device=device)
        for k in range(w2c.shape[0]):
            m = w2c[k].to(dtype)
            ones = torch.ones_like(pts[:, 0]).reshape(-1, 1)
            homo_points = torch.cat([pts, ones], dim=1).reshape(-1, 4, 1)
            cam_cord_homo = m @ homo_points
            cam_cord = cam_cord_homo[:, :3]
            cam_cord[:, 0] *= -1
            uv = Kmat @ cam_cord
            z = uv[:, -1:] + 1e-8
            uv = uv[:, :2] / z
            edge = 0
            cur_seen = (uv[:, 0] < W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < H - edge) & (uv[:, 1] > edge)
            cur_seen = (cur_seen & (z[:, :, 0] < 0)).reshape(-1)
            edge = -1000
            cur_fore = (uv[:, 0] < W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < H - edge) & (uv[:, 1] > edge)
            cur_fore = (cur_fore & (z[:, :, 0] < 0)).reshape(-1)
            u, v = uv[:, 0, 0].clone(), uv[:, 1, 0].clone()
            front = z[:, 0, 0] < 0
            near |= front & ((u.abs() < 1e-3) | ((u - W).abs() < 1e-3) | (v.abs() < 1e-3) | ((v - H).abs() < 1e-3) |
                             ((u + 1000).abs() < 1e-2) | ((u - W - 1000).abs() < 1e-2) |
                             ((v + 1000).abs() < 1e-2) | ((v - H - 1000).abs() < 1e-2))
            dz = -cam_cord[:, 2, 0]
            if depths is not None:
                gt_depth = depths[k].to(dtype).reshape(1, 1, H, W)
                vgrid = uv.reshape(1, 1, -1, 2)
                vgrid[..., 0] = (vgrid[..., 0] / (W - 1) * 2.0 - 1.0)
                vgrid[..., 1] = (vgrid[..., 1] / (H - 1) * 2.0 - 1.0)
                depth_sample = F.grid_sample(gt_depth, vgrid, padding_mode='zeros', align_corners=True).reshape(-1)
                md = torch.max(depth_sample)
                cur_fore[cur_fore.clone()] &= dz[cur_fore] < md
                near |= cur_seen & (((dz - (depth_sample + 0.1)).abs() < 1e-4 * (1 + depth_sample)) |
                                    ((dz - (depth_sample - 2.5)).abs() < 1e-4 * (1 + depth_sample)))
                cur_seen[cur_seen.clone()] &= (dz[cur_seen] < depth_sample[cur_seen] + 0.1) & (depth_sample[cur_seen] - 2.5 < dz[cur_seen])
            elif max_depth is not None:
                md = max_depth[k].to(dtype) * 1.2
                cur_fore[cur_fore.clone()] &= dz[cur_fore] < md
                cur_seen[cur_seen.clone()] &= dz[cur_seen] < md
            if depths is not None or max_depth is not None:
                inside = front & (u < W + 1000) & (u > -1000) & (v < H + 1000) & (v > -1000)
                near |= inside & ((dz - md).abs() < 1e-4 * md)
            seen_mask |= cur_seen
            forecast_mask |= cur_fore
        forecast_mask &= ~seen_mask
        unseen_mask = ~(seen_mask | forecast_mask)
        seen_l.append(seen_mask), fore_l.append(forecast_mask), unseen_l.append(unseen_mask), near_l.append(near)
    if not seen_l:
        e = torch.zeros(0, dtype=torch.bool, device=device)
        return e, e.clone(), e.clone(), e.clone()
    return torch.cat(seen_l), torch.cat(fore_l), torch.cat(unseen_l), torch.cat(near_l)


def classes(seen, forecast):
    """The masks as ``ops.point_masks`` numbers them: 0 unseen, 1 seen, 2 forecast."""
    return seen.to(torch.uint8) + 2 * forecast.to(torch.uint8)


def scene_points(bound, P, seed=5):
    """P points uniform in the bound widened by 10 % of its extent on every side (host tensor): the recipe of
    test_gpu_mesh.py::test_keyframe_project_matches_reference_loops."""
    g = torch.Generator().manual_seed(seed)
    b = bound.float()
    return (torch.rand(P, 3, generator=g) * 1.2 - 0.1) * (b[:, 1] - b[:, 0]) + b[:, 0]


def hand_made():
    """Seven points in front of one camera at the origin (c2w = identity: it looks along -z, x right, y up) with an 80 x 60 image,
    fx = fy = 60: a wall at depth 2 that is 4 deep in the columns from 70 on.  -> (points, w2c, cam, H, W, depths [1,H,W],
    max_depth [1], expected): ``expected`` maps a mode to the classes (0 unseen, 1 seen, 2 forecast) worked out by hand:
      0 on the optical axis 1 m in front of the wall   1 on the wall   2 on the axis 1 m behind the wall
      3 in front of the deep patch, at 3.9             4 five pixels right of the image (inside the 1000 px band), at 1
      5 behind the camera                              6 on the axis at 5, beyond 1.2 x the largest depth
    Depth test with one chunk of 7: the chunk's largest sample is 4 (point 3), so point 2 (at 3) is forecast; with chunks of 3 the
    first chunk samples only the wall at 2, and point 2 is unseen -- the reference's dependence on points_batch_size."""
    H, W = 60, 80
    cam = {"fx": 60.0, "fy": 60.0, "cx": 39.5, "cy": 29.5}
    depths = torch.full((1, H, W), 2.0)
    depths[:, :, 70:] = 4.0
    pts = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -2.0], [0.0, 0.0, -3.0], [35.5 * 3.9 / 60.0, 0.0, -3.9],
                        [45.5 / 60.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -5.0]])
    expected = {"frustum": [1, 1, 1, 1, 2, 0, 1], "limit": [1, 1, 1, 1, 2, 0, 0],
                "test_chunk7": [1, 1, 2, 1, 2, 0, 0], "test_chunk3": [1, 1, 0, 1, 2, 0, 0]}
    return pts, torch.eye(4)[None], cam, H, W, depths, torch.tensor([4.0]), expected


def hand_made_modes(depths, max_depth):
    """mode name of ``hand_made``'s expectations -> the keyword arguments that select it"""
    return {"frustum": {}, "limit": {"max_depth": max_depth}, "test_chunk7": {"depths": depths, "chunk": 7},
            "test_chunk3": {"depths": depths, "chunk": 3}}
