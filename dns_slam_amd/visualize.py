"""Headless visualiser: the reference's ``SLAMFrontend`` (utils/viz.py, driven by visualizer.py) without a window system.

The reference draws the reconstructed mesh, the estimated and ground-truth camera frusta and the two trajectories with open3d's
``Visualizer`` and, with ``--save_rendering``, captures the window once per update.  Here every frame is one call of
``ops.render_mesh`` (csrc/mesh_render.hip): the mesh as shaded triangles, everything else as z-tested points of 4 pixels on a
white background, from the fixed viewer pose of viz.py:166-174.

Not rebuilt: the coordinate-frame axes the reference adds at the origin (viz.py:159), the interactive window (mouse control,
``vis.run()``, the separate process and its queue) and the ffmpeg call that joins the frames into ``vis.mp4``
(visualizer.py:99-102).  Frames are PNG, not JPEG, written by ``write_png`` below (zlib only: neither PIL nor cv2 is needed).
"""
from __future__ import annotations

import math
import os
import struct
import zlib

import numpy as np
import torch

from . import evaluation, ops

CAM_POINTS = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5], [0.5, 1, 1.5], [0, 1.2, 1.5]],
                      np.float64)
CAM_LINES = np.array([[1, 2], [2, 3], [3, 4], [4, 1], [1, 3], [2, 4], [1, 0], [0, 2], [3, 0], [0, 4], [5, 7], [7, 6]])
CAM_LINE_SAMPLES = 100
COLOR_EST, COLOR_GT = (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)
GT_KEY_OFFSET = 100000                                           # viz.py:68: ground-truth actors live beside the estimated ones
Z_FAR = 1000.0                                                   # viz.py:165
MESH_GREY = 0.7                                                  # a mesh without vertex colours


def camera_actor(scale=0.005, is_gt=False):
    """``create_camera_actor`` (viz.py:14-42): the frustum wireframe as a cloud -> (points float64 [1200,3] in the camera's
    frame, colour (r, g, b)): 8 corner points times ``scale``, 12 lines, 100 samples per line (both ends included); red for an
    estimated camera, black for a ground-truth one."""
    pts = scale * CAM_POINTS
    t = np.linspace(0.0, 1.0, CAM_LINE_SAMPLES)
    out = [pts[a][None, :] * (1.0 - t)[:, None] + pts[b][None, :] * t[:, None] for a, b in CAM_LINES]
    return np.concatenate(out), (COLOR_GT if is_gt else COLOR_EST)


def write_png(path, image):
    """uint8 [H,W,3] (or [H,W], grey) -> an 8-bit PNG without interlace, every row with filter type 0."""
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"write_png: a uint8 image [H,W,3] or [H,W], got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.concatenate((np.zeros((H, 1), np.uint8), a.reshape(H, -1)), 1)

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    head = struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", head) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def _pose(p):
    p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
    return np.array(p, dtype=np.float64).reshape(4, 4)


class Frontend:
    """``SLAMFrontend`` with a rasteriser in place of the window: ``update_pose``, ``update_mesh``, ``update_cam_trajectory`` and
    ``reset`` change the scene at once (no queue, no process), ``render()`` draws it -> uint8 [H,W,3] on the host, ``save_frame()``
    writes ``{output}/tmp_rendering/%06d.png`` (numbered from 1, as the reference's captures).

    ``init_pose``: the first camera-to-world pose; the viewer looks through it -- columns 1 and 2 negated, then inverted
    (viz.py:166-174; the step back along the view axis is commented out there and is not taken here).  It is copied, not changed.
    The image is H x W with a vertical field of view of ``fov_deg`` (open3d's default 60), square pixels and the principal point in
    the middle.  ``near`` is the reference's ``set_constant_z_near`` argument: the rasteriser needs z_near > 0, so ``near=0`` (what
    visualizer.py passes) maps to ``ops.render_mesh``'s default z_near of 0.01, any other value is used as it is; z_far is 1000.
    ``estimate_c2w_list`` / ``gt_c2w_list`` [n,4,4]: the poses ``update_cam_trajectory`` draws from.
    The mesh is drawn with ``cull="front"`` on its stored winding -- the reference reverses every face and hides back faces
    (viz.py:96-102, 161) -- and ``shade="headlight"``."""

    def __init__(self, output, init_pose, cam_scale=1, near=0, estimate_c2w_list=None, gt_c2w_list=None, H=720, W=1280, fov_deg=60,
                 device="cuda:0"):
        self.output = str(output)
        self.cam_scale = float(cam_scale)
        self.z_near = 0.01 if float(near) == 0.0 else float(near)
        self.H, self.W = int(H), int(W)
        f = 0.5 * self.H / math.tan(math.radians(float(fov_deg)) / 2.0)
        self.intrinsics = (f, f, self.W / 2.0 - 0.5, self.H / 2.0 - 0.5)
        self.device = torch.device(device)
        self.w2c = torch.from_numpy(evaluation.world_to_camera(_pose(init_pose)[None], flip_yz=True)).to(self.device)
        self.estimate_c2w_list = None if estimate_c2w_list is None else self._poses(estimate_c2w_list)
        self.gt_c2w_list = None if gt_c2w_list is None else self._poses(gt_c2w_list)
        self.cameras = {}                                         # key -> (pose [4,4] float64, is_gt)
        self.traj = {False: None, True: None}                     # is_gt -> float64 [n,3]
        self.mesh = None                                          # (verts, faces, colors) on the device
        self.frame_idx = 0

    @staticmethod
    def _poses(c):
        c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        return np.array(c, dtype=np.float64).reshape(-1, 4, 4)

    def update_pose(self, index, pose, gt=False):
        """The camera actor ``index`` (estimated and ground-truth actors are numbered apart) moves to ``pose`` [4,4] camera-to-world
        with its third column negated (viz.py:192; the reference negates the caller's array in place, this negates a copy)."""
        p = _pose(pose)
        p[:3, 2] *= -1.0
        self.cameras[int(index) + (GT_KEY_OFFSET if gt else 0)] = (p, bool(gt))

    def update_mesh(self, mesh, faces=None, colors=None):
        """``mesh``: the path of a PLY file (``evaluation.read_ply``; vertex colours when it has them), or verts [P,3] with ``faces``
        [F,3] and optional ``colors`` [P,3] (uint8 0..255 or floating point 0..1) as tensors or arrays.  Replaces the mesh."""
        if isinstance(mesh, (str, os.PathLike)):
            m = evaluation.read_ply(mesh)
            mesh, faces, colors = m["verts"], m["faces"], m.get("colors")
        v = torch.as_tensor(mesh).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        f = torch.as_tensor(faces).to(self.device).reshape(-1, 3)
        f = (f if f.dtype in (torch.int32, torch.int64) else f.to(torch.int64)).contiguous()
        if colors is None:
            c = torch.full((v.shape[0], 3), MESH_GREY, dtype=torch.float32, device=self.device)
        else:
            c = torch.as_tensor(colors).to(self.device)
            c = (c.to(torch.float32) / 255.0 if c.dtype == torch.uint8 else c.to(torch.float32)).reshape(-1, 3).contiguous()
        self.mesh = (v, f, c)

    def update_cam_trajectory(self, i, gt):
        """The translations of poses [1:i] of the estimated (``gt`` false) or ground-truth list as points (viz.py:104-125)."""
        poses = self.gt_c2w_list if gt else self.estimate_c2w_list
        if poses is None:
            raise ValueError("update_cam_trajectory: the frontend was made without that pose list")
        self.traj[bool(gt)] = poses[1:int(i), :3, 3].copy()

    def reset(self):
        """Removes the camera actors (viz.py:127-137); the mesh and the trajectories stay."""
        self.cameras = {}

    def scene_points(self):
        """-> (points fp32 [N,3], colours fp32 [N,3]) on the host: the camera actors in ascending key order, then the estimated and
        the ground-truth trajectory."""
        pts, cols = [np.zeros((0, 3))], [np.zeros((0, 3))]
        for key in sorted(self.cameras):
            pose, is_gt = self.cameras[key]
            p, c = camera_actor(self.cam_scale, is_gt)
            pts.append(p @ pose[:3, :3].T + pose[:3, 3])
            cols.append(np.tile(np.asarray(c, np.float64), (len(p), 1)))
        for is_gt in (False, True):
            if self.traj[is_gt] is not None:
                pts.append(self.traj[is_gt])
                cols.append(np.tile(np.asarray(COLOR_GT if is_gt else COLOR_EST, np.float64), (len(self.traj[is_gt]), 1)))
        return np.concatenate(pts).astype(np.float32), np.concatenate(cols).astype(np.float32)

    def render(self):
        """One frame -> uint8 [H,W,3] on the host: colour clamped to [0, 1], times 255, rounded half up."""
        if self.mesh is None:
            v = torch.zeros(0, 3, device=self.device)
            f = torch.zeros(0, 3, dtype=torch.int32, device=self.device)
            c = torch.zeros(0, 3, device=self.device)
        else:
            v, f, c = self.mesh
        p, pc = self.scene_points()
        kw = {}
        if len(p):
            kw = dict(points=torch.from_numpy(p).to(self.device), point_colors=torch.from_numpy(pc).to(self.device))
        out = ops.render_mesh(v, f, c, self.w2c, self.H, self.W, *self.intrinsics, z_near=self.z_near, z_far=Z_FAR, cull="front",
                              shade="headlight", ambient=0.3, background=(1, 1, 1), point_size=4, **kw)
        img = (out["color"][0].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
        return img.cpu().numpy()

    def save_frame(self):
        """Renders and writes the next ``{output}/tmp_rendering/%06d.png`` -> its path."""
        self.frame_idx += 1
        d = os.path.join(self.output, "tmp_rendering")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{self.frame_idx:06d}.png")
        write_png(path, self.render())
        return path
