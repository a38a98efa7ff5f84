"""Semantic mesh extraction: reference ``Mesher`` (slams/meshing.py:17-784) on this package's mapper.

The grid query, the keyframe projection, marching cubes and the connected-components filter run on the GPU (csrc/mesh.hip,
csrc/mesh_cc.hip, ``Mapper.eval_occupancy``); the reference's host-side numpy / skimage / trimesh steps have no counterpart
here beyond the binary PLY writer below.

A mapper trained with stem features (``mapper.encoder`` set) is meshed with ``stem=``: the vertex query then feeds the colour and
logit networks get_2d_feature's keyframe codes (meshing.py:311-377; csrc/mesh_feature.hip, ``ops.keyframe_codes``).  The
geometry needs no codes -- the occupancy is the coarse / fine network's, which reads only the point encoding -- so the grid
pass, marching cubes, cleaning and the component filter are the same with and without ``stem``.

``Mesher.point_masks`` is the reference's split of points into seen / forecast / unseen (meshing.py:124-291; csrc/mesh_masks.hip,
``ops.point_masks``) with its depth test and its all-frames branch; ``forecast=True`` is the reference's ``show_forecast`` mesh
(fine decoders on the seen part of the grid, the coarse network on the forecast band, -100 elsewhere) and ``depth_test=True`` its
``meshing.depth_test`` cleaning.

``Mesher.get_bound_from_frames`` is the reference's scene bound (meshing.py:380-445): the keyframes' depth images fused into a TSDF
(csrc/tsdf.hip, ``ops.tsdf_fuse`` / ``ops.tsdf_vertices``), the convex hull of its vertices and the camera centres (csrc/hull.hip,
``ops.convex_hull``), scaled by ``clean_mesh_bound_scale``; ``bound_planes="frames"`` hands it to the forecast mesh's cleaning.

``Mesher.fill_holes`` and the ``holes=`` keyword are the reference's ``mesh.fill_holes()`` (meshing.py:770, trimesh's
``repair.fill_holes``; csrc/mesh_holes.hip, ``ops.mesh_fill_holes``): the boundary loops of three and four edges closed with faces
wound against their neighbours, in an order that is a function of the mesh alone.
"""
from __future__ import annotations

import collections
import os

import numpy as np
import torch

from . import ops


Bound = collections.namedtuple("Bound", "verts faces planes")
Bound.__doc__ = """Mesher.get_bound_from_frames: verts [h,3] float64 (the scaled hull's vertices), faces [F,3] int64 into verts (outward
orientation), planes [F,4] float64 (unit outward n, d; inside is n . x + d <= 0: what ``inside_planes`` consumes)."""


def open3d_poses(keyframe_dict):
    """The keyframes' poses as the reference hands them to Open3D (meshing.py:409-414), on the host in float64: est_c2w keeps its
    float32 values, columns 1 and 2 of the rotation are negated (this project's cameras look along -z, Open3D's along +z) -- on a
    COPY: the reference negates in place on a view that can alias the keyframe's own CPU tensor --, the extrinsic is its inverse
    and the back-projection pose the inverse of that.  -> (extrinsic [K,4,4], pose [K,4,4], centres [K,3]), numpy float64."""
    K = len(keyframe_dict)
    c = np.zeros((K, 4, 4), np.float64)
    for k, kf in enumerate(keyframe_dict):
        c[k] = torch.as_tensor(kf["est_c2w"]).detach().cpu().numpy().astype(np.float32).astype(np.float64)
    c[:, :3, 1] *= -1.0
    c[:, :3, 2] *= -1.0
    ext = np.stack([np.linalg.inv(c[k]) for k in range(K)]) if K else np.zeros((0, 4, 4))
    pose = np.stack([np.linalg.inv(ext[k]) for k in range(K)]) if K else np.zeros((0, 4, 4))
    return ext, pose, c[:, :3, 3].copy()


class Mesher:
    """``Mesher(cfg, slam)`` of the reference for one ``mapping.Mapper``.  Reads ``cfg['meshing']`` (resolution, level_set,
    points_batch_size, clean_mesh, clean_mesh_bound_scale (default 1.02), remove_small_geometry_threshold), ``cfg['scale']`` (default 1) and
    ``cfg['back_end']['marching_cubes_bound']`` (default: the mapper's bound).

    The reference always filters the cleaned mesh by connected components; here that is asked for per call: a reference config
    with ``clean_mesh: True`` maps onto ``get_mesh(..., components="small")`` (threshold ``remove_small_geometry_threshold *
    scale * scale``), one with ``get_largest_components: True`` onto ``components="largest"``."""

    def __init__(self, cfg: dict, mapper):
        m = cfg["meshing"]
        self.mapper = mapper
        self.device = mapper.device
        self.resolution = int(m["resolution"])
        self.level_set = float(m["level_set"])
        self.points_batch_size = int(m["points_batch_size"])
        self.clean_mesh = bool(m.get("clean_mesh", True))
        self.clean_mesh_bound_scale = float(m.get("clean_mesh_bound_scale", 1.02))
        self.scale = float(cfg.get("scale", 1))
        thr = m.get("remove_small_geometry_threshold")
        self.remove_small_geometry_threshold = None if thr is None else float(thr)
        if m.get("depth_test", False):
            raise NotImplementedError("Mesher: depth_test in the config is not read; pass depth_test=True to get_mesh / extract / "
                                      "point_masks")
        if m.get("get_largest_components", False):
            raise NotImplementedError("Mesher: get_largest_components in the config is not read; pass components=\"largest\" to "
                                      "get_mesh / extract")
        mcb = cfg.get("back_end", {}).get("marching_cubes_bound")
        self.marching_cubes_bound = (np.array(mcb, dtype=np.float64) * self.scale if mcb is not None
                                     else mapper.bound.detach().cpu().numpy().astype(np.float64))
        self.cam = {"fx": mapper.fx, "fy": mapper.fy, "cx": mapper.cx, "cy": mapper.cy}

    # ------------------------------------------------------------------ meshing.py:535-559
    def get_grid_uniform(self, resolution=None):
        """The axes of the query grid: float64 linspace over the bound padded by 0.05, ``resolution`` samples per axis.  The
        points themselves are made on the device per chunk (``grid_points``), in the reference's meshgrid order."""
        n = self.resolution if resolution is None else int(resolution)
        b, pad = self.marching_cubes_bound, 0.05
        return {"xyz": [np.linspace(b[a][0] - pad, b[a][1] + pad, n) for a in range(3)]}

    def grid_points(self, xyz, s0, s1=None):
        """Points s0..s1 of the reference's flattened meshgrid (indexing 'xy': point (j nx + i) nz + k = (x_i, y_j, z_k)),
        fp32 as ``torch.tensor(..., dtype=torch.float)`` rounds them.  Without ``s1``, ``s0`` is an int64 tensor of point numbers."""
        x, y, z = (torch.tensor(a, dtype=torch.float64, device=self.device).float() for a in xyz)
        nx, nz = x.numel(), z.numel()
        n = torch.arange(s0, s1, device=self.device) if s1 is not None else s0
        return torch.stack((x[(n // nz) % nx], y[n // (nx * nz)], z[n % nz]), 1)

    def _keyframes(self, keyframe_dict, stem=None):
        """(w2c, labels, max_depth) of the keyframes; with ``stem`` additionally (depths [K,H,W], origins [K,3], maps), what
        ``ops.keyframe_codes`` reads.  ``maps`` holds ``stem`` and, for ``stem=True``, the keyframes: the [K,h,w,C] stack is
        computed by ``_stem_maps`` when the vertex query first asks for it, not ahead of the grid pass, which never reads it."""
        dev = self.device
        c2w = torch.stack([torch.as_tensor(kf["est_c2w"]).to(dev) for kf in keyframe_dict])
        w2c = torch.inverse(c2w).float()                                     # meshing.py:208,319
        labels = torch.stack([torch.as_tensor(kf["gt_label"]).to(dev).float() for kf in keyframe_dict])
        if stem is None:
            max_depth = torch.stack([torch.as_tensor(kf["gt_depth"]).to(dev).float().max() for kf in keyframe_dict])
            return w2c, labels, max_depth
        if stem is not True and not (isinstance(stem, torch.Tensor) and stem.dim() == 4 and stem.shape[0] == len(keyframe_dict)):
            raise ValueError("Mesher: stem must be True or the [K,h,w,C] stack of the keyframes' stem maps "
                             "(Mesher.keyframe_stem)")
        if stem is True and getattr(self.mapper, "encoder", None) is None:
            raise ValueError("Mesher: stem=True needs mapper.encoder; pass the maps of Mesher.keyframe_stem(..., encoder=) instead")
        depths = torch.stack([torch.as_tensor(kf["gt_depth"]).to(dev).float() for kf in keyframe_dict])
        max_depth = depths.reshape(depths.shape[0], -1).max(1).values
        origins = c2w[:, :3, 3].float().contiguous()                         # refer_o, meshing.py:363
        return w2c, labels, max_depth, depths, origins, {"stem": stem, "keyframes": keyframe_dict}

    def _stem_maps(self, maps):
        """The [K,h,w,C] stack behind the last entry of ``_keyframes(keyframe_dict, stem)``; ``stem=True`` runs the stem here,
        once per bundle."""
        if maps["stem"] is True:
            maps["stem"] = self.keyframe_stem(maps["keyframes"])
        return maps["stem"].to(self.device)

    def _check_supported(self, stem=None):
        if stem is None and getattr(self.mapper, "encoder", None) is not None:
            raise NotImplementedError("Mesher: a mapper with stem features (mapper.encoder set) needs get_2d_feature's 2-D codes "
                                      "through Merge; pass stem=True (or stem= the maps of Mesher.keyframe_stem) to compute them")

    def _mask_args(self, keyframe_dict, all_frames=None, depth_test=False, depths=None):
        """The mode of ``ops.point_masks`` for one extraction, as its keyword arguments (w2c included): the all-frames branch
        (``all_frames = (estimate_c2w_list, idx)``: poses 0 .. idx, inverted in float64 as meshing.py:166-168 do), the depth test
        against ``depths`` or the keyframes' gt_depth in chunks of points_batch_size, or the depth limit."""
        dev = self.device
        if all_frames is not None:
            est, idx = all_frames
            if est is None or idx is None:
                raise ValueError("Mesher: all_frames is (estimate_c2w_list, idx)")
            c2w = torch.as_tensor(est)[:int(idx) + 1].to(dev).double()
            return {"w2c": torch.inverse(c2w).float()}
        c2w = torch.stack([torch.as_tensor(kf["est_c2w"]).to(dev) for kf in keyframe_dict])
        w2c = torch.inverse(c2w).float()                                     # meshing.py:206
        dep = depths if depths is not None else torch.stack([torch.as_tensor(kf["gt_depth"]) for kf in keyframe_dict])
        dep = torch.as_tensor(dep).to(dev).float()
        if depth_test:
            return {"w2c": w2c, "depths": dep, "chunk": self.points_batch_size}
        return {"w2c": w2c, "max_depth": dep.reshape(dep.shape[0], -1).max(1).values}

    def _classes(self, points, mask_args):
        """``ops.point_masks`` of ``points`` in the mode of ``_mask_args``: [P] uint8, 0 unseen, 1 seen, 2 forecast."""
        return ops.point_masks(points, mask_args["w2c"], self.cam, self.mapper.H, self.mapper.W,
                               **{k: v for k, v in mask_args.items() if k != "w2c"})

    @torch.no_grad()
    def point_masks(self, points, keyframe_dict, estimate_c2w_list=None, idx=None, get_mask_use_all_frames=False, depth_test=False,
                    depths=None):
        """The reference's ``point_masks`` (meshing.py:124-291) -> (seen, forecast, unseen), bool [P] on the device; a point is
        forecast only when no keyframe sees it.  ``get_mask_use_all_frames``: the frustum tests alone over the poses
        ``estimate_c2w_list[:idx + 1]`` (each inverted in float64, then fp32), no depth rule.  Otherwise the keyframes'
        ``torch.inverse(est_c2w)``, with the depth limit 1.2 max(gt_depth) or, with ``depth_test``, the occlusion test against the
        keyframes' depth images in chunks of ``points_batch_size`` -- the forecast limit is each chunk's maximum depth sample, as
        in the reference, so the forecast mask depends on points_batch_size.  ``depths`` [K,H,W] replaces the keyframes' gt_depth
        in the depth test (and in the depth limit): it is the caller's hook for the reference's ``use_est_depth``, whose
        ``depth_render`` cannot run in the reference itself and is not rebuilt here."""
        if get_mask_use_all_frames and (estimate_c2w_list is None or idx is None):
            raise ValueError("Mesher.point_masks: get_mask_use_all_frames needs estimate_c2w_list and idx")
        points = torch.as_tensor(points).to(self.device).float()
        cls = self._classes(points, self._mask_args(keyframe_dict, (estimate_c2w_list, idx) if get_mask_use_all_frames else None,
                                                    depth_test, depths))
        return cls == ops.MASK_SEEN, cls == ops.MASK_FORECAST, cls == ops.MASK_UNSEEN

    @torch.no_grad()
    def keyframe_stem(self, keyframe_dict, encoder=None, batch=4):
        """The stem maps of the keyframes' ``gt_color`` (``encoder`` or ``mapper.encoder``, ``batch`` keyframes per call) as
        the channels-last fp32 stack [K, h, w, 64] that ``ops.keyframe_codes`` reads.  The stack stays on the device for the
        whole extraction: K * 64 * h * w * 4 bytes, 52 MB per keyframe at Replica resolution (h x w = 340 x 600).
        An ``encoder.ResNet(backend="hip")`` writes each batch straight into its slice of the stack.  The encoder's ``bn=`` decides
        the codes: "frozen" normalises with the running statistics; "batch" -- what the reference computes, and what a map it
        trained expects -- with the statistics of each call's own images, so there the maps depend on ``batch``."""
        enc = encoder if encoder is not None else getattr(self.mapper, "encoder", None)
        if enc is None:
            raise ValueError("Mesher.keyframe_stem: no encoder (mapper.encoder is None and encoder= was not given)")
        out = None
        for s in range(0, len(keyframe_dict), batch):
            img = torch.stack([torch.as_tensor(kf["gt_color"]).to(self.device).float() for kf in keyframe_dict[s:s + batch]])
            if getattr(enc, "backend", "torch") == "hip":
                if out is None:
                    out = torch.empty(len(keyframe_dict), *ops.stem_out_shape(img.shape[1], img.shape[2]), 64, device=self.device)
                enc.forward_channels_last(img, out=out[s:s + img.shape[0]])
                continue
            f = enc(img[None])[0].float()                                    # [n, C, h, w]
            if out is None:
                out = torch.empty(len(keyframe_dict), f.shape[2], f.shape[3], f.shape[1], device=self.device)
            out[s:s + f.shape[0]] = f.permute(0, 2, 3, 1)
        return out if out is not None else torch.zeros(0, 1, 1, 64, device=self.device)

    @torch.no_grad()
    def get_bound_from_frames(self, keyframe_dict, scale=None, *, voxel_length=None, sdf_trunc=None, stride=4, hull_eps=0.0):
        """The reference's scene bound (meshing.py:380-445) -> ``Bound(verts, faces, planes)`` on the device, in the scaled units
        ``extract`` works in.  The keyframes' gt_depth images are fused into a TSDF under ``open3d_poses`` (``ops.tsdf_fuse``:
        voxel_length 4 scale / 512, sdf_trunc 0.04 scale, every ``stride``-th pixel deciding which 16^3 units a frame touches --
        the reference's parameters and Open3D's; ``scale`` defaults to ``self.scale``); the points are the camera centres followed
        by the vertices of its zero crossing (``ops.tsdf_vertices``); their convex hull (``ops.convex_hull``) is scaled by
        ``clean_mesh_bound_scale`` about the mean c of its vertices, which turns a face (n, d) into (n, s d + (s - 1) n . c).

        ``hull_eps`` is the hull's tolerance and 0 by default.  A tolerance (voxel_length / 128, say) would under-approximate the
        points by at most that much, harmless beside a bound grown by 2 % of a metre-sized room -- but it also drops the hull
        vertices that protrude by less, and the reference scales about the MEAN OF THE HULL'S VERTICES, which then moves: on the
        synthetic test scene 150 vertices instead of 219 shift c by 0.69 m and the planes by up to 1.4 cm, for 146 rounds
        instead of 215.  The exact hull is what the reference builds, so it is the default.  The keyframes are not modified."""
        sc = self.scale if scale is None else float(scale)
        vl = 4.0 * sc / 512.0 if voxel_length is None else float(voxel_length)
        tr = 0.04 * sc if sdf_trunc is None else float(sdf_trunc)
        dev = self.device
        ext, pose, centres = open3d_poses(keyframe_dict)
        if len(keyframe_dict) == 0:
            raise ValueError("Mesher.get_bound_from_frames: keyframe_dict is empty")
        depths = torch.stack([torch.as_tensor(kf["gt_depth"]).to(dev).float() for kf in keyframe_dict]).contiguous()
        units, tsdf, weight = ops.tsdf_fuse(depths, torch.from_numpy(ext).to(dev), torch.from_numpy(pose).to(dev), self.cam, vl, tr, stride)
        verts = ops.tsdf_vertices(units, tsdf, weight, vl)
        points = torch.cat((torch.from_numpy(centres).to(dev), verts))
        vi, faces, planes, _ = ops.convex_hull(points, eps=float(hull_eps))
        hv = points[vi]
        c = hv.mean(0)
        s = self.clean_mesh_bound_scale
        n = planes[:, :3]
        nc = (n[:, 0] * c[0] + n[:, 1] * c[1]) + n[:, 2] * c[2]
        scaled = torch.cat((n, (s * planes[:, 3] + (s - 1.0) * nc)[:, None]), 1)
        new_id = torch.full((points.shape[0],), -1, dtype=torch.int64, device=dev)
        new_id[vi] = torch.arange(vi.numel(), device=dev)
        return Bound(c + s * (hv - c), new_id[faces], scaled)

    def _bound_planes(self, bound_planes, keyframe_dict, build=True):
        """``bound_planes`` of extract / get_mesh / grid_occupancy as planes [M,4]: an array, a ``Bound``, or "frames" = the
        reference's own bound, ``get_bound_from_frames(keyframe_dict).planes`` (built only with ``build``)."""
        if isinstance(bound_planes, str):
            if bound_planes != "frames":
                raise ValueError(f"Mesher: bound_planes must be an [M,4] array of half-spaces, a Bound or \"frames\", got {bound_planes!r}")
            return self.get_bound_from_frames(keyframe_dict).planes if build else bound_planes
        if isinstance(bound_planes, Bound):
            return bound_planes.planes
        return bound_planes

    @torch.no_grad()
    def grid_occupancy(self, keyframe_dict, stage="fine", kf=None, stem=None, forecast=False, depth_test=False, all_frames=None,
                       bound_planes=None):
        """[nx, ny, nz] occupancy volume of the query grid (meshing.py:643-654: keyframe labels -> eval_points per
        points_batch_size chunk -> values[:, 3]) and the grid's axes.  ``stem`` only lifts the refusal of a mapper with an
        encoder and is not used: the reference computes get_2d_feature's codes for every grid chunk, but they reach only the
        colour and logit networks, and this pass keeps the occupancy alone, which the coarse / fine network forms from the
        point encoding.

        ``forecast`` (the reference's show_forecast, meshing.py:601-641): the grid's point masks (``depth_test`` / ``all_frames``
        as in ``point_masks``, taken per points_batch_size chunk of the grid); the seen points, compacted, get their keyframe
        labels and the fine decoders of ``stage`` -- the > 1 point rule per points_batch_size chunk of the COMPACTED points, as
        the reference's loop over ``points[seen_mask]`` has it --, the compacted forecast points the coarse network, the unseen
        points -100.  ``bound_planes`` is accepted in ``extract``'s spellings ("frames" included) and checked, nothing more: the
        reference's grid pass does not read the bound, only the cleaning of the forecast mesh does."""
        self._check_supported(stem)
        self._bound_planes(bound_planes, keyframe_dict, build=False)
        kf = kf or self._keyframes(keyframe_dict)
        grid = self.get_grid_uniform()
        nx, ny, nz = (len(a) for a in grid["xyz"])
        P = nx * ny * nz
        B = self.points_batch_size
        step = B * max(1, (1 << 22) // B)                     # device chunks on points_batch_size boundaries
        if forecast:
            margs = self._mask_args(keyframe_dict, all_frames, depth_test)
            cls = torch.cat([self._classes(self.grid_points(grid["xyz"], s0, min(s0 + step, P)), margs) for s0 in range(0, P, step)])
            occ = torch.full((P,), -100.0, device=self.device)
            for which, stg in ((ops.MASK_SEEN, stage), (ops.MASK_FORECAST, "coarse")):
                idx = torch.nonzero(cls == which).reshape(-1)
                for s0 in range(0, idx.numel(), step):
                    n = idx[s0:s0 + step]
                    pts = self.grid_points(grid["xyz"], n)
                    label = None
                    if stg != "coarse":
                        label, _ = ops.keyframe_project(pts, kf[0], kf[1], kf[2], self.cam)
                    occ[n] = self.mapper.eval_occupancy(pts, label, stage=stg, rule_chunk=B)
            return occ.reshape(ny, nx, nz).permute(1, 0, 2).contiguous(), grid
        occ = torch.empty(P, device=self.device)
        for s0 in range(0, P, step):
            s1 = min(s0 + step, P)
            pts = self.grid_points(grid["xyz"], s0, s1)
            label = None
            if stage != "coarse":
                label, _ = ops.keyframe_project(pts, kf[0], kf[1], kf[2], self.cam)
            occ[s0:s1] = self.mapper.eval_occupancy(pts, label, stage=stage, rule_chunk=B)
        return occ.reshape(ny, nx, nz).permute(1, 0, 2).contiguous(), grid

    @torch.no_grad()
    def extract(self, keyframe_dict, stage="fine", clean_mesh=True, components=None, min_area=None, stem=None, *, forecast=False,
                depth_test=False, all_frames=None, bound_planes=None, holes=None):
        """-> (verts [V,3] fp32 world / scale, faces [F,3] int32, colors [V,3] uint8, labels [V] int64), all on the device.
        ``components``: None, "small" (keep the components whose area exceeds ``min_area``, default
        ``cfg['meshing']['remove_small_geometry_threshold'] * scale * scale``) or "largest" (meshing.py:721-733); the filter
        runs on the cleaned mesh, ahead of the vertex query, and only with ``clean_mesh``.  ``stem``: None (a mapper without
        stem features), True (run ``keyframe_stem``) or the [K,h,w,C] maps: the vertex query then uses the keyframe codes.

        ``depth_test``: the cleaning keeps the faces with a vertex that passes ``point_masks``' depth test (the reference's
        ``meshing.depth_test``).  ``all_frames = (estimate_c2w_list, idx)``: the masks -- of the cleaning and of ``forecast`` --
        are those of get_mask_use_all_frames.  ``forecast`` (the reference's show_forecast): the volume of
        ``grid_occupancy(forecast=True)``; the cleaning (meshing.py:695-708) drops the faces whose three vertices all lie outside
        a convex bound, ``bound_planes`` [M,4]: a point x is inside when n . x + d <= 0 for every row (n, d) -- exactly
        ``scipy.spatial.ConvexHull(...).equations``, in the scaled units of the marching-cubes bound.  ``bound_planes="frames"`` is the
        reference's own bound, ``get_bound_from_frames(keyframe_dict).planes`` (a TSDF fusion of the keyframes and its scaled hull);
        it is never built unasked, so ``forecast`` with ``clean_mesh`` and no ``bound_planes`` is refused.  The vertices whose mask
        is forecast are coloured (0, 255, 255) (:756-762).

        ``holes``: None (no filling), True (= 4, the reference's ``mesh.fill_holes()``, meshing.py:770) or the largest boundary loop to
        close, an int in 3 .. 32: the faces returned are ``fill_holes``' -- the cleaned and filtered faces first, the new ones after
        them.  No vertex is added, so colours and labels are the same."""
        self._check_supported(stem)
        holes = _holes_arg("Mesher.extract", holes)
        if forecast and clean_mesh and bound_planes is None:
            raise NotImplementedError("Mesher.extract: forecast=True with clean_mesh=True needs a bound: bound_planes=\"frames\" builds the "
                                      "reference's (Mesher.get_bound_from_frames), or pass the half-spaces [M,4] of a convex bound")
        self._bound_planes(bound_planes, keyframe_dict, build=False)
        if components not in (None, "small", "largest"):
            raise ValueError(f"Mesher.extract: components must be None, 'small' or 'largest', got {components!r}")
        if components is not None and not clean_mesh:
            raise ValueError("Mesher.extract: components needs clean_mesh=True (the reference filters only the cleaned mesh)")
        if components == "small" and min_area is None:
            if self.remove_small_geometry_threshold is None:
                raise ValueError("Mesher.extract: components='small' needs cfg['meshing']['remove_small_geometry_threshold'] "
                                 "(or min_area=)")
            min_area = self.remove_small_geometry_threshold * self.scale * self.scale
        bound_planes = self._bound_planes(bound_planes, keyframe_dict, build=forecast and clean_mesh)
        kf = self._keyframes(keyframe_dict, stem)
        vol, grid = self.grid_occupancy(keyframe_dict, stage, kf, stem, forecast, depth_test, all_frames)
        x, y, z = grid["xyz"]
        verts, faces = ops.marching_cubes(vol, self.level_set, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
        if clean_mesh and faces.shape[0]:
            if forecast:
                verts, faces = compact_mesh(verts, faces, inside_planes(verts, bound_planes)[faces.long()].any(1))[:2]
            else:
                verts, faces = self.clean(verts, faces, kf, depth_test,
                                          self._mask_args(keyframe_dict, all_frames, depth_test) if depth_test or all_frames else None)
        if components == "small":
            verts, faces = self.filter_components(verts, faces, min_area=min_area)
        elif components == "largest":
            verts, faces = self.filter_components(verts, faces, largest=True)
        colors, labels = self.vertex_query(verts, kf, stage, stem)
        if forecast and verts.shape[0]:
            fore = self._classes(verts, self._mask_args(keyframe_dict, all_frames, depth_test)) == ops.MASK_FORECAST
            colors[fore] = torch.tensor([0, 255, 255], dtype=torch.uint8, device=colors.device)
        if holes is not None:
            faces = self.fill_holes(verts, faces, holes)[0]
        return verts / self.scale, faces, colors, labels

    def clean(self, verts, faces, kf, depth_test=False, mask_args=None):
        """meshing.py:714-719: drop the faces whose three vertices no keyframe sees, then the vertices no face uses.  With
        ``mask_args`` (``_mask_args``: the depth test -- ``depth_test`` must then be set with it -- or the all-frames branch) seen
        is ``point_masks``' in that mode."""
        if depth_test and (mask_args is None or "depths" not in mask_args):
            raise ValueError("Mesher.clean: depth_test needs mask_args=_mask_args(keyframe_dict, depth_test=True)")
        if mask_args is not None:
            seen = self._classes(verts, mask_args) == ops.MASK_SEEN
        else:
            _, seen = ops.keyframe_project(verts, kf[0], kf[1], kf[2], self.cam)
        return compact_mesh(verts, faces, seen[faces.long()].any(1))[:2]

    def filter_components(self, verts, faces, min_area=None, largest=False):
        """meshing.py:721-733 on the device (ops.mesh_components): keep the faces of the connected components whose area is
        ``> min_area`` (strict, as in the reference), or with ``largest`` those of the component of maximum area (ties: the
        component with the smallest face).  ``verts`` are in the scaled units ``extract`` works in, before the division by
        ``scale``.  Faces and vertices keep their original order -- trimesh's split + concatenate lists them component by
        component instead; the set of faces is the same -- and an empty result is the empty mesh [0,3], [0,3] (the reference
        crashes there)."""
        if (min_area is None) == (not largest):
            raise ValueError("Mesher.filter_components: pass min_area or largest=True (one of them)")
        if faces.shape[0] == 0:
            return verts[:0], faces[:0]
        comp, comp_area, _ = ops.mesh_components(verts, faces)
        if largest:
            best = comp_area.max()
            keep = comp == comp[comp_area == best].min()
        else:
            keep = comp_area > float(min_area)
        return compact_mesh(verts, faces, keep)[:2]

    def fill_holes(self, verts, faces, max_edges=4):
        """meshing.py:770 on the device (ops.mesh_fill_holes): -> (faces_out [F + A, 3] int32, info).  The boundary loops of 3 ..
        ``max_edges`` edges whose vertices all have one boundary edge in and one out get a fan from their smallest vertex, wound
        against the faces across the boundary; ``faces`` come first, unchanged, and no vertex is added (include/dns_hip.h)."""
        return ops.mesh_fill_holes(faces, int(verts.shape[0]), max_edges)

    def vertex_query(self, verts, kf, stage="fine", stem=None):
        """meshing.py:735-753: colours (clip(rgb, 0, 1) * 255 as uint8) and labels (argmax, -1 outside the bound) at the
        vertices, the > 1 point rule per points_batch_size chunk of vertices.  With ``stem`` (``kf`` from
        ``_keyframes(keyframe_dict, stem)``) the colour and logit networks read get_2d_feature's keyframe codes as pixel_pts."""
        if verts.shape[0] == 0:
            return (torch.zeros(0, 3, dtype=torch.uint8, device=verts.device), torch.zeros(0, dtype=torch.int64, device=verts.device))
        label, _ = ops.keyframe_project(verts, kf[0], kf[1], kf[2], self.cam)
        codes = None
        if stem is not None:
            if len(kf) < 6:
                raise ValueError("Mesher.vertex_query: stem needs the keyframe bundle of _keyframes(keyframe_dict, stem)")
            codes, _ = ops.keyframe_codes(verts, kf[0], kf[4], kf[3], self._stem_maps(kf[5]), self.cam, self.mapper.decoder.merge)
        values, labels = self.mapper.eval_points(verts, codes, label, stage=stage, rule_chunk=self.points_batch_size)
        colors = (values[:, :3].clamp(0, 1) * 255).to(torch.uint8)
        if labels is None:
            labels = torch.full((verts.shape[0],), -1, dtype=torch.int64, device=verts.device)
        return colors, labels

    def get_mesh(self, mesh_out_file, keyframe_dict, idx, color=True, label=False, palette=None, show_forecast=False,
                 element=False, clean_mesh=None, stage="fine", remove_small_geometry=False, fill_holes=False, components=None,
                 min_area=None, stem=None, *, forecast=False, depth_test=False, all_frames=None, bound_planes=None, holes=None):
        """Writes ``{mesh_out_file}/mesh_{idx}.ply`` (vertex colours when ``color``, the vertex labels as an int property) and,
        with ``label`` and a ``palette`` (class -> RGB: an [n_class, 3] array, a dict or a callable like the reference's
        v_map_function), ``mesh_{idx}_semantic.ply``.  Returns the paths written.  ``components`` / ``min_area``: the
        connected-components filter of ``extract`` (meshing.py:721-733); ``stem``, ``forecast`` (the reference's show_forecast),
        ``depth_test``, ``all_frames`` and ``bound_planes`` ("frames" included): as in ``extract``.
        ``holes``: None, True (= 4, the reference's ``mesh.fill_holes()``, meshing.py:770) or an int in 3 .. 32: ``mesh_{idx}.ply``
        gets ``fill_holes``' face list; as in the reference (:781) the semantic mesh keeps the unfilled faces.  The reference's own
        spellings -- of the filters, of the forecast mesh, of the per-class meshes and ``fill_holes`` -- are refused when asked for,
        each naming ours."""
        if show_forecast:
            raise NotImplementedError("Mesher.get_mesh: show_forecast is not a keyword here; pass forecast=True (with "
                                      "bound_planes=\"frames\" when the mesh is cleaned)")
        if element:
            raise NotImplementedError("Mesher.get_mesh: element is not a keyword here; the per-class meshes are written by "
                                      "Mesher.get_part_meshes")
        if remove_small_geometry:
            raise NotImplementedError("Mesher.get_mesh: remove_small_geometry is not a keyword here; pass components=\"small\" "
                                      "(or components=\"largest\")")
        if fill_holes:
            raise NotImplementedError("Mesher.get_mesh: fill_holes is not a keyword here; pass holes=True (or the largest loop to "
                                      "close, holes=3 .. 32)")
        holes = _holes_arg("Mesher.get_mesh", holes)
        verts, faces, colors, labels = self.extract(keyframe_dict, stage, self.clean_mesh if clean_mesh is None else clean_mesh,
                                                    components, min_area, stem, forecast=forecast, depth_test=depth_test,
                                                    all_frames=all_frames, bound_planes=bound_planes)
        v, f, lab = verts.cpu().numpy(), faces.cpu().numpy(), labels.cpu().numpy()
        filled = f if holes is None else self.fill_holes(verts, faces, holes)[0].cpu().numpy()
        os.makedirs(mesh_out_file, exist_ok=True)
        out = [os.path.join(mesh_out_file, f"mesh_{idx}.ply")]
        write_ply(out[0], v, filled, colors.cpu().numpy() if color else None, lab)
        if label and palette is not None:
            out.append(os.path.join(mesh_out_file, f"mesh_{idx}_semantic.ply"))
            write_ply(out[1], v, f, label_colors(lab, palette), lab)
        return out

    def get_part_meshes(self, mesh_out_file, keyframe_dict, idx, color=True, stage="fine", clean_mesh=None, components=None,
                        min_area=None, stem=None, depth_test=False):
        """The reference's ``element`` branch (meshing.py:786-825): for every distinct vertex label e of the extracted mesh,
        the faces with at least one vertex labelled e, compacted, as ``{mesh_out_file}/mesh_{idx}_part_{int(e)}.ply``.  Colours
        and labels are those of the full mesh's vertex query, not queried again per part.  ``stem``, ``depth_test``: as in
        ``extract``.  Returns the paths written."""
        verts, faces, colors, labels = self.extract(keyframe_dict, stage, self.clean_mesh if clean_mesh is None else clean_mesh,
                                                    components, min_area, stem, depth_test=depth_test)
        os.makedirs(mesh_out_file, exist_ok=True)
        out = []
        for e in torch.unique(labels).tolist():
            v, f, used = compact_mesh(verts, faces, (labels == e)[faces.long()].any(1))
            out.append(os.path.join(mesh_out_file, f"mesh_{idx}_part_{int(e)}.ply"))
            write_ply(out[-1], v.cpu().numpy(), f.cpu().numpy(), colors[used].cpu().numpy() if color else None,
                      labels[used].cpu().numpy())
        return out


def _holes_arg(who, holes):
    """``holes`` of extract / get_mesh -> None or max_edges: True is 4 (trimesh.repair.fill_holes), an int is itself."""
    if holes is None:
        return None
    if holes is True:
        return ops.HOLES_MAX_EDGES
    if isinstance(holes, bool) or not isinstance(holes, (int, np.integer)) or not 3 <= int(holes) <= 32:
        raise ValueError(f"{who}: holes must be None, True or an int in 3 .. 32, got {holes!r}")
    return int(holes)


def inside_planes(points, planes):
    """bool [P]: the points [P,3] inside the convex region of the half-spaces ``planes`` [M,4], n . x + d <= 0 for every row
    (n, d) (``scipy.spatial.ConvexHull.equations``); float64, ((n0 x + n1 y) + n2 z) + d in that order."""
    pl = torch.as_tensor(planes).to(points.device).double().reshape(-1, 4)
    p = points.double()
    val = ((p[:, None, 0] * pl[None, :, 0] + p[:, None, 1] * pl[None, :, 1]) + p[:, None, 2] * pl[None, :, 2]) + pl[None, :, 3]
    return (val <= 0).all(1)


def compact_mesh(verts, faces, keep):
    """The faces with ``keep`` [F] bool set and the vertices they use, both in their original order and the faces re-indexed,
    plus the bool [V] mask of those vertices."""
    faces = faces[keep]
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[faces.reshape(-1).long()] = True
    new_id = torch.cumsum(used, 0, dtype=torch.int64) - 1
    return verts[used], new_id[faces.long()].to(torch.int32), used


def label_colors(labels, palette):
    """uint8 [V,3] colours of the labels through a class -> RGB palette (array, dict or callable); unknown classes black."""
    labels = np.asarray(labels)
    if callable(palette):
        rgb = np.stack([np.asarray(c) for c in palette(labels)], -1) if labels.size else np.zeros((0, 3))
        return np.asarray(rgb).reshape(-1, 3).astype(np.uint8)
    if isinstance(palette, dict):
        n = max(int(k) for k in palette) + 1 if palette else 0
        table = np.zeros((n, 3), np.uint8)
        for k, c in palette.items():
            table[int(k)] = c
    else:
        table = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    out = np.zeros((labels.shape[0], 3), np.uint8)
    ok = (labels >= 0) & (labels < table.shape[0])
    out[ok] = table[labels[ok]]
    return out


def write_ply(path, verts, faces, colors=None, labels=None):
    """Binary little-endian PLY 1.0: vertex ``float x, y, z`` (+ ``uchar red, green, blue``) (+ ``int label``), face
    ``list uchar int vertex_indices``."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = verts.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    if labels is not None:
        fields += [("label", "<i4")]
        props += ["property int label"]
    vd = np.empty(V, dtype=fields)
    vd["x"], vd["y"], vd["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    if colors is not None:
        c = np.asarray(colors, np.uint8).reshape(-1, 3)
        vd["red"], vd["green"], vd["blue"] = c[:, 0], c[:, 1], c[:, 2]
    if labels is not None:
        vd["label"] = np.asarray(labels).astype(np.int32)
    fd = np.empty(faces.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    fd["n"], fd["i"] = 3, faces
    header = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {V}", *props,
                        f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]) + "\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vd.tobytes())
        f.write(fd.tobytes())
