"""Semantic mesh extraction: reference ``Mesher`` (slams/meshing.py:17-784) on this package's mapper.

The grid query, the keyframe projection, marching cubes and the connected-components filter run on the GPU (csrc/mesh.hip,
csrc/mesh_cc.hip, ``Mapper.eval_occupancy``); the reference's host-side numpy / skimage / trimesh steps have no counterpart
here beyond the binary PLY writer below.

A mapper trained with stem features (``mapper.encoder`` set) is meshed with ``stem=``: the vertex query then feeds the colour and
logit networks get_2d_feature's keyframe codes (meshing.py:311-377; csrc/mesh_feature.hip, ``ops.keyframe_codes``).  The
geometry needs no codes -- the occupancy is the coarse / fine network's, which reads only the point encoding -- so the grid
pass, marching cubes, cleaning and the component filter are the same with and without ``stem``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops


class Mesher:
    """``Mesher(cfg, slam)`` of the reference for one ``mapping.Mapper``.  Reads ``cfg['meshing']`` (resolution, level_set,
    points_batch_size, clean_mesh, remove_small_geometry_threshold), ``cfg['scale']`` (default 1) and
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
        self.scale = float(cfg.get("scale", 1))
        thr = m.get("remove_small_geometry_threshold")
        self.remove_small_geometry_threshold = None if thr is None else float(thr)
        if m.get("depth_test", False):
            raise NotImplementedError("Mesher: depth_test=True (point_masks' rendered-depth test) is not supported")
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

    def grid_points(self, xyz, s0, s1):
        """Points s0..s1 of the reference's flattened meshgrid (indexing 'xy': point (j nx + i) nz + k = (x_i, y_j, z_k)),
        fp32 as ``torch.tensor(..., dtype=torch.float)`` rounds them."""
        x, y, z = (torch.tensor(a, dtype=torch.float64, device=self.device).float() for a in xyz)
        nx, nz = x.numel(), z.numel()
        n = torch.arange(s0, s1, device=self.device)
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

    @torch.no_grad()
    def keyframe_stem(self, keyframe_dict, encoder=None, batch=4):
        """The stem maps of the keyframes' ``gt_color`` (``encoder`` or ``mapper.encoder``, ``batch`` keyframes per call) as
        the channels-last fp32 stack [K, h, w, 64] that ``ops.keyframe_codes`` reads.  The stack stays on the device for the
        whole extraction: K * 64 * h * w * 4 bytes, 52 MB per keyframe at Replica resolution (h x w = 340 x 600)."""
        enc = encoder if encoder is not None else getattr(self.mapper, "encoder", None)
        if enc is None:
            raise ValueError("Mesher.keyframe_stem: no encoder (mapper.encoder is None and encoder= was not given)")
        out = None
        for s in range(0, len(keyframe_dict), batch):
            img = torch.stack([torch.as_tensor(kf["gt_color"]).to(self.device).float() for kf in keyframe_dict[s:s + batch]])
            f = enc(img[None])[0].float()                                    # [n, C, h, w]
            if out is None:
                out = torch.empty(len(keyframe_dict), f.shape[2], f.shape[3], f.shape[1], device=self.device)
            out[s:s + f.shape[0]] = f.permute(0, 2, 3, 1)
        return out if out is not None else torch.zeros(0, 1, 1, 64, device=self.device)

    @torch.no_grad()
    def grid_occupancy(self, keyframe_dict, stage="fine", kf=None, stem=None):
        """[nx, ny, nz] occupancy volume of the query grid (meshing.py:643-654: keyframe labels -> eval_points per
        points_batch_size chunk -> values[:, 3]) and the grid's axes.  ``stem`` only lifts the refusal of a mapper with an
        encoder and is not used: the reference computes get_2d_feature's codes for every grid chunk, but they reach only the
        colour and logit networks, and this pass keeps the occupancy alone, which the coarse / fine network forms from the
        point encoding."""
        self._check_supported(stem)
        kf = kf or self._keyframes(keyframe_dict)
        grid = self.get_grid_uniform()
        nx, ny, nz = (len(a) for a in grid["xyz"])
        P = nx * ny * nz
        B = self.points_batch_size
        step = B * max(1, (1 << 22) // B)                     # device chunks on points_batch_size boundaries
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
    def extract(self, keyframe_dict, stage="fine", clean_mesh=True, components=None, min_area=None, stem=None):
        """-> (verts [V,3] fp32 world / scale, faces [F,3] int32, colors [V,3] uint8, labels [V] int64), all on the device.
        ``components``: None, "small" (keep the components whose area exceeds ``min_area``, default
        ``cfg['meshing']['remove_small_geometry_threshold'] * scale * scale``) or "largest" (meshing.py:721-733); the filter
        runs on the cleaned mesh, ahead of the vertex query, and only with ``clean_mesh``.  ``stem``: None (a mapper without
        stem features), True (run ``keyframe_stem``) or the [K,h,w,C] maps: the vertex query then uses the keyframe codes."""
        self._check_supported(stem)
        if components not in (None, "small", "largest"):
            raise ValueError(f"Mesher.extract: components must be None, 'small' or 'largest', got {components!r}")
        if components is not None and not clean_mesh:
            raise ValueError("Mesher.extract: components needs clean_mesh=True (the reference filters only the cleaned mesh)")
        if components == "small" and min_area is None:
            if self.remove_small_geometry_threshold is None:
                raise ValueError("Mesher.extract: components='small' needs cfg['meshing']['remove_small_geometry_threshold'] "
                                 "(or min_area=)")
            min_area = self.remove_small_geometry_threshold * self.scale * self.scale
        kf = self._keyframes(keyframe_dict, stem)
        vol, grid = self.grid_occupancy(keyframe_dict, stage, kf, stem)
        x, y, z = grid["xyz"]
        verts, faces = ops.marching_cubes(vol, self.level_set, (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1]))
        if clean_mesh and faces.shape[0]:
            verts, faces = self.clean(verts, faces, kf)
        if components == "small":
            verts, faces = self.filter_components(verts, faces, min_area=min_area)
        elif components == "largest":
            verts, faces = self.filter_components(verts, faces, largest=True)
        colors, labels = self.vertex_query(verts, kf, stage, stem)
        return verts / self.scale, faces, colors, labels

    def clean(self, verts, faces, kf):
        """meshing.py:714-719: drop the faces whose three vertices no keyframe sees, then the vertices no face uses."""
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
                 min_area=None, stem=None):
        """Writes ``{mesh_out_file}/mesh_{idx}.ply`` (vertex colours when ``color``, the vertex labels as an int property) and,
        with ``label`` and a ``palette`` (class -> RGB: an [n_class, 3] array, a dict or a callable like the reference's
        v_map_function), ``mesh_{idx}_semantic.ply``.  Returns the paths written.  ``components`` / ``min_area``: the
        connected-components filter of ``extract`` (meshing.py:721-733); ``stem``: as in ``extract``.  fill_holes (meshing.py:770) is not implemented and,
        like the reference's own spellings of the filters and of the per-class meshes, refused when asked for."""
        if show_forecast:
            raise NotImplementedError("Mesher.get_mesh: show_forecast is not supported")
        if element:
            raise NotImplementedError("Mesher.get_mesh: element is not a keyword here; the per-class meshes are written by "
                                      "Mesher.get_part_meshes")
        if remove_small_geometry:
            raise NotImplementedError("Mesher.get_mesh: remove_small_geometry is not a keyword here; pass components=\"small\" "
                                      "(or components=\"largest\")")
        if fill_holes:
            raise NotImplementedError("Mesher.get_mesh: fill_holes is not supported")
        verts, faces, colors, labels = self.extract(keyframe_dict, stage, self.clean_mesh if clean_mesh is None else clean_mesh,
                                                    components, min_area, stem)
        v, f, lab = verts.cpu().numpy(), faces.cpu().numpy(), labels.cpu().numpy()
        os.makedirs(mesh_out_file, exist_ok=True)
        out = [os.path.join(mesh_out_file, f"mesh_{idx}.ply")]
        write_ply(out[0], v, f, colors.cpu().numpy() if color else None, lab)
        if label and palette is not None:
            out.append(os.path.join(mesh_out_file, f"mesh_{idx}_semantic.ply"))
            write_ply(out[1], v, f, label_colors(lab, palette), lab)
        return out

    def get_part_meshes(self, mesh_out_file, keyframe_dict, idx, color=True, stage="fine", clean_mesh=None, components=None,
                        min_area=None, stem=None):
        """The reference's ``element`` branch (meshing.py:786-825): for every distinct vertex label e of the extracted mesh,
        the faces with at least one vertex labelled e, compacted, as ``{mesh_out_file}/mesh_{idx}_part_{int(e)}.ply``.  Colours
        and labels are those of the full mesh's vertex query, not queried again per part.  ``stem``: as in ``extract``.  Returns
        the paths written."""
        verts, faces, colors, labels = self.extract(keyframe_dict, stage, self.clean_mesh if clean_mesh is None else clean_mesh,
                                                    components, min_area, stem)
        os.makedirs(mesh_out_file, exist_ok=True)
        out = []
        for e in torch.unique(labels).tolist():
            v, f, used = compact_mesh(verts, faces, (labels == e)[faces.long()].any(1))
            out.append(os.path.join(mesh_out_file, f"mesh_{idx}_part_{int(e)}.ply"))
            write_ply(out[-1], v.cpu().numpy(), f.cpu().numpy(), colors[used].cpu().numpy() if color else None,
                      labels[used].cpu().numpy())
        return out


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
