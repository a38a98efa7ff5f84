"""Keyframe storage of a run (reference ``Mapper.run``: ``keyframe_dict`` / ``keyframe_list``, slams/mapping.py:975-979,1082-1089).

The reference keeps every keyframe as CPU tensors and ``set_target_refer_frames`` copies each target and reference image to the
device on every ``optimize`` call.  ``KeyframeBank`` preallocates the images and the pose tables once -- on the device by default --
and hands out the reference's list of dicts whose values are VIEWS into that storage: ``Mapper.set_target_refer_frames``, ``Mesher``
and ``visualize`` consume the list unchanged, their ``.to(device)`` calls return the views themselves, and that is the saving.
``storage="host"`` keeps the reference's CPU tensors (small-memory devices).

The pose table ``est_c2w [capacity,4,4]`` is what ``ops.keyframe_overlap`` reads: one launch and one [n] read per
``keyframe_selection_overlap`` call in place of one small host-to-device copy per keyframe, a batched inverse and a read.
``Mapper.optimize`` REBINDS ``kf["est_c2w"]`` after bundle adjustment (the reference's :914-926); the dicts handed out write such
an assignment through into the table and keep holding the view, so the table equals the dict entries after every ``optimize``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

_IMAGE_KEYS = ("gt_color", "gt_depth", "gt_label")
_POSE_KEYS = ("gt_c2w", "est_c2w")


class _Keyframe(dict):
    """One entry of ``KeyframeBank.as_list()``: the reference's keys, the values views of the bank's storage.  Assigning to one of
    the bank's keys copies INTO the view (so ``kf["est_c2w"] = refined.clone()`` updates the pose table); other keys are plain."""

    def __init__(self, views):
        super().__init__(views)
        self._views = dict(views)

    def __setitem__(self, key, value):
        view = self._views.get(key) if hasattr(self, "_views") else None
        if view is None:
            return super().__setitem__(key, value)
        with torch.no_grad():
            view.copy_(torch.as_tensor(value).detach().to(device=view.device, dtype=view.dtype))
        super().__setitem__(key, view)


class KeyframeBank:
    def __init__(self, capacity: int, H: int, W: int, n_class: int, device, storage: str = "device", label_dtype=torch.float32):
        if storage not in ("device", "host"):
            raise ValueError(f"KeyframeBank: storage {storage!r} ('device' or 'host')")
        if capacity < 1 or H < 1 or W < 1 or n_class < 1:
            raise ValueError(f"KeyframeBank: capacity {capacity}, image {H} x {W}, n_class {n_class}")
        self.capacity, self.H, self.W, self.n_class = int(capacity), int(H), int(W), int(n_class)
        self.device, self.storage = device, storage
        at = device if storage == "device" else "cpu"
        self.gt_color = torch.zeros(capacity, H, W, 3, dtype=torch.float32, device=at)
        self.gt_depth = torch.zeros(capacity, H, W, dtype=torch.float32, device=at)
        self.gt_label = torch.zeros(capacity, H, W, dtype=label_dtype, device=at)
        self.gt_c2w = torch.zeros(capacity, 4, 4, dtype=torch.float32, device=at)
        self.est_c2w = torch.zeros(capacity, 4, 4, dtype=torch.float32, device=at)
        self.present = torch.zeros(capacity, n_class, dtype=torch.bool, device=at)      # class c occurs in keyframe i
        self.frame_idx = []                                                              # the reference's keyframe_list
        self._list = []

    def __len__(self):
        return len(self._list)

    def add(self, idx: int, gt_color, gt_depth, gt_label, gt_c2w, est_c2w) -> dict:
        """Stores frame ``idx`` as the next keyframe (copies into the preallocated storage; no host read) and returns its dict."""
        i = len(self._list)
        if i >= self.capacity:
            raise RuntimeError(f"KeyframeBank: full ({self.capacity} keyframes); size it from slam.schedule()")
        views = {}
        with torch.no_grad():
            for key, src in zip(_IMAGE_KEYS + _POSE_KEYS, (gt_color, gt_depth, gt_label, gt_c2w, est_c2w)):
                view = getattr(self, key)[i]
                src = torch.as_tensor(src).detach()
                if tuple(src.shape) != tuple(view.shape):
                    raise ValueError(f"KeyframeBank.add: {key} {tuple(src.shape)}, the bank holds {tuple(view.shape)}")
                view.copy_(src.to(device=view.device, dtype=view.dtype))
                views[key] = view
            cls = views["gt_label"].reshape(-1).long().clamp_(0, self.n_class - 1)
            self.present[i].index_fill_(0, cls, True)
        kf = _Keyframe(views)
        self._list.append(kf)
        self.frame_idx.append(int(idx))
        return kf

    def as_list(self):
        """The reference's ``keyframe_dict``: a list (the SAME object on every call, grown by ``add``) of dicts with gt_color,
        gt_depth, gt_label, gt_c2w, est_c2w as views into the bank."""
        return self._list

    def poses(self, n=None):
        """est_c2w [n,4,4] of the first n keyframes, on the compute device (a view for device storage)."""
        n = len(self) if n is None else n
        return self.est_c2w[:n].to(self.device)

    def host_copy(self):
        """The list as independent CPU tensors, what a checkpoint stores (a pickled VIEW would carry the whole bank)."""
        return [{k: v.detach().cpu().clone() for k, v in kf.items()} for kf in self._list]

    def overlap_scorer(self, cam: dict, edge: int = 10, eps: float = 1e-5):
        """-> ``Mapper.overlap_scorer``: (pts [P,3], keyframe_dict) -> float64 [n], count / P with the counts of
        ``ops.keyframe_overlap`` on the bank's pose table (keyframe_dict must be a prefix of ``as_list()``, which is what
        ``set_target_refer_frames`` passes); one [n] int32 read, the one the sort that follows needs."""
        H, W, fx, fy, cx, cy = (cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy"))

        def score(pts, keyframe_dict):
            n = len(keyframe_dict)
            if n > len(self._list) or any(a is not b for a, b in zip(keyframe_dict, self._list)):
                raise ValueError("KeyframeBank.overlap_scorer: keyframe_dict is not a prefix of the bank's list")
            pts = pts.detach().float().contiguous()
            counts = ops.keyframe_overlap(pts, self.poses(n).contiguous(), H, W, fx, fy, cx, cy, edge=edge, eps=eps)
            return counts.cpu().numpy().astype(np.float64) / pts.shape[0]

        return score
