"""Replica and ScanNet frame sources (reference datas/slam_datasets.py) and the camera update of ``DNS_SLAM.update_cam``
(slams/dns_slam.py:110-132).

Decoding a file is host work behind a ``reader=`` hook (path -> ndarray); everything after it -- the float conversions, the two
resizes, the class look-up, ``crop_size`` and ``crop_edge`` -- is one launch on the raw 8/16-bit images (``ops.prepare_frames``,
csrc/frame_prep.hip), where the reference runs ``np.vectorize`` over a dict for every label pixel, resizes on the CPU and copies three
float images to the device.  ``cal_class_n`` numbers the classes exactly as the reference's ``set(label_data.flatten())`` walk does:
a set's iteration order depends only on the order in which its distinct keys arrive, so the values present are taken in first-seen
order (``ops.label_first_seen``), inserted as numpy scalars of the image's dtype, and the set is iterated.

Differences from the reference, on purpose:
  * ``__getitem__`` returns a scaled COPY of the pose.  The reference multiplies ``self.poses[index][:3, 3]`` by ``scale`` in place on
    every read, which is harmless only because every config's scale is 1.
  * ``cv2.undistort`` is not built: no config of the reference sets ``cam.distortion``; one that does raises NotImplementedError.
  * ``frames(indices)`` reads a batch through one launch.
"""
from __future__ import annotations

import csv
import glob
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import ops


def camera_from_cfg(cfg) -> dict:
    """``DNS_SLAM.update_cam``: cfg['cam'] H, W, fx, fy, cx, cy after ``crop_size`` (a resize) and ``crop_edge``, as the dict
    ``synthetic.camera`` returns."""
    cam = cfg["cam"]
    H, W, fx, fy, cx, cy = cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    if "crop_size" in cam:
        crop_size = cam["crop_size"]
        sx, sy = crop_size[1] / W, crop_size[0] / H
        fx, fy, cx, cy = sx * fx, sy * fy, sx * cx, sy * cy
        W, H = crop_size[1], crop_size[0]
    if cam["crop_edge"] > 0:
        H -= cam["crop_edge"] * 2
        W -= cam["crop_edge"] * 2
        cx -= cam["crop_edge"]
        cy -= cam["crop_edge"]
    return {"H": H, "W": W, "fx": fx, "fy": fy, "cx": cx, "cy": cy}


def pil_reader(path):
    """The default ``reader``: a file -> ndarray through Pillow, imported on first use.  Colour comes back uint8 [H,W,3] in RGB order,
    8-bit grey uint8 [H,W], 16-bit grey uint16 [H,W] (what cv2.imread(..., IMREAD_UNCHANGED) returns, but for the channel order)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("dns_slam_amd.datasets: decoding image files needs Pillow (PIL); install it or pass reader= (a function "
                          "path -> ndarray, with an attribute color_order = 'RGB' or 'BGR')") from e
    with Image.open(path) as im:
        if im.mode.startswith("I"):                              # I;16, I;16B, I: 16-bit grey (Pillow widens some to int32)
            a = np.asarray(im)
            if a.min() < 0 or a.max() > 65535:
                raise ValueError(f"{path}: grey values outside uint16")
            return np.ascontiguousarray(a.astype(np.uint16))
        if im.mode == "L":
            return np.array(im, dtype=np.uint8)                         # a copy: torch wants writable memory
        return np.array(im.convert("RGB"), dtype=np.uint8)


pil_reader.color_order = "RGB"


class FramePrep:
    """The device tables of ``ops.prepare_frames`` for one set of image sizes, built once: ``cfg['cam']`` gives ``png_depth_scale``,
    ``crop_size`` (optional) and ``crop_edge``; ``label_hw=None``: no labels.  ``__call__(color_u8, depth_u16, label, lut)`` ->
    (color fp32 [..,H,W,3], depth fp32 [..,H,W], label int64 [..,H,W] or None) for one frame or a batch."""

    def __init__(self, cfg, color_hw, depth_hw, label_hw, device, scale=1.0, method=None):
        cam = cfg["cam"]
        if "distortion" in cam:
            raise NotImplementedError("cfg['cam']['distortion'] is set: cv2.undistort is not built (no config of the reference sets it)")
        self.png_depth_scale = cam["png_depth_scale"]
        self.scale = scale
        self.method = method
        self.tables = ops.frame_prep_tables(color_hw, depth_hw, label_hw, cam.get("crop_size"), cam["crop_edge"], device)
        self.H, self.W = self.tables.H, self.tables.W

    def __call__(self, color_u8, depth_u16, label=None, lut=None, bgr=False):
        return ops.prepare_frames(color_u8, depth_u16, label, lut, self.tables, self.png_depth_scale, self.scale, bgr=bgr,
                                  method=self.method)


class BaseDataset(Dataset):
    """Reference ``BaseDataset``: ``__getitem__(i)`` -> (i, color [H,W,3] fp32, depth [H,W] fp32, label [H,W] int64, pose [4,4]) on
    ``device``.  ``reader``: path -> ndarray (default ``pil_reader``); its ``color_order`` attribute ('RGB', the default, or 'BGR' for
    cv2.imread) says how colour comes back.  ``method``: ``ops.prepare_frames``' (None: the kernel on a GPU, torch ops on the CPU)."""

    def __init__(self, cfg, input_folder, scale, device="cuda:0", reader=None, method=None):
        super().__init__()
        self.name = cfg["dataset"]
        self.cfg = cfg
        self.device = device
        self.scale = scale
        self.png_depth_scale = cfg["cam"]["png_depth_scale"]
        self.semantic = True
        if "distortion" in cfg["cam"]:
            raise NotImplementedError("cfg['cam']['distortion'] is set: cv2.undistort is not built (no config of the reference sets it)")
        self.distortion = None
        self.crop_size = cfg["cam"]["crop_size"] if "crop_size" in cfg["cam"] else None
        self.input_folder = input_folder
        self.crop_edge = cfg["cam"]["crop_edge"]
        self.reader = reader or pil_reader
        self.bgr = str(getattr(self.reader, "color_order", "RGB")).upper() == "BGR"
        self.method = method
        self._preps = {}
        self.lut = None

    def __len__(self):
        return self.n_img

    # the reference's file names (:86-93)
    def frame_paths(self, index):
        raise NotImplementedError

    def label_path(self, index):
        return self.frame_paths(index)[2]

    def read_label(self, index):
        lab = np.ascontiguousarray(self.reader(self.label_path(index)))
        if lab.ndim != 2 or lab.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"{self.label_path(index)}: a label image must decode to uint8 or uint16 [H,W], got {lab.dtype} {lab.shape}")
        return lab

    def read_raw(self, index):
        color_path, depth_path, _ = self.frame_paths(index)
        color = np.ascontiguousarray(self.reader(color_path))
        depth = np.ascontiguousarray(self.reader(depth_path))
        if color.ndim != 3 or color.shape[2] != 3 or color.dtype != np.uint8:
            raise ValueError(f"{color_path}: a colour image must decode to uint8 [H,W,3], got {color.dtype} {color.shape}")
        if depth.ndim != 2 or depth.dtype != np.uint16:
            raise ValueError(f"{depth_path}: a depth image must decode to uint16 [H,W] (16-bit grey PNG), got {depth.dtype} {depth.shape}")
        return color, depth, self.read_label(index) if self.semantic else None

    def _prep(self, color, depth, label):
        key = (color.shape[1:3], depth.shape[1:3], None if label is None else (label.shape[1:3], label.dtype))
        if key not in self._preps:
            self._preps[key] = FramePrep(self.cfg, key[0], key[1], None if label is None else key[2][0], self.device, self.scale,
                                         self.method)
        return self._preps[key]

    def frames(self, indices):
        """A batched read: the files of ``indices`` decoded on the host, one copy per image kind, ONE launch ->
        (indices, color [n,H,W,3], depth [n,H,W], label [n,H,W] ({} without semantics), poses [n,4,4]) on the device."""
        indices = [int(i) for i in indices]
        raws = [self.read_raw(i) for i in indices]
        up = lambda k: torch.from_numpy(np.stack([r[k] for r in raws])).to(self.device)
        color, depth = up(0), up(1)
        label = up(2) if self.semantic else None
        c, d, l = self._prep(color, depth, label)(color, depth, label, self.lut if self.semantic else None, bgr=self.bgr)
        return indices, c, d, l if self.semantic else {}, torch.stack([self.pose(i) for i in indices]).to(self.device)

    def pose(self, index):
        pose = self.poses[index].clone()
        pose[:3, 3] *= self.scale
        return pose

    def __getitem__(self, index):
        _, c, d, l, p = self.frames([index])
        return index, c[0], d[0], l[0] if self.semantic else {}, p[0]

    # cal_class_n (:211-228, :271-287)
    def label_key(self, label):
        return label

    def cal_class_n(self):
        self.label2class_dict = {}
        self.class2label_dict = {}
        self.n_class = 0
        for i in range(0, self.n_img, 5):
            label_data = self.read_label(i)
            first = ops.label_first_seen(torch.from_numpy(label_data).to(self.device), method=self.method).cpu().numpy()
            present = np.nonzero(first >= 0)[0]
            unique_labels = set()
            for v in present[np.argsort(first[present], kind="stable")]:      # first-seen order = the order flatten() feeds the set
                unique_labels.add(label_data.dtype.type(v))
            for label in unique_labels:
                key = self.label_key(label)
                if key not in self.label2class_dict.keys():
                    self.label2class_dict.update({key: self.n_class})
                    self.class2label_dict.update({self.n_class: key})
                    self.n_class += 1
        self.lut = torch.from_numpy(self.make_lut()).to(self.device)

    def make_lut(self):
        """int32 [65536]: map_function for every raw label value."""
        return np.array([self.map_function(v) for v in range(ops.LABEL_VALUES)], dtype=np.int32)

    @staticmethod
    def _pose_from(values):
        c2w = np.array(values).reshape(4, 4)
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        return torch.from_numpy(c2w).float()


class ScanNet(BaseDataset):
    def __init__(self, cfg, input_folder, scale, device="cuda:0", reader=None, method=None):
        super().__init__(cfg, input_folder, scale, device, reader, method)
        cam = cfg["cam"]
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        by_number = lambda x: int(os.path.basename(x)[:-4])
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, "color", "*.jpg")), key=by_number)
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, "depth", "*.png")), key=by_number)
        self.label_paths = sorted(glob.glob(os.path.join(self.input_folder, "label-filt", "*.png")), key=by_number)
        self.id_map = {}
        with open(self.input_folder + "/scannetv2-labels.combined.tsv", "r", newline="", encoding="utf-8") as file:
            rows = csv.reader(file, delimiter="\t")
            next(rows)
            for row in rows:
                self.id_map[int(row[0])] = int(row[4])
        self.load_poses(os.path.join(self.input_folder, "pose"))
        self.n_img = len(self.color_paths)
        self.cal_class_n()

    def frame_paths(self, index):
        f = self.input_folder
        return f"{f}/color/{index}.jpg", f"{f}/depth/{index}.png", f"{f}/label-filt/{index}.png"

    def label_key(self, label):
        return self.id_map.get(label, 0)

    def map_function(self, value):
        return self.label2class_dict.get(self.id_map.get(value, 0), 0)

    def load_poses(self, path):
        self.poses = []
        for pose_path in sorted(glob.glob(os.path.join(path, "*.txt")), key=lambda x: int(os.path.basename(x)[:-4])):
            with open(pose_path, "r") as f:
                lines = f.readlines()
            self.poses.append(self._pose_from([list(map(float, line.split(" "))) for line in lines]))


class Replica(BaseDataset):
    def __init__(self, cfg, input_folder, scale, device="cuda:0", reader=None, method=None):
        super().__init__(cfg, input_folder, scale, device, reader, method)
        self.H, self.W = cfg["cam"]["H"], cfg["cam"]["W"]
        self.hfov = 90
        self.fx = self.W / 2.0 / math.tan(math.radians(self.hfov / 2.0))      # the pin-hole camera has the same value for fx and fy
        self.fy = self.fx
        self.cx = (self.W - 1.0) / 2.0
        self.cy = (self.H - 1.0) / 2.0
        self.color_paths = sorted(glob.glob(f"{self.input_folder}/rgb/rgb_*.png"))
        self.depth_paths = sorted(glob.glob(f"{self.input_folder}/depth/depth_*.png"))
        self.n_img = len(self.color_paths)
        self.load_poses(f"{self.input_folder}/traj_w_c.txt")
        self.cal_class_n()

    def frame_paths(self, index):
        f = self.input_folder
        return f"{f}/rgb/rgb_{index}.png", f"{f}/depth/depth_{index}.png", f"{f}/semantic_class/semantic_class_{index}.png"

    def map_function(self, value):
        return self.label2class_dict.get(value, value)

    def load_poses(self, path):
        self.poses = []
        with open(path, "r") as f:
            lines = f.readlines()
        for i in range(self.n_img):
            self.poses.append(self._pose_from(list(map(float, lines[i].split()))))


dataset_dict = {
    "replica": Replica,
    "scannet": ScanNet,
}


def get_dataset(cfg, input_folder, scale, device="cuda:0", reader=None, method=None):
    return dataset_dict[cfg["dataset"]](cfg, input_folder, scale, device=device, reader=reader, method=method)
