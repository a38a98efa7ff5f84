"""The reference's top level: ``DNS_SLAM(cfg, device).run()`` (slams/dns_slam.py) with the frame loops of ``Mapper.run``
(slams/mapping.py:952-1146) and ``Tracker.run`` (slams/tracking.py:229-376), as ONE deterministic loop in one process.

The reference starts a mapping and a tracking process that hand frames to each other through shared counters.  Under
``sync_method: strict`` the interleaving is fully determined -- the tracker waits for the mapper before every frame that follows a
mapped one (tracking.py:259-263), the mapper for the tracker before every frame it maps (mapping.py:994-998) -- so the two loops
are executed here in that order by one loop, and ``schedule(n_img, cfg)`` computes the order without touching a device.  ``loose``
and ``free`` depend on the processes' timing and are refused.

Quirks of the reference as it executes, kept (each named again where it is implemented):
  * frame 0 becomes keyframe 0 at its ground-truth pose before anything is mapped (mapping.py:970-979); estimate_c2w_list[0] and
    [1] are the ground-truth poses (:972,982; tracking.py:272-273,369);
  * the first mapping pass maps FRAME 1, not frame 0: front_idx starts at 1 (dns_slam.py:54, mapping.py:991-997); it runs
    n_iters_first iterations in one outer pass, mode 'overlap' (:1020-1035); later passes run two outer passes of n_iters // 2,
    'overlap' then 'global';
  * frames 0 and 1 are never optimised by the tracker (tracking.py:272);
  * pose_init uses the constant-speed rule for idx > 2 only (tracking.py:216-227);
  * with a stem encoder the tracker's reference view is (refer_color, current frame), the second following the pose
    (tracking.py:293,316-319); ``idx - 1 % optimize_every_n_frames == 0`` (tracking.py:288) parses as
    ``idx - (1 % n) == 0``, never true for idx >= 2, so refer_color / refer_c2w stay those of frame 1 unless
    optimize_every_n_frames == 1;
  * refer_c2w of frame 1 is estimate_c2w_list[1] as the first mapping pass left it (refined if is_BA), read (tracking.py:277) before
    the tracker's loop writes the ground truth back (:369);
  * a frame is mapped when idx % optimize_every_n_frames == 0 or idx == n_img - 1 (mapping.py:994-997); afterwards, in this
    order: estimate_c2w_list[idx] = cur_c2w if is_BA (:1044), the log line (:1048-1072), frame_vis (:1075-1079), the keyframe
    (:1082-1089), the mesh (:1092-1107), the checkpoint model_{idx}.pt (:1127), and on the last frame frame_vis again --
    whatever ``verbose`` and ``vis_every`` say -- and model.pt (:1133-1145); vis and mesh need ``verbose`` (:1076,1093), mesh idx > 0,
    checkpoint idx > 1.
"""
from __future__ import annotations

import math
import os
import time

import torch

from . import synthetic
from .common import get_camera_from_tensor, get_quad_from_c2w
from .keyframes import KeyframeBank

# Whether a run's keyframe_selection_overlap scores through ops.keyframe_overlap (the bank's scorer) or the torch block, unless
# cfg['mapping']['overlap_kernel'] says otherwise.  Follows item 3 of tools/time_slam.py (profiles/slam_time.txt): the
# kernel with its [n] read takes a quarter of the torch block's time at 1600 points x 50 and x 400 keyframes.
OVERLAP_KERNEL_DEFAULT = True


def _keys(cfg, n_img):
    m = cfg["mapping"]
    sync = cfg.get("sync_method", "strict")
    if sync != "strict":
        raise NotImplementedError(f"sync_method {sync!r}: the order of a 'loose' or 'free' run depends on the two processes' timing; "
                                  "only 'strict' is a deterministic loop")
    if n_img < 2:
        raise ValueError(f"a run needs at least 2 frames (the first mapping pass maps frame 1), got {n_img}")
    k = {key: int(m.get(key, 0)) for key in ("vis_every", "mesh_every", "checkpoint_every")}
    k["every"], k["kf_every"] = int(m["optimize_every_n_frames"]), int(m["choose_keyframe_every"])
    if k["every"] < 1 or k["kf_every"] < 1:
        raise ValueError("optimize_every_n_frames and choose_keyframe_every must be >= 1")
    k["n_first"], k["n_iters"] = int(m.get("n_iters_first", m["n_iters"])), int(m["n_iters"])
    k["verbose"], k["use_gt_camera"] = bool(cfg.get("verbose", True)), bool(cfg.get("use_gt_camera", False))
    return k


def _after_map(idx, n_img, k, keyframes):
    """The events that follow the mapping of frame idx, in the reference's order (mapping.py:1075-1145)."""
    ev = []
    if k["vis_every"] > 0 and (idx % k["vis_every"] == 0 or idx <= 1) and k["verbose"]:                 # :1075-1076
        ev.append(("vis", idx))
    if (idx % k["kf_every"] == 0 or idx == n_img - 2) and idx not in keyframes:                       # :1082-1083
        keyframes.append(idx)
        ev.append(("keyframe", idx))
    if k["mesh_every"] > 0 and idx % k["mesh_every"] == 0 and idx > 0 and k["verbose"]:                # :1092-1093
        ev.append(("mesh", idx))
    if k["checkpoint_every"] > 0 and idx % k["checkpoint_every"] == 0 and idx > 1:                     # :1127
        ev.append(("checkpoint", f"model_{idx}.pt"))
    if idx == n_img - 1:                                                                               # :1133-1145, unconditional
        ev += [("vis", idx), ("checkpoint", "model.pt")]
    return ev


def schedule(n_img: int, cfg: dict) -> list:
    """The events of ``DNS_SLAM.run`` on n_img frames, in order, from the configuration alone:
    ("keyframe", idx), ("map", idx, n_iters, modes), ("track", idx), ("vis", idx), ("mesh", idx), ("checkpoint", name);
    ``modes`` is a tuple, one ``Mapper.optimize`` call of n_iters iterations per entry."""
    k = _keys(cfg, n_img)
    keyframes = [0]
    events = [("keyframe", 0)]                                            # mapping.py:970-979
    events.append(("map", 1, k["n_first"], ("overlap",)))                 # :1020-1023: is_init, front_idx = 1
    events += _after_map(1, n_img, k, keyframes)
    for idx in range(2, n_img):
        if not k["use_gt_camera"]:
            events.append(("track", idx))                                 # tracking.py:272: idx <= 1 or use_gt_camera skip
        if idx % k["every"] == 0 or idx == n_img - 1:                     # mapping.py:994-997
            events.append(("map", idx, k["n_iters"] // 2, ("overlap", "global")))
            events += _after_map(idx, n_img, k, keyframes)
    return events


def pose_init(prev_c2w: torch.Tensor, prev2_c2w: torch.Tensor, idx: int, const_speed: bool = True) -> torch.Tensor:
    """tracking.py:216-227: the pose a frame's optimisation starts from.  Constant speed for idx > 2 only: with
    pre = fl32(estimate[idx - 1]), delta = pre @ inverse(fl32(estimate[idx - 2])), the result is delta @ pre; else estimate[idx - 1].
    Evaluated where the arguments live (the driver keeps the trajectory on the host, so a run's initial poses do not depend on the
    device's inverse)."""
    if const_speed and idx > 2:
        pre = prev_c2w.float()
        delta = pre @ prev2_c2w.float().inverse()
        return (delta @ pre).detach()
    return prev_c2w.detach().clone()


def _to_c2w(cam7: torch.Tensor) -> torch.Tensor:
    """(quat, T) [7] -> [4,4] (tracking.py:346-347)."""
    return torch.cat([get_camera_from_tensor(cam7), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=cam7.dtype, device=cam7.device)], 0)


def _cam7(c2w: torch.Tensor) -> torch.Tensor:
    c2w = torch.as_tensor(c2w).detach().float().cpu()
    return torch.cat((get_quad_from_c2w(c2w), c2w[:3, 3]), 0)


class DNS_SLAM:
    """``DNS_SLAM(cfg, device).run()``.  Owns the dataset (``datasets.get_dataset`` on cfg['dataset_dir'] / dataset / scene unless
    one is passed: ``__len__``, ``__getitem__ -> (idx, color, depth, label, c2w)``, ``n_class``, ``class2label_dict``), the camera
    (``datasets.camera_from_cfg``), the bound (``synthetic.load_bound``'s rule on cfg['back_end']['bound']), ``Decoder``,
    ``Mapper``, ``Tracker``, ``Mesher`` (when cfg has 'meshing') and ``Checkpoint``, ``estimate_c2w_list`` / ``gt_c2w_list``
    [n_img,4,4] on the host, and ``keyframe_list`` / ``keyframe_dict`` (a ``keyframes.KeyframeBank``).  Two configuration keys
    are this project's own: cfg['keyframe_storage'], 'device' (default) or 'host' (the reference's CPU tensors), and
    cfg['mapping']['overlap_kernel'] (default ``OVERLAP_KERNEL_DEFAULT``): score keyframe_selection_overlap with
    ``ops.keyframe_overlap`` on the bank's pose table, or with the mapper's torch block.  ``encoder``: the frozen image stem (``encoder.ResNet``) or None.  ``n_img``: run the first
    n_img frames only.

    Scene copy: the tracker reads the mapper's decoder directly (``Tracker.frozen_scene`` keeps it unchanged while a pose is
    optimised).  The reference's ``update_para_from_mapping`` deep-copies the scene before every tracked frame only because its
    tracker is another process; in one loop the copy would be bit-identical to its source.

    Deviations: the trajectory and pose_init live on the host (the reference multiplies and inverts on the device); the tracker's
    log line carries the best total loss where the reference prints its colour and depth terms (``track_frame`` keeps the total
    only); frame_vis writes a PNG sheet without titles (``Mapper.frame_vis``); meshes are written as mesh/{idx:05d}_mesh.ply,
    where tools/visualize.py reads them."""

    def __init__(self, cfg: dict, device="cuda", dataset=None, encoder=None, n_img=None):
        from . import datasets
        from .checkpoint import Checkpoint
        from .decoder import Decoder
        from .mapping import Mapper
        from .tracking import Tracker
        self.cfg, self.device = cfg, device
        self.scene = cfg.get("scene", "scene")
        self.verbose = bool(cfg.get("verbose", True))
        # dns_slam.py:23: out_dir / dataset / scene; a key the configuration does not hold is left out of the path
        parts = [str(cfg.get("out_dir", "output"))] + [str(cfg[k]) for k in ("dataset", "scene") if k in cfg]
        self.out_dir = os.path.join(*parts)
        os.makedirs(self.out_dir, exist_ok=True)
        scale = cfg.get("scale", 1)
        if dataset is None and cfg.get("dataset") == "synthetic":          # the box room of synthetic.py: no files (configs/synthetic.yaml)
            s, c = cfg.get("synthetic", {}), cfg["cam"]
            dataset = synthetic.SyntheticSequence(n=int(s.get("n_frames", 8)), H=c["H"], W=c["W"], fx=c["fx"], step=float(s.get("step", 0.04)),
                                                  seed=int(s.get("seed", 0)), bound=cfg["back_end"]["bound"])
            if any(abs(float(c[k]) - float(dataset.cam[k])) > 1e-9 for k in ("fx", "fy", "cx", "cy")) or c.get("crop_edge", 0):
                raise ValueError(f"dataset 'synthetic' renders with the camera {dataset.cam}; cfg['cam'] must say the same, crop_edge 0")
        if dataset is None:
            dataset = datasets.get_dataset(cfg, os.path.join(cfg["dataset_dir"], cfg["dataset"], cfg["scene"]), scale, device)
        self.dataset = dataset
        self.n_class, self.class2label_dict = dataset.n_class, dataset.class2label_dict
        self.n_img = len(dataset) if n_img is None else min(int(n_img), len(dataset))
        self.keys = _keys(cfg, self.n_img)                                 # refuses 'loose' / 'free' and fewer than 2 frames
        self.cam = datasets.camera_from_cfg(cfg)
        self.bound = synthetic.load_bound(cfg["back_end"]["bound"], cfg.get("bound_divisible", 0.32), scale)
        self.decoder = Decoder(cfg["model"], self.bound, self.n_class).to(device)
        self.mapper = Mapper(cfg, self.decoder, self.bound, self.cam, device=device)
        self.mapper.encoder = encoder
        self.mapper.class2label_dict = self.class2label_dict
        self.tracker = Tracker(cfg, self.decoder, self.bound, self.cam, device=device)
        self.encoder = encoder
        self.mesher = None
        if "meshing" in cfg:
            from .meshing import Mesher
            self.mesher = Mesher(cfg, self.mapper)
        elif self.keys["mesh_every"] > 0 and self.keys["verbose"]:
            raise ValueError("mesh_every > 0 needs cfg['meshing']")
        self.checkpoint = Checkpoint(self.out_dir, device=device, decoder=self.decoder, fine_decoders=self.mapper.fine_decoders)
        self.estimate_c2w_list = torch.zeros(self.n_img, 4, 4)
        self.gt_c2w_list = torch.zeros(self.n_img, 4, 4)
        self.const_speed = bool(cfg.get("const_speed_assumption", True))
        self.plan = schedule(self.n_img, cfg)
        self.bank = None                                                   # allocated by run() from the first frame's shapes
        self.keyframe_list, self.keyframe_dict = [], []
        # the bank's scorer replaces keyframe_selection_overlap's projection block where cfg['mapping']['overlap_kernel'] asks for it
        # (DESIGN 4.29 holds the measurement the default follows)
        self.overlap_kernel = bool(cfg["mapping"].get("overlap_kernel", OVERLAP_KERNEL_DEFAULT))
        self.events = []
        self.timing = {"track": 0.0, "map": 0.0, "total": 0.0}

    # ------------------------------------------------------------------ helpers
    def _frame(self, i):
        idx, color, depth, label, c2w = self.dataset[i]
        dev = self.device
        return color.to(dev), depth.to(dev), label.to(dev), torch.as_tensor(c2w).float()

    def _emit(self, on_event, ev, payload=None):
        self.events.append(ev)
        if on_event is not None:
            on_event(ev, payload if payload is not None else {})

    def _log(self, name, line):
        with open(os.path.join(self.out_dir, name), "a") as f:
            f.write(line)

    def _make_bank(self, color, label):
        cap = sum(1 for e in self.plan if e[0] == "keyframe")
        self.bank = KeyframeBank(cap, color.shape[0], color.shape[1], self.n_class, self.device,
                                 storage=self.cfg.get("keyframe_storage", "device"), label_dtype=label.dtype)
        self.keyframe_dict, self.keyframe_list = self.bank.as_list(), self.bank.frame_idx
        self.mapper.keyframe_dict, self.mapper.keyframe_list = self.keyframe_dict, self.keyframe_list
        if self.overlap_kernel:
            self.mapper.overlap_scorer = self.bank.overlap_scorer(self.cam)

    def _checkpoint(self, name, idx):
        # the reference's keyword set (mapping.py:1119-1125); fine_decoders is written by Checkpoint from the mapper's pool
        return self.checkpoint.save(name, scene=self.scene, idx=idx, keyframe_dict=self.bank.host_copy(),
                                    keyframe_list=list(self.keyframe_list), estimate_c2w_list=self.estimate_c2w_list.clone(),
                                    gt_c2w_list=self.gt_c2w_list.clone())

    def _mesh(self, idx):
        m = self.cfg["meshing"]
        folder = os.path.join(self.out_dir, "mesh")
        paths = self.mesher.get_mesh(folder, self.keyframe_dict, idx, color=m.get("color", True), clean_mesh=m.get("clean_mesh", True),
                                     stem=True if self.encoder is not None else None)
        final = os.path.join(folder, f"{idx:05d}_mesh.ply")                # where tools/visualize.py looks
        os.replace(paths[0], final)
        return final

    # ------------------------------------------------------------------ the two loop bodies
    def _track(self, idx, frame, state, on_event):
        color, depth, label, gt_c2w = frame
        every = self.keys["every"]
        if every == 1:                                                     # tracking.py:288: never true through its first operand
            state["refer_color"], state["refer_c2w"] = state["pre_color"], self.estimate_c2w_list[idx - 1].clone()
        init = pose_init(self.estimate_c2w_list[idx - 1], self.estimate_c2w_list[idx - 2], idx, self.const_speed)
        cur = {"gt_color": color, "gt_depth": depth, "gt_label": label}
        features = refer = None
        if self.encoder is not None:                                       # tracking.py:293-296,316-319
            with torch.no_grad():
                features = self.encoder(torch.stack((state["refer_color"], color), 0)[None].to(self.device))
            w2c = torch.stack((torch.inverse(state["refer_c2w"].float()), torch.inverse(init.float())), 0)
            refer = {"est_w2c": w2c.to(self.device), "follow": (False, True)}
        t0 = time.perf_counter()
        cam7, best = self.tracker.track_frame(cur, init, features=features, refer_frames=refer)
        got = torch.cat((cam7.detach().reshape(-1), best.detach().reshape(-1))).cpu()        # the ONE host read of a tracked frame
        elapsed = time.perf_counter() - t0
        self.timing["track"] += elapsed
        c2w = _to_c2w(got[:7])                                             # keep-best pose (tracking.py:331-336,346-347)
        self.estimate_c2w_list[idx] = c2w                                  # :369
        self.gt_c2w_list[idx] = gt_c2w                                     # :370
        state["pre_color"] = color                                         # :352
        if self.verbose:                                                   # :354-367
            gt7 = _cam7(gt_c2w)
            before, after = float((gt7 - _cam7(init)).abs().mean()), float((gt7 - got[:7]).abs().mean())
            # the reference's fields (:361-366), with the best TOTAL loss where it prints the colour and depth terms and their psnr
            self._log("output_front.txt", f"Current frame: {idx} FRONT END: loss: {float(got[7]):.4f} "
                                          f"ATE before: {before:.6f} after: {after:.6f} "
                                          f"time elapsed: total {self.timing['track']} current {elapsed}\n")
        self._emit(on_event, ("track", idx), {"init_c2w": init, "camera_tensor": got[:7], "loss": got[7]})

    def _map(self, ev, frame, on_event):
        _, idx, n_iters, modes = ev
        color, depth, label, gt_c2w = frame
        cur_c2w = self.estimate_c2w_list[idx].clone()                      # mapping.py:1010
        t0 = time.perf_counter()
        for mode in modes:                                                 # :1031-1038
            self.mapper.mapping_mode = mode
            cur_c2w, loss = self.mapper.optimize(n_iters, idx, color, depth, label, gt_c2w.to(self.device), cur_c2w)
        names = [n for n in ("p_loss", "d_loss", "l_loss", "lt_loss", "smooth_loss") if n in loss]
        if self.verbose:                                                   # pose and log terms in ONE host read
            terms = [torch.as_tensor(loss[n]).detach().to(device=cur_c2w.device, dtype=torch.float32).reshape(1) for n in names]
            got = torch.cat([cur_c2w.detach().reshape(-1).float()] + terms).cpu()
        elif self.mapper.is_BA:
            got = cur_c2w.detach().reshape(-1).float().cpu()
        else:
            got = None
        elapsed = time.perf_counter() - t0
        self.timing["map"] += elapsed
        if self.mapper.is_BA:                                              # :1044-1045
            self.estimate_c2w_list[idx] = got[:16].reshape(4, 4)
        if self.verbose:                                                   # :1048-1072
            vals = {n: float(v) for n, v in zip(names, got[16:])}
            psnr = -10.0 * math.log10(vals["p_loss"]) if vals.get("p_loss", 0.0) > 0.0 else float("inf")     # mse2psnr
            # the reference's line, field for field (:1064-1071; "rgh" is its spelling)
            self._log("output_back_fine.txt", f"{self.scene} Current frame: {idx} BACK END: rgh loss: {vals.get('p_loss', float('nan')):.4f} "
                      f"psnr: {psnr:.4f} depth loss: {vals.get('d_loss', float('nan')):.4f} "
                      f"label loss: {vals.get('l_loss', float('nan')):.4f} coarse2fine loss: {vals.get('lt_loss', float('nan')):.4f} "
                      f"ATE: {float(loss['loss_camera_tensor']):.6f} "
                      f"time elapsed: total {self.timing['map']} current {elapsed}\n")
        self._emit(on_event, ev, dict(loss))
        return cur_c2w

    # ------------------------------------------------------------------ run
    def run(self, on_event=None):
        """Executes ``self.plan`` (= ``schedule(n_img, cfg)``); every event is appended to ``self.events`` as it is executed and
        passed, with a payload dict, to ``on_event(event, payload)``: for "track" init_c2w, camera_tensor (the best (quat, T)) and
        loss; for "map" the loss dict of the last ``optimize`` call.  Returns ``estimate_c2w_list``."""
        t_run = time.perf_counter()
        n_img = self.n_img
        frame0 = self._frame(0)
        self._make_bank(frame0[0], frame0[2])
        self.gt_c2w_list[0] = frame0[3]                                    # mapping.py:970-972
        self.estimate_c2w_list[0] = frame0[3]
        frame = self._frame(1)
        self.gt_c2w_list[1] = frame[3]                                     # :980-982
        self.estimate_c2w_list[1] = frame[3]
        state = {"pre_color": frame[0], "refer_color": frame[0], "refer_c2w": None}       # tracking.py:272-278 at idx = 1
        if self.keys["use_gt_camera"]:
            # tracking.py:272-273,369-370: the tracker's loop optimises nothing and writes the ground truth for EVERY frame
            for i in range(2, n_img):
                self.gt_c2w_list[i] = torch.as_tensor(self.dataset[i][4]).float()
                self.estimate_c2w_list[i] = self.gt_c2w_list[i]
        cur_idx, cur_c2w = 1, None
        for ev in self.plan:
            kind, idx = ev[0], ev[1]
            if kind in ("track", "map") and idx != cur_idx:
                frame, cur_idx = self._frame(idx), idx
            if kind == "keyframe":
                src = frame0 if idx == 0 else frame
                pose = src[3] if idx == 0 else cur_c2w                     # keyframe 0: ground truth; later ones: the mapped pose (:1089)
                self.bank.add(idx, src[0], src[1], src[2], src[3], pose)
                self._emit(on_event, ev)
            elif kind == "map":
                cur_c2w = self._map(ev, frame, on_event)
                if idx == 1:
                    # tracking.py:277 reads estimate[1] as the first pass left it; :369 then writes the ground truth back
                    state["refer_c2w"] = self.estimate_c2w_list[1].clone()
                    self.estimate_c2w_list[1] = frame[3]
            elif kind == "track":
                self._track(idx, frame, state, on_event)
            elif kind == "vis":
                self.mapper.frame_vis(idx, frame[0], frame[1], frame[2], frame[3], cur_c2w, out_dir=self.out_dir)
                self._emit(on_event, ev)
            elif kind == "mesh":
                self._emit(on_event, ev, {"path": self._mesh(idx)})
            elif kind == "checkpoint":
                self._emit(on_event, ev, {"path": self._checkpoint(ev[1], cur_idx)})   # ev[1]: the file name
        self.timing["total"] = time.perf_counter() - t_run
        return self.estimate_c2w_list

