"""The C-ABI launch sequence of MapStep / TrackStep, one line per call, for comparing two trees.

A recording proxy takes the place of ``ops.lib`` (and of its ``_raw``), two consecutive steps of every configuration below run
from fixed seeds, and every call -- of the constructor and of the steps, size queries aside -- is printed in host order as
``entry(arg, ...)``.  Integers and floats are printed by value, ctypes arrays by contents, structs passed by reference field
by field, and every distinct pointer value (stream handles and interior pointers such as ``buf + 4 * pe`` included) as ``p<k>``,
k = its order of first appearance within the configuration.  Two trees whose steps are the same launch sequence print the same
text: run it on both and ``diff`` the outputs.  Torch-level work (events, stream waits, fills, index_select, the generator)
is not seen; the step tests cover that.

    python tools/launch_log.py [--out FILE] [--only SUBSTRING]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from dns_slam_amd import ops  # noqa: E402

DEV = "cuda"
_QUERIES = ("dns_abi_version", "dns_last_error", "dns_init", "dns_grid_meta_init", "dns_device_error")


class Log:
    def __init__(self, out):
        self.out, self.ids, self.lines = out, {}, 0

    def begin(self, name):
        self.ids = {}
        self.out.write(f"== {name}\n")
        self.lines += 1

    def pointer(self, value):
        if not value:
            return "null"
        if value not in self.ids:
            self.ids[value] = len(self.ids)
        return f"p{self.ids[value]}"

    def fmt(self, v):
        if v is None:
            return "null"
        if isinstance(v, (bool, int)):
            return str(int(v))
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, C.c_void_p):
            return self.pointer(v.value)
        if isinstance(v, C.Structure):
            parts = []
            for name, typ in v._fields_:
                val = getattr(v, name)
                parts.append(f"{name}={self.pointer(val) if typ is C.c_void_p else self.fmt(val)}")
            return "{" + ", ".join(parts) + "}"
        if isinstance(v, C.Array):
            return "[" + ", ".join(self.fmt(e) for e in v) + "]"
        if isinstance(v, C._Pointer):
            return "*" + self.fmt(v.contents) if v else "null"
        if isinstance(v, C._SimpleCData):
            return self.fmt(v.value)
        if hasattr(v, "_obj"):                             # ctypes.byref(...)
            return "&" + self.fmt(v._obj)
        raise TypeError(f"launch_log: argument of type {type(v).__name__}")

    def call(self, name, args):
        self.out.write(f"{name}({', '.join(self.fmt(a) for a in args)})\n")
        self.lines += 1


class Recorder:
    """Forwards every attribute to ``inner``; calls of dns_* entry points are logged first."""

    def __init__(self, inner, log, raw=None):
        self.__dict__.update(_inner=inner, _log=log, _raw_proxy=raw)

    def __getattr__(self, name):
        if name == "_raw" and self._raw_proxy is not None:
            return self._raw_proxy
        target = getattr(self._inner, name)
        if not name.startswith("dns_") or name in _QUERIES or name.endswith(("_floats", "_bytes")) or name.startswith("dns_kernel_timing"):
            return target

        def logged(*a):
            self._log.call(name, a)
            return target(*a)
        return logged

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _mapper(nn=32, nl=1, dtype="fp32"):
    """The shape of tests/test_gpu_slam._setup: 4 frames x 360 rays, 32 + 15 samples, smooth_pts 12, hash 2^14."""
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.mapping import Mapper
    from util import randomise_
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=0)
    cfg = synthetic.default_cfg(n_pixels=360, n_samples_ray=32, n_surface_ray=15, n_frames=4, hash_size=14, voxel_size=0.08,
                                n_neurons=nn, n_hidden_layers=nl, smooth_pts=12, mlp_dtype=dtype)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    mapper = Mapper(cfg, dec, bound, cam, device=DEV)
    mapper.set_decoder(frames)
    randomise_(dec, 11, scale=1.0)
    with torch.no_grad():
        dec.pe_fn.grid_fn.params.mul_(2000.0)
    randomise_([mapper.fine_decoders.pool], 12)
    return mapper, frames


def map_config(log, name, nn=32, nl=1, dtype="fp32", code=False, stem=False, BA=True, two_streams=True, smooth=True,
               half_rows=None, prepared=None, **kw):
    from dns_slam_amd.fused_step import MapStep
    refer = feats = None
    if stem:
        from test_gpu_features import _stem_setup
        _, _, _, frames, _, mapper, refer, feats = _stem_setup(nn=nn, nl=nl)
    else:
        mapper, frames = _mapper(nn, nl, dtype)
    mapper.static_shapes, mapper.is_BA = True, BA
    mapper.overlap_smooth = mapper.prefetch_draws = two_streams
    if prepared is not None:
        mapper.prepared_images = prepared
    if half_rows is not None:
        os.environ["DNS_HALF_ROWS"] = half_rows
    _, ql, Tl = mapper.set_optimizer(frames, fused=True)
    prep = mapper.prepare_frames(frames)
    if code:
        npf = prep["n1"] + prep["n2"]
        feats = (torch.rand(4 * npf, 32 + 15, 32, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    _seed(123)
    torch.cuda.synchronize()
    log.begin(name)
    ms = MapStep(mapper, frames, ql, Tl, prep=prep, features=feats, refer_frames=refer, smooth=smooth, **kw)
    ms.step()
    ms.step()
    torch.cuda.synchronize()
    os.environ.pop("DNS_HALF_ROWS", None)
    return ms


def track_config(log, name, code=False, stem=False, fused=False):
    from test_gpu_slam import _setup
    from dns_slam_amd.fused_step import TrackStep
    from dns_slam_amd.tracking import Tracker
    refer = feats = None
    if stem:                                               # test_track_step_with_stem_features_equals_the_tracker_loop
        from dns_slam_amd.encoder import ResNet
        from util import randomise_
        cfg, bound, cam, frames, dec, _ = _setup()
        randomise_(dec.merge, 21)
        tracker = Tracker(cfg, dec, bound, cam, device=DEV)
        cur = {k: frames[k][1] for k in ("gt_color", "gt_depth", "gt_label")}
        views = torch.stack([frames["gt_color"][0], frames["gt_color"][1], frames["gt_color"][2]])[None].to(DEV)
        feats = ResNet(seed=3).to(DEV)(views).detach()
        refer = {"est_w2c": torch.stack([torch.inverse(frames["est_c2w"][k].float()) for k in (0, 1, 2)]).to(DEV)}
        c2w = frames["est_c2w"][1].clone()
        c2w[:3, 3] += 0.02
    else:                                                  # test_track_step_equals_the_tracker_loop
        cfg, bound, cam, frames, dec, _ = _setup(64, 2, n_pixels=400)
        cfg["tracking"]["n_pixels"] = 256
        tracker = Tracker(cfg, dec, bound, cam, device=DEV)
        tracker.border = 5
        cur = {k: frames[k][2] for k in ("gt_color", "gt_depth", "gt_label")}
        c2w = frames["est_c2w"][2].clone()
        c2w[:3, 3] += torch.tensor([0.02, -0.01, 0.015], dtype=c2w.dtype)
        if code:
            feats = (torch.rand(256, 32 + 15, 32, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV)
    tracker.static_shapes = True
    _seed(3)
    torch.cuda.synchronize()
    log.begin(name)
    with tracker.frozen_scene():
        ts = TrackStep(tracker, cur, c2w, features=feats, refer_frames=refer)
        if fused:
            assert ts.fused_supported()
            ts.run_fused(2)
        else:
            ts.step()
            ts.step()
    torch.cuda.synchronize()
    return ts


CONFIGS = [
    ("map fp32 32x1 code BA two-streams", lambda log, n: map_config(log, n, code=True)),
    ("map fp32 32x1 live one-stream", lambda log, n: map_config(log, n, two_streams=False)),
    ("map fp32 32x1 live two-streams", lambda log, n: map_config(log, n)),
    ("map is_BA=False", lambda log, n: map_config(log, n, BA=False)),
    ("map smooth=False", lambda log, n: map_config(log, n, smooth=False)),
    ("map keep_hidden", lambda log, n: map_config(log, n, nn=64, nl=2, keep_hidden=True)),
    ("map prepared_images=False", lambda log, n: map_config(log, n, code=True, prepared=False)),
    ("map split_rows code", lambda log, n: map_config(log, n, code=True, split_rows=True)),
    ("map split_rows live", lambda log, n: map_config(log, n, nn=64, nl=2, split_rows=True)),
    ("map split_rows one-stream", lambda log, n: map_config(log, n, code=True, split_rows=True, two_streams=False)),
    ("map fp16 64x2 half rows", lambda log, n: map_config(log, n, nn=64, nl=2, dtype="fp16", half_rows="1")),
    ("map fp16 64x2 half rows one-stream", lambda log, n: map_config(log, n, nn=64, nl=2, dtype="fp16", half_rows="1", two_streams=False)),
    ("map fp16 64x2 operand", lambda log, n: map_config(log, n, nn=64, nl=2, dtype="fp16", half_rows="0")),
    ("map fp16 64x2 operand split_rows", lambda log, n: map_config(log, n, nn=64, nl=2, dtype="fp16", half_rows="0", split_rows=True)),
    ("map stem BA two-streams", lambda log, n: map_config(log, n, stem=True)),
    ("map stem BA one-stream", lambda log, n: map_config(log, n, stem=True, two_streams=False)),
    ("track step", lambda log, n: track_config(log, n)),
    ("track step code", lambda log, n: track_config(log, n, code=True)),
    ("track step stem", lambda log, n: track_config(log, n, stem=True)),
    ("track run_fused(2)", lambda log, n: track_config(log, n, fused=True)),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the log to this file instead of stdout")
    ap.add_argument("--only", default=None, help="run the configurations whose name contains this")
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    log = Log(out)
    inner = ops.lib
    ops.lib = Recorder(inner, log, raw=Recorder(inner._raw, log))
    try:
        for name, run in CONFIGS:
            if args.only is None or args.only in name:
                n0 = log.lines
                run(log, name)
                print(f"{name}: {log.lines - n0 - 1} calls", file=sys.stderr)
    finally:
        ops.lib = inner
        if args.out:
            out.close()
    print(f"{log.lines} lines", file=sys.stderr)


if __name__ == "__main__":
    main()
