"""Depth L1 on the 256^3 mesh tools/time_mesh.py builds (the synthetic room, cleaned) and a perturbed copy of it: ms for
ops.rasterize_depth with method="auto" against method="simple" at V views of 500 x 500 drawn by evaluation.sample_views inside
the mesh's view box, ops.depth_l1 on the two stacks, and the whole evaluation.calc_2d_metric; checks that the two methods
return the same bits.

    python tools/time_raster.py [--res 256] [--kf 50] [--ply FILE.ply] [--views 16] [--hw 500] [--reps 3] [--once]
    (--ply: time that mesh instead; --once: one calc_2d_metric without alignment, for a profiler run)
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import evaluation as E, ops              # noqa: E402


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def synthetic_mesh(res, kf, dev):
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.mapping import Mapper
    from dns_slam_amd.meshing import Mesher
    from util import randomise_
    cam = synthetic.camera(H=120, W=160, fx=120.0, fy=120.0)
    bound, cam, frames = synthetic.make_scene(kf, cam=cam, seed=1)
    cfg = synthetic.default_cfg()
    dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
    mapper = Mapper(cfg, dec, bound, cam, device=dev)
    mapper.set_decoder(frames)
    randomise_(dec, 1)
    randomise_([mapper.fine_decoders.pool], 2)
    cfg["meshing"] = {"resolution": res, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True,
                      "remove_small_geometry_threshold": 0.2}
    kfs = [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i]}
           for i in range(kf)]
    v, f, _, _ = Mesher(cfg, mapper).extract(kfs)
    return v, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--ply")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--hw", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    if a.ply:
        m = E.read_ply(a.ply)
        v, f = torch.from_numpy(m["verts"]).to(dev), torch.from_numpy(m["faces"]).to(dev)
    else:
        v, f = synthetic_mesh(a.res, a.kf, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    v2 = v + torch.randn(v.shape, device=dev, generator=g) * 0.01         # the "reconstruction": 1 cm of noise per coordinate
    H = W = a.hw
    kw = dict(H=H, W=W, focal=300.0 * a.hw / 500.0)
    if a.once:
        out = E.calc_2d_metric(v2, f, v, f, align=False, n_imgs=a.views, **kw)
        torch.cuda.synchronize()
        print(out["depth_l1_cm"])
        return
    extents, transform = E.view_box(v)
    c2w = E.sample_views(extents, transform, a.views, seed=0)
    w2c = torch.from_numpy(E.world_to_camera(c2w, flip_yz=False)).to(dev)
    cam = (H, W, kw["focal"], kw["focal"], H / 2.0 - 0.5, W / 2.0 - 0.5)
    t_auto, (d_auto, st) = timed(lambda: ops.rasterize_depth_launch(v, f, w2c, *cam), a.reps)
    t_simple, (d_simple, _) = timed(lambda: ops.rasterize_depth_launch(v, f, w2c, *cam, method="simple"), 1)
    same = bool(torch.equal(d_auto.view(torch.int32), d_simple.view(torch.int32)))
    _, st2 = ops.rasterize_depth(v, f, w2c, *cam, return_stats=True)
    d_rec, _ = ops.rasterize_depth_launch(v2, f, w2c, *cam)
    t_l1, err = timed(lambda: ops.depth_l1(d_auto, d_rec), a.reps)
    t_dl1, res = timed(lambda: E.depth_l1(v2, f, v, f, c2w, **kw), a.reps)
    t_all, full = timed(lambda: E.calc_2d_metric(v2, f, v, f, align=True, n_imgs=a.views, **kw), 1)
    pairs = f.shape[0] * a.views
    print(f"mesh: {v.shape[0]} vertices, {f.shape[0]} faces; {a.views} views of {H} x {W}; {torch.cuda.get_device_name()}")
    print(f"  rasterize_depth, auto     {t_auto:10.3f} ms   ({t_auto / a.views:.3f} ms per view, {pairs / t_auto * 1e-6:.2f} G set-ups/s; "
          f"{st2['small']} pairs by their set-up thread, {st2['large']} through the list; covered pixels {float((d_auto > 0).float().mean()):.4f})")
    print(f"  rasterize_depth, simple   {t_simple:10.3f} ms   (same bits: {same}; auto is {t_simple / t_auto:.2f} x faster)")
    print(f"  depth_l1 (two stacks)     {t_l1:10.3f} ms   ({2 * d_auto.numel() * 4 / t_l1 * 1e-6:.1f} GB/s)")
    print(f"  evaluation.depth_l1       {t_dl1:10.3f} ms   (two meshes, one host read; Depth L1 {res['depth_l1_cm']:.4f} cm)")
    print(f"  calc_2d_metric, aligned   {t_all:10.3f} ms   (ICP, {a.views} views sampled, Depth L1 {full['depth_l1_cm']:.4f} cm)")
    if not same:
        sys.exit("the two methods differ")


if __name__ == "__main__":
    main()
