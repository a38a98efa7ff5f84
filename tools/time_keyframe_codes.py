"""The keyframe codes of the mesh vertex query (csrc/mesh_feature.hip, ops.keyframe_codes) at the reference's scale: 1.2 M
points x 50 keyframes with 340 x 600 stem maps -- ms for the pair list (count + prefix + emit), the rows, the network
(OneBlob + Merge MLP) and the mean, and for the whole call -- against the torch composition of the same steps (the
per-keyframe loop of tests/kf_codes_ref.py, with the four bilinear taps gathered from the half-resolution map instead of the
full-resolution up-sample); then Mesher.extract at 256^3 with and without ``stem``.  Companion of tools/time_mesh.py.

    python tools/time_keyframe_codes.py [--points 1200000] [--kf 50] [--H 680] [--W 1200] [--res 256] [--reps 3] [--no-extract]
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic                      # noqa: E402
from dns_slam_amd._lib import check, lib, ptr, stream_ptr    # noqa: E402
from dns_slam_amd.decoder import Decoder                     # noqa: E402
from dns_slam_amd.encoder import ResNet                      # noqa: E402
from dns_slam_amd.mapping import Mapper                      # noqa: E402
from dns_slam_amd.meshing import Mesher                      # noqa: E402
import kf_codes_ref                                          # noqa: E402
from util import randomise_                                  # noqa: E402


def timed(fn, reps):
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


@torch.no_grad()
def torch_codes(pts, w2c, org, dep, stem, cam, merge):
    """get_2d_feature as torch ops on the device, keyframe by keyframe; the stem value at the rounded pixel comes from four
    gathered taps of the half-resolution map (align_corners=True), not from an up-sampled copy."""
    Kn, H, W = dep.shape
    h, w = stem.shape[1:3]
    code = torch.zeros(pts.shape[0], merge.decoder.n_output_dims, device=pts.device)
    count = torch.zeros(pts.shape[0], device=pts.device)
    for k in range(Kn):
        c = pts @ w2c[k, :3, :3].T + w2c[k, :3, 3]
        z = c[:, 2] + 1e-8
        u = (cam["fx"] * -c[:, 0] + cam["cx"] * c[:, 2]) / z
        v = (cam["fy"] * c[:, 1] + cam["cy"] * c[:, 2]) / z
        seen = (u < W) & (u > 0) & (v < H) & (v > 0) & (z < 0)
        iu = torch.round(u[seen]).long().clamp(0, W - 1)
        iv = torch.round(v[seen]).long().clamp(0, H - 1)
        d, dp = dep[k, iv, iu], -z[seen]
        trunc = ~(dp < d * 0.95) & ~(dp > d * 1.05)
        idx = torch.nonzero(seen)[:, 0][trunc]
        iu, iv = iu[trunc], iv[trunc]
        sx, sy = iu.float() * ((w - 1) / (W - 1)), iv.float() * ((h - 1) / (H - 1))
        x0, y0 = sx.long(), sy.long()
        lx, ly = (sx - x0)[:, None], (sy - y0)[:, None]
        x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
        m = stem[k]
        ft = (1 - ly) * ((1 - lx) * m[y0, x0] + lx * m[y0, x1]) + ly * ((1 - lx) * m[y1, x0] + lx * m[y1, x1])
        lat = merge((pts[idx] - org[k])[None], org[k:k + 1], ft[None])
        code[idx] += lat
        count[idx] += 1
    code[count > 0] /= count[count > 0, None]
    return code, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1200000)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--H", type=int, default=680)
    ap.add_argument("--W", type=int, default=1200)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-extract", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    cam = synthetic.camera(H=a.H, W=a.W, fx=a.W / 2.0, fy=a.W / 2.0)
    bound, cam, frames = synthetic.make_scene(a.kf, cam=cam, seed=1)
    cfg = synthetic.default_cfg()
    dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
    mapper = Mapper(cfg, dec, bound, cam, device=dev)
    mapper.set_decoder(frames)
    randomise_(dec, 1)
    randomise_([mapper.fine_decoders.pool], 2)
    cfg["meshing"] = {"resolution": a.res, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True}
    kfs = [{k: frames[k][i] for k in ("est_c2w", "gt_label", "gt_depth", "gt_color")} for i in range(a.kf)]
    m = Mesher(cfg, mapper)
    enc = ResNet(seed=0).to(dev)
    merge = dec.merge
    t_stem, stem = timed(lambda: m.keyframe_stem(kfs, enc), 1)
    w2c, _, _, dep, org, _ = m._keyframes(kfs, stem)
    pts = kf_codes_ref.mixed_points(a.points, kfs, cam, bound, torch.Generator().manual_seed(0)).to(dev)
    P, Kn, H, W = pts.shape[0], a.kf, a.H, a.W
    h, w, Cc = stem.shape[1:]
    reps = a.reps
    intr = (C.c_float * 4)(cam["fx"], cam["fy"], cam["cx"], cam["cy"])

    # ---- the passes alone, on one chunk-free list (the whole of the points; the product call chunks by its workspace budget)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    t_count, _ = timed(lambda: check(lib.dns_kf_pair_count(ptr(pts), P, ptr(w2c), Kn, ptr(dep), H, W, intr, ptr(count), stream_ptr())), reps)
    incl = torch.cumsum(count, 0, dtype=torch.int64)
    offset = incl - count
    n = int(incl[-1])
    rec = torch.empty(max(n, 1), 4, dtype=torch.int32, device=dev)
    t_emit, _ = timed(lambda: check(lib.dns_kf_pair_emit(ptr(pts), P, ptr(w2c), Kn, ptr(dep), H, W, intr, ptr(offset), ptr(rec), n,
                                                          stream_ptr())), reps)
    t_list, _ = timed(lambda: ops.keyframe_pairs(pts, w2c, dep, cam), reps)
    ld, n_pe, hid = merge.decoder.n_input_dims, merge.pe_dim, merge.decoder.n_output_dims
    rows, rel = torch.empty(max(n, 1), ld, device=dev), torch.empty(max(n, 1), 3, device=dev)
    t_rows, _ = timed(lambda: check(lib.dns_kf_pair_rows(ptr(rec), n, ptr(pts), P, ptr(org), Kn, ptr(stem), Cc, h, w, H, W, ptr(rel),
                                                          C.c_void_p(rows.data_ptr() + 4 * n_pe), ld, stream_ptr())), reps)
    b6 = ops._bound6(merge.bound)
    t_pe, _ = timed(lambda: check(lib.dns_encode_fwd(ptr(rel), b6, n, merge.pe_fn.n_bins, None, None, None, ptr(rows), ld, None, 0,
                                                      None, stream_ptr())), reps)
    with torch.no_grad():
        t_mlp, lat = timed(lambda: merge.decoder(rows[:n]), reps)
    code = torch.empty(P, hid, device=dev)
    t_mean, _ = timed(lambda: check(lib.dns_kf_code_mean(ptr(lat), lat.stride(0), n, ptr(offset), ptr(count), P, hid, ptr(code),
                                                          stream_ptr())), reps)
    t_all, (code_p, count_p) = timed(lambda: ops.keyframe_codes(pts, w2c, org, dep, stem, cam, merge), reps)
    t_torch, (code_t, count_t) = timed(lambda: torch_codes(pts, w2c, org, dep, stem, cam, merge), 1)
    same = (count_p.float() == count_t)
    err = float((code_p[same] - code_t[same]).abs().max() / code_t.abs().max())
    chunk = min(max((ops.KF_WORKSPACE_BYTES // (4 * (ld + hid + 7))) // Kn, 1), P)
    print(f"{P} points x {Kn} keyframes, {H} x {W} images, stem maps {h} x {w} x {Cc} ({stem.numel() * 4 / 1e6:.0f} MB, "
          f"{t_stem:.1f} ms to compute), {torch.cuda.get_device_name()}")
    print(f"  {n} pairs ({n / P:.2f} per point, {100.0 * n / (P * Kn):.2f} % of the {P * Kn} candidates); "
          f"{int((count > 0).sum())} points with a pair")
    print(f"  pair count                                  {t_count:8.3f} ms")
    print(f"  pair emit                                   {t_emit:8.3f} ms")
    print(f"  pair list (count + cumsum + host read + emit + int64 columns) {t_list:8.3f} ms")
    print(f"  rows (relative point + 4 taps x {Cc} channels)  {t_rows:8.3f} ms   {t_rows * 1e6 / max(n, 1):.2f} ns per pair, "
          f"{n * (4 * Cc * 4 + Cc * 4 + 28) / t_rows / 1e6:.0f} GB/s of taps read + row written")
    print(f"  OneBlob into the rows                       {t_pe:8.3f} ms")
    print(f"  Merge network {ld} -> {merge.decoder.n_neurons} -> {hid}                 {t_mlp:8.3f} ms   {t_mlp * 1e6 / max(n, 1):.2f} ns per row")
    print(f"  mean over the segments                      {t_mean:8.3f} ms")
    print(f"  ops.keyframe_codes ({(P + chunk - 1) // chunk} chunks of {chunk} points)   {t_all:8.3f} ms")
    print(f"  torch composition, keyframe by keyframe     {t_torch:8.3f} ms   (codes agree to {err:.1e} of their scale on the "
          f"{int(same.sum())} points with equal counts, {int((~same).sum())} counts differ)")
    if a.no_extract:
        return
    mapper.encoder = None
    t_plain, out0 = timed(lambda: m.extract(kfs), reps)
    mapper.encoder = enc
    t_stem_given, out1 = timed(lambda: m.extract(kfs, stem=stem), reps)
    t_stem_true, _ = timed(lambda: m.extract(kfs, stem=True), 1)
    kf = m._keyframes(kfs, stem)
    v = out1[0] * m.scale
    t_vq0, _ = timed(lambda: m.vertex_query(v, kf[:3]), reps)
    t_vq1, _ = timed(lambda: m.vertex_query(v, kf, stem=stem), reps)
    print(f"extract at {a.res}^3, {Kn} keyframes: {out1[0].shape[0]} vertices, {out1[1].shape[0]} faces "
          f"(same mesh without stem: {torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])})")
    print(f"  extract without stem                        {t_plain:8.2f} ms   (vertex query {t_vq0:.2f} ms)")
    print(f"  extract with stem = the maps                {t_stem_given:8.2f} ms   (vertex query {t_vq1:.2f} ms)")
    print(f"  extract with stem = True (maps computed)    {t_stem_true:8.2f} ms")


if __name__ == "__main__":
    main()
