"""ops.mesh_fill_holes by kernel (HIP events round every launch, the library's dns_kernel_timing): the median, minimum and maximum
of 20 calls after a warm-up, on the 512 x 256 torus of tests/test_gpu_fill_holes.py (every 53rd cell's lower face removed) and on the
cleaned mesh of Mesher.extract on the synthetic room (tools/time_mesh.py's set-up).  Next to it, on the same meshes:
ops.mesh_components by kernel (its cc_edges builds the same edge table), both ops' wall time per call with their host read, and
the host restatement tests/fill_holes_ref.py.

    python tools/time_fill_holes.py [--res 256] [--kf 50] [--reps 20] [--no-room]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dns_slam_amd import ops, synthetic                      # noqa: E402
import fill_holes_ref as fr                                  # noqa: E402


def kernel_times(fn, reps):
    """{kernel: [ms per call]} over ``reps`` calls of fn after one warm-up call, and the wall ms per call (host read included)."""
    fn()
    torch.cuda.synchronize()
    per, wall = {}, []
    for _ in range(reps):
        ops.timer.arm(kernels=True)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        ops.timer.disarm()
        once = {}
        for _, kern, ms, _, _ in ops.timer.kernel_spans:
            once[kern] = once.get(kern, 0.0) + ms
        for k, ms in once.items():
            per.setdefault(k, []).append(ms)
    return per, wall


def wall_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def line(name, ms):
    ms = np.asarray(ms)
    return f"    {name:28s} {np.median(ms):8.3f} ms   ({ms.min():.3f} .. {ms.max():.3f})"


def report(title, verts, faces, reps):
    V, F = int(verts.shape[0]), int(faces.shape[0])
    out, info = ops.mesh_fill_holes(faces, V)
    print(f"{title}: {V} vertices, {F} faces, {info['boundary_edges']} boundary edges, {info['loops_filled']} loops filled with "
          f"{info['faces_added']} faces, {info['vertices_skipped']} vertices skipped")
    per, _ = kernel_times(lambda: ops.mesh_fill_holes(faces, V), reps)
    print("  ops.mesh_fill_holes, by kernel (median of %d, min .. max):" % reps)
    for k, ms in per.items():
        print(line(k, ms))
    print(line("all kernels", np.sum([ms for ms in per.values()], 0)))
    print(line("whole call, with its host read", wall_times(lambda: ops.mesh_fill_holes(faces, V), reps)))
    per, _ = kernel_times(lambda: ops.mesh_components(verts, faces), reps)
    print("  ops.mesh_components, by kernel:")
    for k, ms in per.items():
        print(line(k, ms))
    print(line("all kernels", np.sum([ms for ms in per.values()], 0)))
    print(line("whole call, with its host read", wall_times(lambda: ops.mesh_components(verts, faces), reps)))
    fn = faces.cpu().numpy()
    host = []
    for _ in range(3):
        t = time.perf_counter()
        r_added, r_info = fr.fill_holes(fn, V)
        host.append((time.perf_counter() - t) * 1e3)
    print(line("host restatement (3 calls)", host))
    same = np.array_equal(out[F:].cpu().numpy(), r_added) and info == r_info
    print(f"  equal to the host restatement: {same}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-room", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name())
    f, n = fr.torus(512, 256)
    gone = np.zeros(len(f), bool)
    gone[2 * np.arange(0, len(f) // 2, 53)] = True
    verts = torch.rand(n, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    ok = report("torus 512 x 256", verts, torch.from_numpy(f[~gone]).to(dev), a.reps)
    if not a.no_room:
        from dns_slam_amd.decoder import Decoder
        from dns_slam_amd.mapping import Mapper
        from dns_slam_amd.meshing import Mesher
        from util import randomise_
        cam = synthetic.camera(H=120, W=160, fx=120.0, fy=120.0)
        bound, cam, frames = synthetic.make_scene(a.kf, cam=cam, seed=1)
        cfg = synthetic.default_cfg()
        dec = Decoder(cfg["model"], bound, n_class=8).to(dev)
        mapper = Mapper(cfg, dec, bound, cam, device=dev)
        mapper.set_decoder(frames)
        randomise_(dec, 1)
        randomise_([mapper.fine_decoders.pool], 2)
        cfg["meshing"] = {"resolution": a.res, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True}
        kfs = [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i]}
               for i in range(a.kf)]
        v, fc, _, _ = Mesher(cfg, mapper).extract(kfs)
        ok = report(f"room, extract at {a.res}^3 with {a.kf} keyframes", v, fc, a.reps) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
