"""One 1280 x 720 frame of the headless visualiser on the 256^3 mesh tools/time_mesh.py builds (the synthetic room, cleaned): ms
for ops.render_mesh_launch with shade="headlight", without points and with the points of a session (two camera actors and two
trajectories, as dns_slam_amd/visualize.py builds them), under either culling mode (the synthetic map's decoder is random: which
side of its surfaces faces the viewer is arbitrary), and for ops.rasterize_depth_launch on the same mesh and view; median
and range over --reps repetitions, each timed on its own between device synchronisations, after a warm-up of each.

    python tools/time_render_mesh.py [--res 256] [--kf 50] [--ply FILE.ply] [--H 720 --W 1280] [--reps 20] [--traj 2000]
    (--ply: time that mesh instead)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dns_slam_amd import evaluation as E, ops                  # noqa: E402
from dns_slam_amd.visualize import Frontend                    # noqa: E402
from time_raster import synthetic_mesh                         # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms, out


def show(name, ms, note=""):
    print(f"  {name:34s} median {statistics.median(ms):8.3f} ms   range {min(ms):8.3f} .. {max(ms):8.3f} ms{note}")
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--kf", type=int, default=50)
    ap.add_argument("--ply")
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--traj", type=int, default=2000)
    a = ap.parse_args()
    dev = "cuda:0"
    if a.ply:
        m = E.read_ply(a.ply)
        v, f = torch.from_numpy(m["verts"]).to(dev), torch.from_numpy(m["faces"]).to(dev)
    else:
        v, f = synthetic_mesh(a.res, a.kf, dev)
    f = f.to(torch.int32).contiguous()
    col = torch.rand(v.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    rng = np.random.default_rng(0)
    if a.ply:
        extents, transform = E.view_box(v)
        gl = np.array(E.sample_views(extents, transform, 1, seed=0)[0], np.float64)      # an OpenCV pose inside the mesh's box ...
        gl[:3, 1] *= -1
        gl[:3, 2] *= -1                                           # ... in the stored form the frontend takes (y up, looking along -z)
        keys = gl[None]
    else:
        # the keyframes the mesh was extracted from: the mesher keeps what they saw, so the first of them sees the mesh
        from dns_slam_amd import synthetic
        keys = synthetic.make_scene(a.kf, cam=synthetic.camera(H=120, W=160, fx=120.0, fy=120.0), seed=1)[2]["est_c2w"].double().numpy()
        gl = keys[0].copy()
    poses = keys[np.arange(a.traj) % len(keys)].copy()
    poses[:, :3, 3] += -gl[:3, 2][None] * np.linspace(0.3, 1.5, a.traj)[:, None] + rng.normal(size=(a.traj, 3)) * 0.05
    fe = Frontend("unused", gl, cam_scale=0.1, estimate_c2w_list=poses, gt_c2w_list=poses[::-1].copy(), H=a.H, W=a.W)
    fe.update_pose(1, poses[-1], gt=False)
    fe.update_pose(1, poses[0], gt=True)
    fe.update_cam_trajectory(a.traj, gt=False)
    fe.update_cam_trajectory(a.traj, gt=True)
    p, pc = fe.scene_points()
    p, pc = torch.from_numpy(p).to(dev), torch.from_numpy(pc).to(dev)
    cam = (a.H, a.W, *fe.intrinsics)
    kw = dict(z_near=fe.z_near, z_far=1000.0)
    lit = dict(kw, shade="headlight")
    t_lit, out = timed(lambda: ops.render_mesh_launch(v, f, col, fe.w2c, *cam, **lit), a.reps)
    t_pts, out_p = timed(lambda: ops.render_mesh_launch(v, f, col, fe.w2c, *cam, points=p, point_colors=pc, point_size=4, **lit), a.reps)
    t_front, out_f = timed(lambda: ops.render_mesh_launch(v, f, col, fe.w2c, *cam, cull="front", **lit), a.reps)
    t_back, out_b = timed(lambda: ops.render_mesh_launch(v, f, col, fe.w2c, *cam, cull="back", **lit), a.reps)
    t_none, out_n = timed(lambda: ops.render_mesh_launch(v, f, col, fe.w2c, *cam, **kw), a.reps)
    t_depth, (d, _) = timed(lambda: ops.rasterize_depth_launch(v, f, fe.w2c, *cam, fe.z_near, 1000.0), a.reps)
    same = bool(torch.equal(out_n["depth"].view(torch.int32), d.view(torch.int32)))
    st = ops.render_mesh_launch(v, f, col, fe.w2c, *cam, stats=True, **lit)["status"].cpu().tolist()
    share = lambda o: float((o["index"] >= 0).float().mean())
    print(f"mesh: {v.shape[0]} vertices, {f.shape[0]} faces; one view of {a.H} x {a.W}; {p.shape[0]} points; {torch.cuda.get_device_name()}")
    print(f"  pixels covered by the mesh {share(out):.4f} (front-culled {share(out_f):.4f}, back-culled {share(out_b):.4f}), by points "
          f"{float((out_p['index'] <= -2).float().mean()):.4f}; {st[2]} pairs by their set-up thread, {st[1]} through the list")
    m_lit = show("render_mesh, shaded", t_lit)
    m_pts = show("  the same with the points", t_pts)
    show("  the same, cull='front'", t_front)
    show("  the same, cull='back'", t_back)
    m_none = show("render_mesh, unshaded", t_none, f"   (depth == rasterize_depth: {same})")
    m_depth = show("rasterize_depth", t_depth)
    print(f"  render_mesh / rasterize_depth: {m_lit / m_depth:.2f} (shaded), {m_pts / m_depth:.2f} (shaded, with points), "
          f"{m_none / m_depth:.2f} (unshaded)")
    if not same:
        sys.exit("the depth images differ")
    if share(out) == 0.0:
        sys.exit("the view sees no face of the mesh: these times measure the set-up alone")


if __name__ == "__main__":
    main()
