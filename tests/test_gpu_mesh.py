"""GPU: mesh extraction (csrc/mesh.hip, Mapper.eval_occupancy, dns_slam_amd.meshing) against the numpy marching cubes of
tests/mc_ref.py and torch restatements of the reference's keyframe loops (slams/meshing.py:203-274, 313-373, 562-784)."""
import copy

import numpy as np
import pytest
import torch

import mc_ref
from util import randomise_, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _assert_same_mesh(gv, gf, rv, rf):
    gv, gf = gv.cpu().numpy(), gf.cpu().numpy()
    assert gf.dtype == np.int32 and gf.shape == rf.shape and (gf == rf).all()
    assert gv.shape == rv.shape
    if len(rv):
        ulp = np.spacing(np.float32(np.abs(rv).max()))
        assert np.abs(gv.astype(np.float64) - rv).max() <= ulp


def _gpu_mc(vol, o, sp, level=0.0):
    from dns_slam_amd import ops
    return ops.marching_cubes(torch.as_tensor(vol).to(DEV), level, o, sp)


def _fields():
    out = {}
    for name, make in (("sphere", mc_ref.sphere_field), ("torus", mc_ref.torus_field), ("random", mc_ref.random_field)):
        vol, o, sp, _ = make()
        out[name] = (vol, o, sp)
    vol, o, sp, _ = mc_ref.sphere_field(40)
    slab = vol.copy()
    slab[:, 25:, :] = -100                                    # an out-of-bound slab cuts the sphere open
    out["slab"] = (slab, o, sp)
    out["at_level"] = (np.round(vol * 8) / 8, o, sp)          # many corners exactly at the level
    out["empty"] = (np.full((17, 9, 12), -1.0, np.float32), o, sp)
    out["thin"] = (vol[:, :, 20:21].copy(), o, sp)             # one z plane: no cubes, edges only
    return out


@pytest.mark.parametrize("name", ["sphere", "torus", "random", "slab", "at_level", "empty", "thin"])
def test_marching_cubes_equals_numpy(name):
    vol, o, sp = _fields()[name]
    vol = vol.astype(np.float32)
    rv, rf = mc_ref.marching_cubes(vol, 0.0, o, sp)
    gv, gf = _gpu_mc(vol, o, sp)
    _assert_same_mesh(gv, gf, rv, rf)
    if name == "empty":
        assert gv.shape == (0, 3) and gf.shape == (0, 3)


def test_marching_cubes_multiblock_256():
    """256^3 random smooth field: > 2^20 vertices, 65536 count blocks through the one-workgroup scan."""
    rng = np.random.default_rng(7)
    ax = np.linspace(-1, 1, 256, dtype=np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = np.zeros_like(X)
    for _ in range(4):
        k = rng.normal(size=3) * 20
        vol += np.sin(k[0] * X + k[1] * Y + k[2] * Z + rng.uniform(0, 6)).astype(np.float32)
    del X, Y, Z
    sp = [float(ax[1] - ax[0])] * 3
    gv, gf = _gpu_mc(vol, (-1.0, -1.0, -1.0), sp, level=0.1)
    rv, rf = mc_ref.marching_cubes(vol, 0.1, (-1.0, -1.0, -1.0), sp)
    assert len(rv) > (1 << 20)
    _assert_same_mesh(gv, gf, rv, rf)


def test_marching_cubes_scan_runs_of_two():
    """65 x 64 x 64 points are 1040 count blocks, the smallest grid of this kind at which every thread of the one-workgroup carry
    scan covers a run of two blocks."""
    axes = [np.linspace(-1, 1, n) for n in (65, 64, 64)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    vol = (0.6 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    assert (vol.size + 255) // 256 == 1040
    o, sp = (-1.0, -1.0, -1.0), [float(a[1] - a[0]) for a in axes]
    rv, rf = mc_ref.marching_cubes(vol, 0.0, o, sp)
    assert rv.shape == (6832, 3) and rf.shape == (13660, 3)
    gv, gf = _gpu_mc(vol, o, sp)
    _assert_same_mesh(gv, gf, rv, rf)


def test_marching_cubes_sphere_area():
    n = 128
    ax = np.linspace(-0.5, 0.5, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.3 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    gv, gf = _gpu_mc(vol, (-0.5,) * 3, [ax[1] - ax[0]] * 3)
    a = mc_ref.area(gv.cpu().numpy(), gf.cpu().numpy())
    assert abs(a - 4 * np.pi * 0.09) <= 0.01 * 4 * np.pi * 0.09
    assert mc_ref.check_manifold(gf.cpu().numpy()) == (True, True)


def test_marching_cubes_refusals():
    from dns_slam_amd import ops
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros(4, 4, 4, device=DEV), 0.0, (0, 0, 0), (1.0, float("nan"), 1.0))
    from dns_slam_amd import _lib
    assert int(_lib.lib.dns_mc_ws_bytes(2048, 2048, 1024)) == 0          # 2^32 points: >= 2^31 edges
    assert _lib.lib.dns_mc_count(None, 2048, 2048, 1024, 0.0, None, None, None) == -1


# ---- keyframe projection -------------------------------------------------------------------------------------------------
def _scene(n_frames=6):
    from dns_slam_amd import synthetic
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(n_frames, cam=cam, seed=3)
    return bound, cam, frames


def _keyframes(frames):
    return [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i],
             "gt_color": frames["gt_color"][i]} for i in range(frames["est_c2w"].shape[0])]


def _ref_project(points, keyframe_dict, cam, H, W):
    """The reference's loops (meshing.py:203-274 without the depth test, 313-373's label), in torch on the device, plus a flag
    of the points within 1e-3 px of a rounding / image-edge boundary (or at the depth limit) of some keyframe."""
    K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]], device=DEV)
    label_pts = torch.zeros(points.shape[0], device=DEV)
    seen_mask = torch.zeros(points.shape[0], dtype=torch.bool, device=DEV)
    near = torch.zeros(points.shape[0], dtype=torch.bool, device=DEV)
    for kf in keyframe_dict:
        c2w = kf["est_c2w"].to(DEV)
        w2c = torch.inverse(c2w).float()
        homo = torch.cat([points, torch.ones_like(points[:, :1])], 1).reshape(-1, 4, 1)
        cam_cord = (w2c @ homo)[:, :3]
        cam_cord[:, 0] *= -1
        uv = K.float() @ cam_cord.float()
        z = uv[:, -1:] + 1e-8
        uv = (uv[:, :2] / z).float()
        m = (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
        m = (m & (z[:, :, 0] < 0)).reshape(-1)
        u, v = uv[:, 0, 0], uv[:, 1, 0]
        md = torch.max(kf["gt_depth"].to(DEV)) * 1.2
        dz = -cam_cord[:, 2, 0]
        near |= (z[:, 0, 0] < 0) & ((((u - u.floor() - 0.5).abs() < 1e-3) | ((v - v.floor() - 0.5).abs() < 1e-3)) |
                                    (u.abs() < 1e-3) | ((u - W).abs() < 1e-3) | (v.abs() < 1e-3) | ((v - H).abs() < 1e-3) |
                                    ((dz - md).abs() < 1e-5 * md))
        uv_ = torch.round(uv[m, :, 0]).to(torch.int64)
        uv_[:, 0] = uv_[:, 0].clamp(0, W - 1)
        uv_[:, 1] = uv_[:, 1].clamp(0, H - 1)
        label_pts[m] = kf["gt_label"].to(DEV)[uv_[:, 1], uv_[:, 0]].float()
        s = m.clone()
        s[m.clone()] &= dz[m] < md
        seen_mask |= s
    return label_pts, seen_mask, near


def test_keyframe_project_matches_reference_loops():
    from dns_slam_amd import ops
    bound, cam, frames = _scene(6)
    g = torch.Generator().manual_seed(5)
    b = bound.float()
    P = 300000
    pts = ((torch.rand(P, 3, generator=g) * 1.2 - 0.1) * (b[:, 1] - b[:, 0]) + b[:, 0]).to(DEV)
    kfs = _keyframes(frames)
    H, W = cam["H"], cam["W"]
    rl, rs, near = _ref_project(pts, kfs, cam, H, W)
    w2c = torch.inverse(frames["est_c2w"].to(DEV)).float()
    md = frames["gt_depth"].to(DEV).reshape(6, -1).max(1).values
    gl, gs = ops.keyframe_project(pts, w2c, frames["gt_label"].to(DEV), md, cam)
    bad = (gl != rl) | (gs != rs)
    assert bool((~near[bad]).sum() == 0), int((~near[bad]).sum())
    assert int(bad.sum()) <= 1e-3 * P
    assert 0.05 < float(rs.float().mean()) < 0.95               # the scene sees some of the points, not all
    # no keyframes: label 0, nothing seen
    gl0, gs0 = ops.keyframe_project(pts[:1000], w2c[:0], frames["gt_label"][:0].to(DEV), md[:0], cam)
    assert (gl0 == 0).all() and not gs0.any()


def test_keyframe_project_many_keyframes():
    """More keyframes than one LDS tile (256): the tiles run from the last to the first."""
    from dns_slam_amd import ops
    bound, cam, frames = _scene(3)
    n = 600
    idx = torch.arange(n) % 3
    c2w = frames["est_c2w"][idx].clone()
    c2w[:, :3, 3] += torch.randn(n, 3, generator=torch.Generator().manual_seed(1)) * 0.05
    labels = frames["gt_label"][idx] + (torch.arange(n) % 5)[:, None, None].float() * 10
    depth = frames["gt_depth"][idx]
    kfs = [{"est_c2w": c2w[i], "gt_label": labels[i], "gt_depth": depth[i]} for i in range(n)]
    g = torch.Generator().manual_seed(2)
    b = bound.float()
    pts = ((torch.rand(20000, 3, generator=g)) * (b[:, 1] - b[:, 0]) + b[:, 0]).to(DEV)
    rl, rs, near = _ref_project(pts, kfs, cam, cam["H"], cam["W"])
    gl, gs = ops.keyframe_project(pts, torch.inverse(c2w.to(DEV)).float(), labels.to(DEV),
                                  depth.to(DEV).reshape(n, -1).max(1).values, cam)
    bad = (gl != rl) | (gs != rs)
    assert bool((~near[bad]).sum() == 0) and int(bad.sum()) <= 1e-3 * pts.shape[0]


# ---- occupancy query and the whole extraction ----------------------------------------------------------------------------
def _mapper(seed=1):
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.mapping import Mapper
    bound, cam, frames = _scene(6)
    cfg = synthetic.default_cfg(n_pixels=240, n_samples_ray=32, n_surface_ray=15, hash_size=14, voxel_size=0.08, smooth_pts=10)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    mapper = Mapper(cfg, dec, bound, cam, device=DEV)
    mapper.set_decoder(frames)
    randomise_(dec, seed)
    with torch.no_grad():
        dec.pe_fn.grid_fn.params.mul_(2000.0)
    randomise_([mapper.fine_decoders.pool], seed + 1)
    cfg = copy.deepcopy(cfg)
    cfg["meshing"] = {"resolution": 40, "level_set": 0.0, "points_batch_size": 16384, "clean_mesh": True}
    return cfg, bound, cam, frames, mapper


def test_eval_occupancy_equals_eval_points():
    cfg, bound, cam, frames, mapper = _mapper()
    g = torch.Generator().manual_seed(4)
    b = bound.float()
    P, B = 50000, 16384
    pts = ((torch.rand(P, 3, generator=g) * 1.1 - 0.05) * (b[:, 1] - b[:, 0]) + b[:, 0]).to(DEV)
    classes = sorted(mapper.fine_decoders.keys())
    lab = torch.tensor(classes)[torch.randint(0, len(classes), (P,), generator=g)]
    single = classes[-1]
    chunk1 = lab[B:2 * B]
    chunk1[chunk1 == single] = classes[0]
    chunk1[100] = single                                       # a class with ONE point in the second chunk
    pts[B + 100] = ((b[:, 0] + b[:, 1]) / 2).to(DEV)           # inside the bound
    lab = lab.to(DEV)
    for stage in ("fine", "coarse"):
        la = lab if stage == "fine" else None
        occ = mapper.eval_occupancy(pts, la, stage=stage)
        ref = mapper.eval_points(pts, None, la, stage=stage)[0][:, 3]
        assert rel_err(occ, ref) <= 1e-5
        occ_c = mapper.eval_occupancy(pts, la, stage=stage, rule_chunk=B, n_pts_batch=1 << 15)
        ref_c = torch.cat([mapper.eval_points(pts[s:s + B], None, None if la is None else la[s:s + B], stage=stage)[0][:, 3]
                           for s in range(0, P, B)])
        assert rel_err(occ_c, ref_c) <= 1e-5
        if stage == "fine":
            assert ref_c[B + 100] == 0.0 or not (mapper.bound_dev[:, 0] < pts[B + 100].double()).all()  # zeros: no network
            assert bool((occ_c != occ).any())                  # the per-chunk rule differs from the per-call one
            ep = mapper.eval_points(pts, None, la, rule_chunk=B)
            refp = [mapper.eval_points(pts[s:s + B], None, la[s:s + B]) for s in range(0, P, B)]
            assert rel_err(ep[0], torch.cat([r[0] for r in refp])) <= 1e-5
            assert (ep[1] == torch.cat([r[1] for r in refp])).float().mean() >= 0.999


def test_extract_step_by_step(tmp_path):
    from dns_slam_amd import ops
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = _mapper()
    kfs = _keyframes(frames)
    mesher = Mesher(cfg, mapper)
    B = 16384
    # 1. the grid pass as the reference's driver runs it: numpy meshgrid points, per-chunk keyframe labels + eval_points
    grid = mesher.get_grid_uniform()
    x, y, z = grid["xyz"]
    xx, yy, zz = np.meshgrid(x, y, z)
    gp = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float).to(DEV).contiguous()
    w2c = torch.inverse(torch.stack([k["est_c2w"] for k in kfs]).to(DEV)).float()
    labs = torch.stack([k["gt_label"] for k in kfs]).to(DEV)
    md = torch.stack([k["gt_depth"].max() for k in kfs]).to(DEV)
    z_all = []
    for s in range(0, gp.shape[0], B):
        lab, _ = ops.keyframe_project(gp[s:s + B], w2c, labs, md, cam)
        z_all.append(mapper.eval_points(gp[s:s + B], None, lab)[0][:, 3])
    ref_vol = torch.cat(z_all).reshape(len(y), len(x), len(z)).permute(1, 0, 2)
    vol, _ = mesher.grid_occupancy(kfs)
    assert rel_err(vol, ref_vol) <= 1e-5
    # 2. marching cubes of that volume
    vol_np = vol.cpu().numpy()
    o, sp = (x[0], y[0], z[0]), (x[2] - x[1], y[2] - y[1], z[2] - z[1])
    rv, rf = mc_ref.marching_cubes(vol_np, 0.0, o, sp)
    assert len(rf) > 100
    v0, f0, c0, l0 = mesher.extract(kfs, clean_mesh=False)
    _assert_same_mesh(v0, f0, rv, rf)
    # 3. colours and labels: eval_points at the vertices, per points_batch_size chunk
    vals, vlab = [], []
    for s in range(0, v0.shape[0], B):
        lab, _ = ops.keyframe_project(v0[s:s + B], w2c, labs, md, cam)
        a, b_ = mapper.eval_points(v0[s:s + B], None, lab)
        vals.append(a), vlab.append(b_)
    vals, vlab = torch.cat(vals), torch.cat(vlab)
    ref_col = (vals[:, :3].clamp(0, 1) * 255).to(torch.uint8)
    assert (c0.int() - ref_col.int()).abs().max() <= 1
    assert (l0 == vlab).float().mean() >= 0.999
    # 4. cleaning: the faces with a seen vertex, then the used vertices renumbered (numpy restatement)
    _, seen = ops.keyframe_project(v0, w2c, labs, md, cam)
    seen = seen.cpu().numpy()
    keep = seen[rf].any(1)
    assert 0 < keep.sum() < len(rf) or keep.all()
    fk = rf[keep]
    used = np.zeros(len(rv), bool)
    used[fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    v1, f1, c1, l1 = mesher.extract(kfs, clean_mesh=True)
    _assert_same_mesh(v1, f1, rv[used], remap[fk].astype(np.int32))
    assert (c1 == c0[torch.from_numpy(used).to(DEV)]).float().mean() >= 0.999
    # 5. the files
    pal = np.random.default_rng(0).integers(0, 256, size=(8, 3)).astype(np.uint8)
    paths = mesher.get_mesh(str(tmp_path), kfs, 7, label=True, palette=pal)
    assert [p.split("/")[-1] for p in paths] == ["mesh_7.ply", "mesh_7_semantic.ply"]
    pv, pf = mc_ref.read_ply(paths[0])
    assert (np.stack((pv["x"], pv["y"], pv["z"]), 1) == v1.cpu().numpy()).all() and (pf == f1.cpu().numpy()).all()
    assert (np.stack((pv["red"], pv["green"], pv["blue"]), 1) == c1.cpu().numpy()).all()
    assert (pv["label"] == l1.cpu().numpy()).all()
    sv, sf = mc_ref.read_ply(paths[1])
    l1n = l1.cpu().numpy()
    exp = np.zeros((len(l1n), 3), np.uint8)
    exp[l1n >= 0] = pal[l1n[l1n >= 0]]
    assert (np.stack((sv["red"], sv["green"], sv["blue"]), 1) == exp).all() and (sf == pf).all()


def test_mesher_refusals():
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = _mapper()
    kfs = _keyframes(frames)
    mesher = Mesher(cfg, mapper)
    for kw in ({"show_forecast": True}, {"element": True}, {"fill_holes": True}, {"remove_small_geometry": True}):
        with pytest.raises(NotImplementedError):
            mesher.get_mesh("/nonexistent", kfs, 0, **kw)
    for key in ("depth_test", "get_largest_components"):
        c = copy.deepcopy(cfg)
        c["meshing"][key] = True
        with pytest.raises(NotImplementedError):
            Mesher(c, mapper)
    mapper.encoder = object()
    with pytest.raises(NotImplementedError):
        mesher.extract(kfs)
