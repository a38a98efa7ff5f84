"""GPU: the keyframe codes of the mesh vertex query (csrc/mesh_feature.hip, ops.keyframe_pairs / ops.keyframe_codes) and the
``stem=`` keyword of dns_slam_amd.meshing.Mesher, against the torch restatement of the reference's get_2d_feature
(tests/kf_codes_ref.py) and the CPU oracle.  The scene, the mapper and the keyframes are those of tests/test_gpu_mesh.py."""
import functools

import numpy as np
import pytest
import torch

import kf_codes_ref
import mc_ref
import test_gpu_mesh as tm
from oracle import feature_ref as fr
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_MAIN = 20000
# seed of the 20 000 points: with it the restatement alone, on the CPU, flags 1.0 % of the points `near` (cap: 5 %) and gives
# 27 % of them a pair (floor: 20 %)
SEED = 5


def _bundle(kfs):
    c2w = torch.stack([k["est_c2w"] for k in kfs]).to(DEV)
    return (torch.inverse(c2w).float(), c2w[:, :3, 3].float().contiguous(), torch.stack([k["gt_depth"] for k in kfs]).to(DEV).float())


@functools.lru_cache(maxsize=None)
def _main():
    """The 6-keyframe scene, ResNet(seed=0) as the stem, 20 000 points (half uniform in the bound padded by 5 %, half near the
    surfaces the keyframes see, kf_codes_ref.mixed_points) and the restatement's results for them, computed once."""
    from dns_slam_amd.encoder import ResNet
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = tm._mapper()
    kfs = tm._keyframes(frames)
    enc = ResNet(seed=0).to(DEV)
    pts = kf_codes_ref.mixed_points(P_MAIN, kfs, cam, bound, torch.Generator().manual_seed(SEED)).to(DEV)
    merge = mapper.decoder.merge
    with torch.no_grad():
        ref = kf_codes_ref.get_2d_feature(pts, kfs, cam, enc, merge, 32)
    w2c, org, dep = _bundle(kfs)
    stem = Mesher(cfg, mapper).keyframe_stem(kfs, enc)
    return dict(cfg=cfg, bound=bound, cam=cam, frames=frames, mapper=mapper, kfs=kfs, enc=enc, pts=pts, merge=merge, ref=ref,
                w2c=w2c, org=org, dep=dep, stem=stem)


def _codes(m, pts, sl=slice(None), **kw):
    from dns_slam_amd import ops
    return ops.keyframe_codes(pts, m["w2c"][sl], m["org"][sl], m["dep"][sl], m["stem"][sl], m["cam"], m["merge"], **kw)


def _check_pairs(pt, kf, iu, iv, count, mask, near, cam):
    K, P = mask.shape
    got = torch.zeros_like(mask)
    got[kf, pt] = True
    diff = (got != mask).any(0)
    print(f"pairs: {pt.numel()} listed, {int(mask.sum())} in the restatement, {int(diff.sum())} points differ, "
          f"{int((diff & ~near).sum())} of them not near, near {float(near.float().mean()):.4f}")
    assert int((diff & ~near).sum()) == 0
    assert int(diff.sum()) <= 1e-3 * P
    key = pt * K + kf
    assert bool((key[1:] > key[:-1]).all())                                   # point-major, keyframes ascending
    assert torch.equal(torch.bincount(pt, minlength=P), count.long())
    assert count.dtype == torch.int32 and pt.dtype == torch.int64 and kf.dtype == torch.int64
    if pt.numel():
        assert 0 <= int(iu.min()) and int(iu.max()) < cam["W"] and 0 <= int(iv.min()) and int(iv.max()) < cam["H"]


def test_stem_maps_layout():
    m = _main()
    f = m["enc"](m["frames"]["gt_color"].to(DEV)[None])[0]                    # [K, 64, h, w]
    assert m["stem"].shape == (6, 30, 40, 64) and m["stem"].dtype == torch.float32 and m["stem"].is_contiguous()
    # batches of 4 + 2 keyframes against one of 6: the convolution may pick another summation order per batch size, and two
    # orders of a 147-term fp32 sum differ by at most 147 * 2^-24 = 8.8e-6 of the sum of the terms' magnitudes
    assert rel_err(m["stem"], f.permute(0, 2, 3, 1)) <= 1e-5


def test_pairs_match_restatement():
    from dns_slam_amd import ops
    m = _main()
    _, _, rcount, mask, near = m["ref"]
    pt, kf, iu, iv, count = ops.keyframe_pairs(m["pts"], m["w2c"], m["dep"], m["cam"])
    _check_pairs(pt, kf, iu, iv, count, mask, near, m["cam"])
    assert float(near.float().mean()) <= 0.05
    assert float((count > 0).float().mean()) > 0.2
    ok = ~near
    assert torch.equal(count[ok].float(), rcount[ok])


def test_codes_match_restatement_and_oracle():
    m = _main()
    rcode, _, rcount, _, near = m["ref"]
    code, count = _codes(m, m["pts"])
    assert code.shape == (P_MAIN, 32) and code.dtype == torch.float32 and count.dtype == torch.int32
    assert bool(torch.isfinite(code).all())
    assert bool((code[count == 0] == 0).all())
    ok = ~near
    e = rel_err(code[ok], rcode[ok])
    print(f"codes against the restatement: rel_err {e:.3e} over {int(ok.sum())} points")
    assert e <= 1e-5
    # the CPU oracle: its stem, F.interpolate, its Merge, through the same restatement, on 2 000 of the points
    n = 2000
    enc = m["enc"].conv_blocks
    sd = [t.detach().cpu() for t in (enc.conv1.weight, enc.bn1.weight, enc.bn1.bias, enc.bn1.running_mean, enc.bn1.running_var)]
    params = m["merge"].decoder.params.detach().cpu()
    bound = m["bound"]
    kfs_cpu = [{k: v.cpu() for k, v in kf.items()} for kf in m["kfs"]]
    with torch.no_grad():
        ocode, _, ocount, _, onear = kf_codes_ref.get_2d_feature(
            m["pts"][:n].cpu(), kfs_cpu, m["cam"], lambda img: fr.stem_forward(img, *sd, eps=enc.bn1.eps),
            lambda p, o, ft: fr.merge_forward(params, bound, p, o, ft), 32)
    ok = ~(near[:n].cpu() | onear)
    assert int(ok.sum()) > 0.9 * n and int((ocount[ok] > 0).sum()) > 0.2 * n
    assert_close(code[:n].cpu()[ok], ocode[ok], what="keyframe codes against the oracle")


@pytest.mark.parametrize("case", ["P1", "P257", "K1"])
def test_edges_small(case):
    from dns_slam_amd import ops
    m = _main()
    rcode, _, rcount, mask, near = m["ref"]
    if case == "K1":
        sl, pts = slice(0, 1), m["pts"][:5000]
        with torch.no_grad():
            rc, _, rn, rmask, rnear = kf_codes_ref.get_2d_feature(pts, m["kfs"][:1], m["cam"], m["enc"], m["merge"], 32)
    else:
        sl = slice(None)
        if case == "P1":
            i = int(torch.nonzero((rcount > 0) & ~near)[0])
            idx = slice(i, i + 1)
        else:
            idx = slice(1000, 1257)
        pts, rc, rn, rmask, rnear = m["pts"][idx], rcode[idx], rcount[idx], mask[:, idx], near[idx]
    pt, kf, iu, iv, count = ops.keyframe_pairs(pts, m["w2c"][sl], m["dep"][sl], m["cam"])
    _check_pairs(pt, kf, iu, iv, count, rmask, rnear, m["cam"])
    code, count2 = _codes(m, pts, sl)
    assert torch.equal(count, count2)
    ok = ~rnear
    assert int((rn[ok] > 0).sum()) > 0
    assert rel_err(code[ok], rc[ok]) <= 1e-5
    assert bool((code[count2 == 0] == 0).all())


def test_edges_empty():
    from dns_slam_amd import ops
    m = _main()
    pts = m["pts"][:300]
    # no keyframes: zeros, no launch
    code, count = _codes(m, pts, slice(0, 0))
    assert code.shape == (300, 32) and not code.any() and count.shape == (300,) and not count.any()
    assert ops.keyframe_pairs(pts, m["w2c"][:0], m["dep"][:0], m["cam"])[0].numel() == 0
    # no points
    code, count = _codes(m, pts[:0])
    assert code.shape == (0, 32) and count.shape == (0,)
    # an all-zero depth image: no pairs
    pt, _, _, _, count = ops.keyframe_pairs(pts, m["w2c"], torch.zeros_like(m["dep"]), m["cam"])
    assert pt.numel() == 0 and not count.any()
    code, count = ops.keyframe_codes(pts, m["w2c"], m["org"], torch.zeros_like(m["dep"]), m["stem"], m["cam"], m["merge"])
    assert not code.any() and not count.any()
    # a point no keyframe sees, next to one that has a pair
    _, _, rcount, _, near = m["ref"]
    i = int(torch.nonzero((rcount > 0) & ~near)[0])
    two = torch.stack((torch.full((3,), 1e3, device=DEV), m["pts"][i]))
    code, count = _codes(m, two)
    assert count.tolist() == [0, int(rcount[i])] and not code[0].any() and bool(code[1].any())


def test_many_keyframes_cross_the_lds_tile():
    """300 keyframes of 12 x 16 images (the recipe of test_keyframe_project_many_keyframes): two LDS tiles of 256; the
    keyframes of a point stay ascending across the tiles, and the codes are means over many views."""
    from dns_slam_amd import ops, synthetic
    from dns_slam_amd.meshing import Mesher
    m = _main()
    cam = synthetic.camera(H=12, W=16, fx=12.0, fy=12.0)
    bound, cam, frames = synthetic.make_scene(3, cam=cam, seed=3)
    n = 300
    idx = torch.arange(n) % 3
    c2w = frames["est_c2w"][idx].clone()
    c2w[:, :3, 3] += torch.randn(n, 3, generator=torch.Generator().manual_seed(1)) * 0.05
    color = (frames["gt_color"][idx] + (torch.arange(n) % 7)[:, None, None, None].float() * 0.05).clamp(0, 1)
    kfs = [{"est_c2w": c2w[i], "gt_label": frames["gt_label"][idx[i]], "gt_depth": frames["gt_depth"][idx[i]],
            "gt_color": color[i]} for i in range(n)]
    pts = kf_codes_ref.mixed_points(3000, kfs, cam, bound, torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        rcode, _, rcount, mask, near = kf_codes_ref.get_2d_feature(pts, kfs, cam, m["enc"], m["merge"], 32)
    w2c, org, dep = _bundle(kfs)
    pt, kf, iu, iv, count = ops.keyframe_pairs(pts, w2c, dep, cam)
    _check_pairs(pt, kf, iu, iv, count, mask, near, cam)
    has_hi, has_lo = torch.zeros(3000, dtype=torch.bool, device=DEV), torch.zeros(3000, dtype=torch.bool, device=DEV)
    has_hi[pt[kf >= 256]] = True
    has_lo[pt[kf < 256]] = True
    assert int((has_hi & has_lo).sum()) > 100                                 # segments that span both tiles
    stem = Mesher(m["cfg"], m["mapper"]).keyframe_stem(kfs, m["enc"])
    code, count2 = ops.keyframe_codes(pts, w2c, org, dep, stem, cam, m["merge"])
    assert torch.equal(count, count2) and int(count.max()) > 20
    ok = ~near
    e = rel_err(code[ok], rcode[ok])
    print(f"300 keyframes: rel_err {e:.3e}, near {float(near.float().mean()):.4f}, max count {int(count.max())}")
    assert e <= 1e-5
    code4, count4 = ops.keyframe_codes(pts, w2c, org, dep, stem, cam, m["merge"], max_pairs=300 * 700)
    assert torch.equal(code4, code) and torch.equal(count4, count2)


def test_chunking_and_repeat_are_bit_identical():
    m = _main()
    code, count = _codes(m, m["pts"])
    code_b, count_b = _codes(m, m["pts"])
    assert torch.equal(code, code_b) and torch.equal(count, count_b)
    code_c, count_c = _codes(m, m["pts"], max_pairs=6 * 4000)                 # 5 chunks of 4 000 points
    assert torch.equal(code, code_c) and torch.equal(count, count_c)
    code_d, _ = _codes(m, m["pts"], max_pairs=6 * 1111)                       # 19 chunks, the last one short
    assert torch.equal(code, code_d)


def test_refusals():
    from dns_slam_amd import _lib, ops
    m = _main()
    pts = m["pts"][:100]
    a = (m["w2c"], m["org"], m["dep"], m["stem"])
    bad = [(a[0], a[1], a[2], m["stem"][..., :6].contiguous()),               # C = 6
           (a[0], a[1], a[2], m["stem"][..., :32].contiguous()),              # 48 + 32 != 112
           (a[0][:5], a[1], a[2], a[3]), (a[0], a[1][:5], a[2], a[3]), (a[0], a[1], a[2][:5], a[3]), (a[0], a[1], a[2], a[3][:5]),
           (a[0], a[1], a[2], a[3].double()), (a[0], a[1], a[2], a[3].cpu()), (a[0].cpu(), a[1], a[2], a[3])]
    for w2c, org, dep, stem in bad:
        with pytest.raises(ValueError):
            ops.keyframe_codes(pts, w2c, org, dep, stem, m["cam"], m["merge"])
    with pytest.raises(ValueError):
        ops.keyframe_codes(pts[:, :2], *a, m["cam"], m["merge"])
    with pytest.raises(ValueError):
        ops.keyframe_pairs(pts, m["w2c"][:5], m["dep"], m["cam"])
    # the entry point itself answers a channel count that is no multiple of 4 with an error code
    rec = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, 112, device=DEV)
    rc = _lib.lib.dns_kf_pair_rows(_lib.ptr(rec), 1, _lib.ptr(pts), 100, _lib.ptr(m["org"]), 6, _lib.ptr(m["stem"]), 6, 30, 40, 60, 80,
                                   _lib.ptr(out), _lib.ptr(out), 112, None)
    assert rc == -1 and b"dns_kf_pair_rows" in _lib.lib.dns_last_error()


def test_mesher_with_stem(tmp_path):
    from dns_slam_amd import ops
    from dns_slam_amd.encoder import ResNet
    from dns_slam_amd.meshing import Mesher, compact_mesh
    cfg, bound, cam, frames, mapper = tm._mapper()
    kfs = tm._keyframes(frames)
    mesher = Mesher(cfg, mapper)
    B = 16384
    plain = {cm: mesher.extract(kfs, clean_mesh=cm) for cm in (False, True)}  # encoder None: the geometry to keep
    mapper.encoder = ResNet(seed=0).to(DEV)
    with pytest.raises(NotImplementedError, match="stem="):
        mesher.extract(kfs)
    with_stem = {cm: mesher.extract(kfs, clean_mesh=cm, stem=True) for cm in (False, True)}
    for cm in (False, True):
        assert torch.equal(with_stem[cm][0], plain[cm][0]) and torch.equal(with_stem[cm][1], plain[cm][1])
    assert plain[True][1].shape[0] > 100
    # the step-by-step vertex query: keyframe labels, the restatement's codes, eval_points per points_batch_size chunk
    w2c = torch.inverse(torch.stack([k["est_c2w"] for k in kfs]).to(DEV)).float()
    labs = torch.stack([k["gt_label"] for k in kfs]).to(DEV)
    md = torch.stack([k["gt_depth"].max() for k in kfs]).to(DEV)
    for cm in (False, True):
        v, _, c, l = with_stem[cm]
        with torch.no_grad():
            codes, _, _, _, near = kf_codes_ref.get_2d_feature(v, kfs, cam, mapper.encoder, mapper.decoder.merge, 32)
        vals, vlab = [], []
        for s in range(0, v.shape[0], B):
            lab, _ = ops.keyframe_project(v[s:s + B], w2c, labs, md, cam)
            a, b_ = mapper.eval_points(v[s:s + B], codes[s:s + B], lab)
            vals.append(a), vlab.append(b_)
        vals, vlab = torch.cat(vals), torch.cat(vlab)
        ref_col = (vals[:, :3].clamp(0, 1) * 255).to(torch.uint8)
        d = (c.int() - ref_col.int()).abs().max(1).values
        print(f"clean_mesh={cm}: {v.shape[0]} vertices, colour differences > 1 level: {int((d > 1).sum())} "
              f"({int(((d > 1) & ~near).sum())} not near), labels agree {float((l == vlab).float().mean()):.5f}, "
              f"colours differ from the stem-less ones on {float((c != plain[cm][2]).any(1).float().mean()):.3f}")
        assert int(d.max()) <= 1
        assert float((l == vlab).float().mean()) >= 0.999
        assert float((c != plain[cm][2]).any(1).float().mean()) > 0.10
    # the maps given: the same bits
    maps = mesher.keyframe_stem(kfs)
    again = mesher.extract(kfs, clean_mesh=True, stem=maps)
    assert all(torch.equal(x, y) for x, y in zip(again, with_stem[True]))
    mapper.encoder = None                                                     # maps are used as given without an encoder
    again = mesher.extract(kfs, clean_mesh=True, stem=maps)
    assert all(torch.equal(x, y) for x, y in zip(again, with_stem[True]))
    with pytest.raises(ValueError):
        mesher.extract(kfs, stem=True)
    mapper.encoder = ResNet(seed=0).to(DEV)
    # the files
    v1, f1, c1, l1 = with_stem[True]
    paths = mesher.get_mesh(str(tmp_path), kfs, 3, stem=True)
    pv, pf = mc_ref.read_ply(paths[0])
    assert (np.stack((pv["x"], pv["y"], pv["z"]), 1) == v1.cpu().numpy()).all() and (pf == f1.cpu().numpy()).all()
    assert (np.stack((pv["red"], pv["green"], pv["blue"]), 1) == c1.cpu().numpy()).all()
    assert (pv["label"] == l1.cpu().numpy()).all()
    with pytest.raises(NotImplementedError):
        mesher.get_mesh(str(tmp_path), kfs, 3)
    parts = mesher.get_part_meshes(str(tmp_path), kfs, 3, stem=True)
    classes = torch.unique(l1).tolist()
    assert len(parts) == len(classes) > 0
    for path, e in zip(parts, classes):
        assert path.endswith(f"mesh_3_part_{int(e)}.ply")
        _, _, used = compact_mesh(v1, f1, (l1 == e)[f1.long()].any(1))
        qv, _ = mc_ref.read_ply(path)
        assert (np.stack((qv["red"], qv["green"], qv["blue"]), 1) == c1[used].cpu().numpy()).all()
