"""GPU: the mesh hole filling (csrc/mesh_holes.hip, ops.mesh_fill_holes, Mesher.fill_holes and the ``holes`` keyword) against the
host restatement of tests/fill_holes_ref.py.  Everything is integer equality: torch.equal on the added block, dict equality on
info."""
import filecmp

import numpy as np
import pytest
import torch

import fill_holes_ref as fr
import mc_ref
from test_gpu_mesh import _keyframes, _mapper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(f):
    return torch.as_tensor(np.ascontiguousarray(f, dtype=np.int32)).reshape(-1, 3).to(DEV)


def _fill(faces, n_verts, max_edges=None):
    from dns_slam_amd import ops
    ft = _t(faces)
    out, info = ops.mesh_fill_holes(ft, n_verts) if max_edges is None else ops.mesh_fill_holes(ft, n_verts, max_edges)
    assert out.dtype == torch.int32 and out.shape == (ft.shape[0] + info["faces_added"], 3) and torch.equal(out[:ft.shape[0]], ft)
    return out[ft.shape[0]:], info


def _assert_equals_ref(faces, n_verts, max_edges=None):
    added, info = _fill(faces, n_verts, max_edges)
    r_added, r_info = fr.fill_holes(faces, n_verts, 4 if max_edges is None else max_edges)
    assert torch.equal(added.cpu(), torch.from_numpy(r_added)) and info == r_info, (info, r_info)
    return added.cpu().numpy(), info


@pytest.mark.parametrize("name", sorted(fr.HAND_CASES))
def test_hand_cases(name):
    c = fr.HAND_CASES[name]
    added, info = _assert_equals_ref(c["faces"], c["n_verts"], None if c["max_edges"] == 4 else c["max_edges"])
    assert np.array_equal(added, c["added"])
    for k, v in c["info"].items():
        assert info[k] == v, (k, info)


def test_arguments():
    from dns_slam_amd import ops
    tri = _t([[0, 1, 2]])
    for bad in ([[0, 1, 3]], [[0, -1, 2]], [[0, 1, 2], [2, 1, 1 << 30]]):
        with pytest.raises(ValueError):
            ops.mesh_fill_holes(_t(bad), 3)
    for bad in (2, 33, 4.0, True):
        with pytest.raises(ValueError):
            ops.mesh_fill_holes(tri, 3, bad)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(tri.long(), 3)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(tri.reshape(-1), 3)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(tri.cpu(), 3)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(tri, -1)
    empty = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    out, info = ops.mesh_fill_holes(empty, 5)
    assert out is empty and info == fr.fill_holes(np.zeros((0, 3), np.int32), 5)[1]


@pytest.fixture(scope="module")
def torus24():
    f, n = fr.torus(24, 24, seed=5)
    holes = fr.torus_holes(f, n, seed=11)
    return f, n, holes, f[~fr.holes_mask(len(f), holes)]


def test_torus_default(torus24):
    f, n, holes, open_f = torus24
    assert len(holes["tri"]) >= 10 and len(holes["quad"]) >= 10 and len(holes["hex"]) >= 3
    assert fr.fill_holes(open_f, n)[1]["vertices_skipped"] == 0
    added, info = _assert_equals_ref(open_f, n)
    n_tri, n_quad, n_hex = (len(holes[k]) for k in ("tri", "quad", "hex"))
    assert info["loops_filled"] == n_tri + n_quad and info["boundary_edges"] == 3 * n_tri + 4 * n_quad + 6 * n_hex
    # the 3-holes get their faces back (up to rotation); the quads are closed: what is left open is the hexagons
    tri_back = np.array([a for a in added.tolist() if sorted(a) in [sorted(f[t].tolist()) for t in holes["tri"]]])
    assert np.array_equal(fr.canon(tri_back), fr.canon(f[list(holes["tri"])]))
    again, info2 = _fill(np.concatenate((open_f, added)), n)
    assert len(again) == 0 and info2["boundary_edges"] == 6 * n_hex and info2["vertices_skipped"] == 0


def test_torus_max_edges_6(torus24):
    from dns_slam_amd import ops
    f, n, holes, open_f = torus24
    added, info = _assert_equals_ref(open_f, n, 6)
    assert info["loops_filled"] == sum(len(v) for v in holes.values())
    closed = np.concatenate((open_f, added))
    assert fr.directed_edges_paired(closed)
    verts = torch.rand(n, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert ops.mesh_components(verts, _t(closed))[2] == 1
    out, info2 = ops.mesh_fill_holes(_t(closed), n)
    assert info2["watertight"] and info2["faces_added"] == 0 and out.shape[0] == len(closed)


def test_invariance(torus24):
    f, n, holes, open_f = torus24
    base, info = _fill(open_f, n, 6)
    again, info_again = _fill(open_f, n, 6)
    assert torch.equal(base, again) and info == info_again
    rng = np.random.default_rng(3)
    g = open_f[rng.permutation(len(open_f))]
    rot = rng.integers(0, 3, len(g))
    g = np.stack([g[np.arange(len(g)), (rot + k) % 3] for k in range(3)], 1)
    assert (rot != 0).any() and not np.array_equal(g, open_f)
    moved, info_moved = _fill(g, n, 6)
    assert torch.equal(base, moved) and info == info_moved


def test_large_torus():
    """512 x 256, F = 262144 less every 53rd cell's lower face: 2474 loops over 512 workgroups of vertices and a table of 2^20
    slots."""
    f, n = fr.torus(512, 256)
    gone = np.zeros(len(f), bool)
    gone[2 * np.arange(0, len(f) // 2, 53)] = True
    added, info = _assert_equals_ref(f[~gone], n)
    assert info["loops_filled"] == 2474 and len(added) == 2474


def test_carry_scan_runs_of_two():
    """262401 vertices are 1026 workgroups of 256: every thread of the carry scan covers a run of two.  Lone triangles in the first
    workgroup, across the workgroups 0 / 1, in the last workgroup of the last full pair and in the two after it; a quad across
    511 / 512, i.e. across two scan threads."""
    n = 1024 * 256 + 257
    q = 512 * 256 - 2
    faces = [[a, a + 1, a + 2] for a in (0, 255, 1023 * 256 + 100, 1024 * 256 + 10, n - 3)] + [[q, q + 1, q + 2], [q, q + 2, q + 3]]
    added, info = _assert_equals_ref(np.array(faces, np.int32), n, 4)
    assert added.tolist() == [[0, 2, 1], [255, 257, 256], [131070, 131072, 131071], [131070, 131073, 131072],
                              [261988, 261990, 261989], [262154, 262156, 262155], [262398, 262400, 262399]]
    assert info.pop("faces_added") == 7 and info.pop("loops_filled") == 6 and info.pop("boundary_edges") == 19
    assert not any(info.values()), info


# ---- the mesher -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = _mapper()
    kfs = _keyframes(frames)
    mesher = Mesher(cfg, mapper)
    return mesher, kfs, mesher.extract(kfs)


def test_get_mesh_holes(scene, tmp_path):
    from dns_slam_amd import ops
    mesher, kfs, (v, f, c, l) = scene
    pal = np.random.default_rng(0).integers(0, 256, size=(8, 3)).astype(np.uint8)
    plain = mesher.get_mesh(str(tmp_path / "plain"), kfs, 0, label=True, palette=pal)
    none = mesher.get_mesh(str(tmp_path / "none"), kfs, 0, label=True, palette=pal, holes=None)
    assert len(plain) == len(none) == 2 and all(filecmp.cmp(a, b, shallow=False) for a, b in zip(plain, none))
    filled = mesher.get_mesh(str(tmp_path / "filled"), kfs, 0, label=True, palette=pal, holes=True)
    exp, info = ops.mesh_fill_holes(f, v.shape[0])
    pv, pf = mc_ref.read_ply(filled[0])
    assert np.array_equal(pf, exp.cpu().numpy()) and len(pv) == v.shape[0]
    sv, sf = mc_ref.read_ply(filled[1])
    assert np.array_equal(sf, f.cpu().numpy())
    v4, f4, c4, l4 = mesher.extract(kfs, holes=4)
    assert torch.equal(f4, exp) and torch.equal(v4, v) and torch.equal(c4, c) and torch.equal(l4, l)
    assert torch.equal(mesher.extract(kfs, holes=6)[1], ops.mesh_fill_holes(f, v.shape[0], 6)[0])
    for bad in (2, 33, False, "yes"):
        with pytest.raises(ValueError):
            mesher.extract(kfs, holes=bad)
    with pytest.raises(NotImplementedError, match="holes=True"):
        mesher.get_mesh(str(tmp_path / "refused"), kfs, 0, fill_holes=True)


def test_mesher_fill_holes_brings_faces_back(scene):
    mesher, kfs, (v, f, c, l) = scene
    fn = f.cpu().numpy()
    a, b, _, _ = fr.boundary(fn, v.shape[0])
    on_boundary = np.zeros(v.shape[0], bool)
    on_boundary[a] = True
    e = np.sort(np.stack((fn, fn[:, [1, 2, 0]]), 2).reshape(-1, 2).astype(np.int64), 1)             # edge 3 f + k
    _, inv, cnt = np.unique(e[:, 0] << 32 | e[:, 1], return_inverse=True, return_counts=True)
    manifold = (cnt[inv].reshape(-1, 3) == 2).all(1)                 # the faces whose three edges two faces hold
    rng = np.random.default_rng(9)
    used, gone = on_boundary.copy(), []                              # interior faces, no two sharing a vertex
    for i in rng.permutation(len(fn)).tolist():
        if len(gone) < 20 and manifold[i] and not used[fn[i]].any():
            used[fn[i]] = True
            gone.append(i)
    assert len(gone) == 20
    vs = fn[gone].reshape(-1)
    assert len(np.unique(vs)) == 60 and not on_boundary[vs].any()
    keep = np.ones(len(fn), bool)
    keep[gone] = False
    out, info = mesher.fill_holes(v, _t(fn[keep]))
    r_added, r_info = fr.fill_holes(fn[keep], v.shape[0])
    assert info == r_info and torch.equal(out[int(keep.sum()):].cpu(), torch.from_numpy(r_added))
    back = out[int(keep.sum()):].cpu().numpy()
    mine = np.isin(back[:, 0], vs)                                   # the loops of the deleted faces (others: the mesh's own 3- and 4-holes)
    assert np.array_equal(fr.canon(back[mine]), fr.canon(fn[gone]))
    assert np.array_equal(fr.canon(back[~mine]), fr.canon(fr.fill_holes(fn, v.shape[0])[0]))
