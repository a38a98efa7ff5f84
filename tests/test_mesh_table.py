"""CPU: the generated marching-cubes table (tools/gen_mc_table.py -> csrc/mc_table.hpp), the numpy restatement of the GPU
marching cubes (tests/mc_ref.py) on closed analytic surfaces, and the PLY writer of dns_slam_amd.meshing."""
import os
import itertools

import numpy as np
import pytest

import mc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = mc_ref.load_generator()


def test_table_header_is_the_generator_output():
    with open(os.path.join(ROOT, "dns_slam_amd", "csrc", "mc_table.hpp")) as f:
        committed = f.read()
    assert GEN.render(GEN.build_table()) == committed


# ---- an independent statement of the rule: corners, edges and faces from coordinates ------------------------------------
def _corner(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def _edge_ends(e):
    a = e // 4
    o = [x for x in range(3) if x != a]
    p = np.zeros(3, int)
    p[o[0]], p[o[1]] = e & 1, (e >> 1) & 1
    q = p.copy()
    q[a] = 1
    return p, q


def _rule_segments(case, a, s):
    """Directed segments on cube face (axis a, side s): the face's sign-changing edges paired (ambiguous face: around each
    inside corner), run so that (B - A) x n points to the inside corner's side, n the outward normal."""
    n = np.zeros(3)
    n[a] = 1 if s else -1
    corners = [c for c in range(8) if _corner(c)[a] == s]
    inside = {c: bool((case >> c) & 1) for c in corners}
    edges = [e for e in range(12) if e // 4 != a and _edge_ends(e)[0][a] == s]
    cross = [e for e in edges if inside[int(np.dot(_edge_ends(e)[0], [1, 2, 4]))] != inside[int(np.dot(_edge_ends(e)[1], [1, 2, 4]))]]
    mid = {e: (_edge_ends(e)[0] + _edge_ends(e)[1]) / 2 for e in range(12)}
    if not cross:
        return set()
    ins = [c for c in corners if inside[c]]
    if len(cross) == 2:
        groups = [(cross, ins[0])]
    else:
        assert len(cross) == 4 and len(ins) == 2
        groups = [([e for e in cross if np.abs(mid[e] - _corner(c)).sum() == 0.5], c) for c in ins]
    segs = set()
    for (ea, eb), c in groups:
        d = mid[eb] - mid[ea]
        side = np.dot(np.cross(d, n), _corner(c) - mid[ea])
        assert side != 0
        segs.add((ea, eb) if side > 0 else (eb, ea))
    return segs


def test_table_boundaries_are_the_rule_segments():
    table = GEN.build_table()
    assert max(len(t) for t in table) == 5
    for case in range(256):
        directed = [(t[i], t[(i + 1) % 3]) for t in table[case] for i in range(3)]
        assert len(set(directed)) == len(directed), case                      # each directed edge once
        boundary = {d for d in directed if (d[1], d[0]) not in directed}
        rule = set().union(*(_rule_segments(case, a, s) for a in range(3) for s in (0, 1)))
        assert boundary == rule, (case, boundary, rule)


def test_shared_faces_glue_with_opposite_directions():
    """Cube A's face (a, 1) is cube B's face (a, 0): whatever the other corners, the segments are the same with the edges
    shifted along a, and run the other way."""
    def shift(e, a):                                  # edge of face (a, 1) of A -> the same edge as an edge of face (a, 0) of B
        p, q = _edge_ends(e)
        p[a] -= 1
        return next(f for f in range(12) if f // 4 == e // 4 and (_edge_ends(f)[0] == p).all())
    for a in range(3):
        for ca in range(256):
            segs_a = _rule_segments(ca, a, 1)
            face_bits = [(ca >> c) & 1 for c in range(8) if _corner(c)[a] == 1]
            low = [c for c in range(8) if _corner(c)[a] == 0]
            for rest in range(16):
                cb = sum(bit << c for bit, c in zip(face_bits, low)) + sum(((rest >> i) & 1) << c for i, c in
                                                                          enumerate(c for c in range(8) if _corner(c)[a] == 1))
                segs_b = _rule_segments(cb, a, 0)
                assert {(shift(y, a), shift(x, a)) for x, y in segs_a} == segs_b, (a, ca, cb)


# ---- the numpy restatement on closed analytic surfaces --------------------------------------------------------------------
from mc_ref import random_field, sphere_field, torus_field  # noqa: E402


FIELDS = {"sphere": (sphere_field, 2), "torus": (torus_field, 0), "random": (random_field, None)}


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_mc_ref_closed_oriented_surfaces(name):
    make, chi = FIELDS[name]
    vol, o, sp, grad = make()
    v, f = mc_ref.marching_cubes(vol, 0.0, o, sp)
    assert len(f) > 1000
    two_faces, directed_once = mc_ref.check_manifold(f)
    assert two_faces and directed_once
    assert np.unique(f).size == len(v)                    # every vertex used
    if chi is not None:
        assert mc_ref.euler(v, f) == chi
    c = v[f].astype(np.float64).mean(1)
    n = mc_ref.face_normals(v, f)
    g = grad(c)
    inner = (n * g).sum(1)
    keep = np.abs(c).max(1) < 0.9                          # away from the -100 shell of the random field
    assert np.mean(inner[keep] < 0) >= 0.99                # normals point down the gradient (inside = high values)


def test_mc_ref_vertices_on_their_edges():
    vol, o, sp, _ = sphere_field(32)
    v, f = mc_ref.marching_cubes(vol, 0.0, o, sp)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(r - 0.6).max() < 0.01
    empty_v, empty_f = mc_ref.marching_cubes(np.full((8, 8, 8), -1, np.float32), 0.0, o, sp)
    assert empty_v.shape == (0, 3) and empty_f.shape == (0, 3)


def test_ply_round_trip(tmp_path):
    from dns_slam_amd.meshing import label_colors, write_ply
    rng = np.random.default_rng(3)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    f = rng.integers(0, 50, size=(70, 3)).astype(np.int32)
    c = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    lab = rng.integers(-1, 8, size=50)
    p = str(tmp_path / "m.ply")
    write_ply(p, v, f, c, lab)
    rv, rf = mc_ref.read_ply(p)
    assert rv.dtype.names == ("x", "y", "z", "red", "green", "blue", "label")
    assert (np.stack((rv["x"], rv["y"], rv["z"]), 1) == v).all()
    assert (np.stack((rv["red"], rv["green"], rv["blue"]), 1) == c).all()
    assert (rv["label"] == lab).all() and (rf == f).all()
    write_ply(p, v, f)
    rv, rf = mc_ref.read_ply(p)
    assert rv.dtype.names == ("x", "y", "z") and (rf == f).all()
    pal = rng.integers(0, 256, size=(8, 3)).astype(np.uint8)
    lc = label_colors(lab, pal)
    assert (lc[lab >= 0] == pal[lab[lab >= 0]]).all() and (lc[lab < 0] == 0).all()
    assert (label_colors(lab, {i: tuple(pal[i]) for i in range(8)}) == lc).all()


def test_mesh_ops_refuse_cpu_tensors():
    import torch
    from dns_slam_amd import ops
    with pytest.raises(ValueError):
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        ops.keyframe_project(torch.zeros(5, 3), torch.eye(4)[None], torch.zeros(1, 4, 4), torch.ones(1),
                             {"fx": 1.0, "fy": 1.0, "cx": 0.0, "cy": 0.0})
