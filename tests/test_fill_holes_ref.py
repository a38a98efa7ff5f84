"""CPU: the host restatement of the hole filling (tests/fill_holes_ref.py) on hand-built meshes with the added faces written out,
against networkx.cycle_basis and trimesh's rules where every boundary vertex is simple, and the C ABI's size refusals."""
import numpy as np
import pytest

import fill_holes_ref as fr


@pytest.mark.parametrize("name", sorted(fr.HAND_CASES))
def test_hand_cases(name):
    c = fr.HAND_CASES[name]
    added, info = fr.fill_holes(c["faces"], c["n_verts"], c["max_edges"])
    assert added.dtype == np.int32 and np.array_equal(added, c["added"]), added
    assert info["faces_added"] == len(c["added"]) and info["bad_index"] == 0
    for k, v in c["info"].items():
        assert info[k] == v, (k, info)
    assert info["watertight"] == (info["boundary_edges"] == 0 and info["nonmanifold_edges"] == 0)


def test_refusals_and_empty():
    with pytest.raises(ValueError):
        fr.fill_holes([[0, 1, 4]], 4)
    with pytest.raises(ValueError):
        fr.fill_holes([[0, 1, -1]], 4)
    for bad in (2, 33):
        with pytest.raises(ValueError):
            fr.fill_holes([[0, 1, 2]], 3, bad)
    added, info = fr.fill_holes(np.zeros((0, 3), np.int32), 7)
    assert added.shape == (0, 3) and info["watertight"] and all(info[k] == 0 for k in fr.INFO_KEYS)


def test_filled_mesh_is_closed_and_wound():
    """Tetrahedron and octahedron with any one face removed: the filled mesh pairs every directed edge with its reverse."""
    for solid, n in ((fr.TETRAHEDRON, 4), (fr.OCTAHEDRON, 6)):
        for gone in range(len(solid)):
            f = np.delete(solid, gone, 0)
            added, info = fr.fill_holes(f, n)
            assert np.array_equal(fr.canon(added), fr.canon(solid[[gone]])) and info["loops_filled"] == 1
            assert fr.directed_edges_paired(np.concatenate((f, added)))


def _torus_case():
    f, n = fr.torus(24, 24, seed=5)
    holes = fr.torus_holes(f, n, seed=11)
    return f, n, holes, f[~fr.holes_mask(len(f), holes)]


def test_torus_hole_set():
    f, n, holes, open_f = _torus_case()
    assert len(holes["tri"]) >= 10 and len(holes["quad"]) >= 10 and len(holes["hex"]) >= 3
    assert all(len(h) == 6 for h in holes["hex"])
    added, info = fr.fill_holes(open_f, n)
    assert info["vertices_skipped"] == 0 and info["nonmanifold_edges"] == 0
    assert info["loops_filled"] == len(holes["tri"]) + len(holes["quad"]) and len(added) == len(holes["tri"]) + 2 * len(holes["quad"])
    assert info["boundary_edges"] == 3 * len(holes["tri"]) + 4 * len(holes["quad"]) + 6 * len(holes["hex"])
    # the smallest vertex of a loop is not always the removed face's first
    assert any(int(f[t].argmin()) != 0 for t in holes["tri"])
    all6, info6 = fr.fill_holes(open_f, n, 6)
    assert info6["loops_filled"] == sum(len(v) for v in holes.values())
    assert fr.directed_edges_paired(np.concatenate((open_f, all6)))


def _check_against_cycle_basis(faces, n_verts, max_edges=4):
    """Where every boundary vertex is simple: the filled loops are the cycles of 3 and 4 edges of the boundary graph, a 3-loop's
    face and a quad's two faces are trimesh's (hole[[0,1,2]] / hole[[0,1,2]], hole[[2,3,0]] of the cycle in some rotation), wound
    against the boundary half-edges."""
    nx = pytest.importorskip("networkx")
    a, b, _, _ = fr.boundary(faces, n_verts)
    added, info = fr.fill_holes(faces, n_verts, max_edges)
    assert info["vertices_skipped"] == 0
    g = nx.Graph()
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    cycles = [c for c in nx.cycle_basis(g) if 3 <= len(c) <= 4]
    loops = [lp for lp in fr.simple_loops(a, b, n_verts)[0] if 3 <= len(lp) <= 4]
    assert sorted(map(sorted, cycles)) == sorted(map(sorted, loops))
    half = set(zip(a.tolist(), b.tolist()))
    by_owner = {}
    for face in added.tolist():
        by_owner.setdefault(face[0], []).append(face)
        for k in range(3):                                           # a new face never repeats a boundary half-edge: it reverses it
            p, q = face[k], face[(k + 1) % 3]
            assert (p, q) not in half
    for cyc in cycles:
        got = by_owner[min(cyc)]
        closed = {(q, p) for f3 in got for p, q in zip(f3, f3[1:] + f3[:1])} & half
        assert closed == {e for e in half if e[0] in cyc}            # every half-edge of the cycle is reversed by a new face
        if len(cyc) == 3:
            assert len(got) == 1 and sorted(got[0]) == sorted(cyc)
        else:
            tri = lambda r: {frozenset((cyc[r], cyc[(r + 1) % 4], cyc[(r + 2) % 4])), frozenset((cyc[(r + 2) % 4], cyc[(r + 3) % 4], cyc[r]))}
            assert len(got) == 2 and {frozenset(f3) for f3 in got} in (tri(0), tri(1))
    return len(cycles)


def test_against_cycle_basis():
    for name in ("tetrahedron_minus_face", "octahedron_minus_adjacent", "octahedron_minus_opposite", "lone_triangle", "cone_5_of_4"):
        c = fr.HAND_CASES[name]
        _check_against_cycle_basis(c["faces"], c["n_verts"])
    f, n, holes, open_f = _torus_case()
    assert _check_against_cycle_basis(open_f, n) == len(holes["tri"]) + len(holes["quad"])


def test_restatement_is_quick_on_the_large_torus():
    """512 x 256, every 53rd cell's lower face gone: the shape of the GPU test; the loops are the removed faces."""
    f, n = fr.torus(512, 256)
    gone = np.zeros(len(f), bool)
    gone[2 * np.arange(0, len(f) // 2, 53)] = True
    added, info = fr.fill_holes(f[~gone], n)
    assert info["vertices_skipped"] == 0 and info["loops_filled"] == int(gone.sum()) == 2474
    assert np.array_equal(fr.canon(added), fr.canon(f[gone]))


def test_abi_sizes():
    from dns_slam_amd import _lib
    ws = lambda F, V: int(_lib.lib.dns_mesh_holes_ws_bytes(F, V))
    assert ws(0, 10) == 0 and ws(1 << 29, 10) == 0 and ws(10, 1 << 31) == 0
    assert ws(1, 0) > 0 and ws(1, 3) % 256 == 0 and ws((1 << 29) - 1, (1 << 31) - 1) > 16 * 4 * ((1 << 29) - 1)
    assert _lib.lib.dns_mesh_holes_count(None, 1 << 29, 3, 4, None, None, None) == -1
    assert _lib.lib.dns_mesh_holes_count(None, 1, 3, 2, None, None, None) == -1
    assert _lib.lib.dns_mesh_holes_count(None, 1, 3, 33, None, None, None) == -1
    assert _lib.lib.dns_mesh_holes_emit(None, 3, 4, None, None) == -1
    assert _lib.lib.dns_mesh_holes_emit(None, 0, 4, None, None) == 0       # V = 0: nothing to do
