"""CPU: the host reference of the mesh component pass (tests/mesh_cc_ref.py) on hand-built meshes with known answers and on
the five-sphere field the GPU tests use."""
import numpy as np

import mc_ref
import mesh_cc_ref as cc


def _partition(comp):
    return sorted(tuple(np.nonzero(comp == c)[0]) for c in np.unique(comp))


def test_two_octahedra_exact_areas():
    v, f = cc.two_octahedra()
    comp, area, n = cc.components(v, f)
    assert n == 2 and comp.dtype == np.int32 and area.dtype == np.float64
    assert (comp == np.repeat([0, 8], 8)).all()
    # a face of the octahedron of radius r has area sqrt(3) r^2 / 2, each product exact in float64; 8 terms per sum
    for sl, r in ((slice(0, 8), 1.0), (slice(8, 16), 2.0)):
        exact = 4 * np.sqrt(3.0) * r * r
        assert (np.abs(area[sl] - exact) <= 8 * 2.0 ** -52 * exact).all()
    assert (cc.face_areas(v, f)[:8] == 0.5 * np.sqrt(3.0)).all()


def test_shared_vertex_does_not_join():
    v, f = cc.touching_tetrahedra()
    comp, area, n = cc.components(v, f)
    assert n == 2 and (comp == np.repeat([0, 4], 4)).all()
    assert mc_ref.check_manifold(f)[0]


def test_non_manifold_edge_joins_nothing():
    v, f = cc.fan()
    comp, area, n = cc.components(v, f)
    assert n == 3 and (comp == [0, 1, 2]).all() and (area == 0.5).all()
    assert len(cc.face_adjacency(f)) == 0


def test_open_strip_is_one_component():
    v, f = cc.strip(7)
    comp, area, n = cc.components(v, f)
    assert n == 1 and (comp == 0).all() and (area == 3.5).all()
    assert cc.boundary_edges(f) == 9
    v, f = cc.strip(5000, closed=True)
    comp, area, n = cc.components(v, f)
    assert n == 1 and (comp == 0).all() and cc.boundary_edges(f) == 5000
    assert int(f.max()) < len(v) and len(cc.face_adjacency(f)) == 5000


def test_face_listed_twice():
    v, f = cc.doubled_face()
    comp, area, n = cc.components(v, f)
    assert n == 1 and (comp == 0).all() and (area == 1.0).all()
    # an edge key that occurs twice inside ONE face joins nothing: (0, 1) below is held by the degenerate face 1 alone
    f2 = np.array([[0, 1, 2], [0, 1, 0]], np.int32)
    assert cc.components(v, f2)[2] == 2


def test_empty_and_single():
    assert cc.components(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))[2] == 0
    comp, area, n = cc.components(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32))
    assert n == 1 and comp[0] == 0 and abs(area[0] - 0.5 * np.sqrt(3.0)) <= 2.0 ** -52


def test_five_spheres():
    v, f = cc.five_spheres()
    assert v.shape == (2014, 3) and f.shape == (4008, 3)
    assert mc_ref.check_manifold(f) == (True, True) and cc.boundary_edges(f) == 0
    comp, area, n = cc.components(v, f)
    assert n == 5
    roots = np.unique(comp)
    assert (comp[roots] == roots).all()                                   # the id is a face of the component: its smallest
    assert all(np.nonzero(comp == r)[0].min() == r for r in roots)
    per = np.sort(area[roots])
    assert np.allclose(per, [0.0336, 0.1704, 0.4922, 0.7750, 2.0002], atol=5e-5)
    assert abs(per.sum() - mc_ref.area(v, f)) <= 1e-12
    assert int((per > 0.2).sum()) == 3 and np.abs(per / 0.2 - 1).min() > 0.14
    # every component is a closed surface of its own: Euler characteristic 2
    for r in roots:
        assert mc_ref.euler(v, f[comp == r]) == 2
    # the partition does not depend on the order of the faces
    perm = np.random.default_rng(0).permutation(len(f))
    comp_p = cc.components(v, f[perm])[0]
    back = np.empty_like(comp_p)
    back[perm] = comp_p
    assert _partition(back) == _partition(comp)


def test_other_gpu_cases_are_what_the_tests_assume():
    v, f = cc.random_surface()
    comp, area, n = cc.components(v, f)
    assert len(f) == 15852 and n == 3
    assert np.allclose(np.sort(area[np.unique(comp)]), [0.008, 0.970, 23.566], atol=5e-4)
    v, f = cc.open_surface()
    assert len(f) == 3602 and cc.boundary_edges(f) == 328 and cc.components(v, f)[2] == 1


def test_workspace_size_and_refused_sizes():
    """Host arithmetic of the C ABI (no launch): 84 bytes per face (4F table slots of 20 bytes + the parents), each of the four
    arrays padded to 256 bytes; 2^29 faces and more are refused."""
    from dns_slam_amd import _lib
    ws = lambda F: int(_lib.lib.dns_mesh_cc_ws_bytes(F))
    assert ws(0) == 0 and ws(1 << 29) == 0 and ws((1 << 32) - 1) == 0
    assert ws(64) == 84 * 64 and ws(1 << 20) == 84 << 20
    assert 84 <= ws(1) <= 84 + 3 * 256 and 84 * 1001 <= ws(1001) <= 84 * 1001 + 3 * 256
    assert _lib.lib.dns_mesh_components(None, 0, None, 1 << 29, None, None, None, None, None) == -1
    assert b"2^29" in _lib.lib.dns_last_error()
    assert _lib.lib.dns_mesh_components(None, 0, None, 0, None, None, None, None, None) == 0      # F = 0: nothing to do
