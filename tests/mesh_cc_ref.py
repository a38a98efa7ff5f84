"""Host reference of csrc/mesh_cc.hip: connected components of a triangle list under trimesh's face_adjacency (what the
reference's mesh.split(only_watertight=False) uses), with numpy and scipy.sparse.csgraph.

    Of the 3F undirected edges (min(a,b), max(a,b)) of all faces, a key that occurs exactly twice joins the two faces that hold
    it (nothing if both occurrences are in one face); a key that occurs once or three or more times joins nothing; faces that
    share only a vertex are not adjacent.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def face_areas(verts, faces):
    """float64 [F]: 0.5 |(v1 - v0) x (v2 - v0)| from the float32 positions, in the operation order of the kernel."""
    v = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)


def face_adjacency(faces):
    """int64 [A, 2]: the pairs of distinct faces that are the only two holders of an undirected edge."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    if F == 0:
        return np.zeros((0, 2), np.int64)
    e = np.sort(np.stack((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]), 1).reshape(-1, 2), 1)     # edge 3 f + k
    owner = np.repeat(np.arange(F), 3)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, owner = e[order], owner[order]
    start = np.ones(len(e), bool)
    start[1:] = (e[1:] != e[:-1]).any(1)
    first = np.nonzero(start)[0]
    count = np.diff(np.append(first, len(e)))
    two = first[count == 2]
    pairs = np.stack((owner[two], owner[two + 1]), 1)
    return pairs[pairs[:, 0] != pairs[:, 1]]


def components(verts, faces):
    """-> (comp [F] int32: the smallest face index of the face's component, comp_area [F] float64: the component's area,
    n_comp)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    if F == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float64), 0
    adj = face_adjacency(f)
    g = coo_matrix((np.ones(len(adj), np.int8), (adj[:, 0], adj[:, 1])), shape=(F, F))
    n, lab = connected_components(g, directed=False)
    smallest = np.full(n, F, np.int64)
    np.minimum.at(smallest, lab, np.arange(F))
    area = np.zeros(n, np.float64)
    np.add.at(area, lab, face_areas(verts, f))
    return smallest[lab].astype(np.int32), area[lab], int(n)


def boundary_edges(faces):
    """The number of undirected edges exactly one face holds."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), 1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return int((cnt == 1).sum())


# ---- hand-built meshes with known answers: name -> (verts float32 [V,3], faces int32 [F,3]) -------------------------------
def octahedron(r, centre=(0.0, 0.0, 0.0)):
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], np.float32) + np.asarray(centre, np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def two_octahedra():
    """Radii 1 and 2 (powers of two: every product is exact), areas 4 sqrt(3) and 16 sqrt(3)."""
    (v0, f0), (v1, f1) = octahedron(1.0), octahedron(2.0, (8.0, 0.0, 0.0))
    return np.concatenate((v0, v1)), np.concatenate((f0, f1 + len(v0))).astype(np.int32)


def touching_tetrahedra():
    """Two tetrahedra that share vertex 0 and nothing else."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
    t = lambda a, b, c, d: [[a, b, c], [a, c, d], [a, d, b], [b, d, c]]
    return v, np.array(t(0, 1, 2, 3) + t(0, 4, 5, 6), np.int32)


def fan():
    """Three triangles on the common edge (0, 1): a non-manifold edge joins nothing."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def strip(n, closed=False):
    """n triangles between two rows of vertices; ``closed`` joins the last pair of vertices to the first (n even)."""
    m = (n + 1) // 2 + 1
    t = np.arange(m, dtype=np.float64)
    if closed:
        assert n % 2 == 0
        ang = 2 * np.pi * t / (m - 1)
        row = np.stack((np.cos(ang), np.sin(ang)), 1) * (m / 6.0)
    else:
        row = np.stack((t, np.zeros(m)), 1)
    v = np.concatenate((np.concatenate((row, np.zeros((m, 1))), 1), np.concatenate((row, np.ones((m, 1))), 1))).astype(np.float32)
    i = np.arange(m - 1)
    lo = np.stack((i, i + 1, i + m), 1)                     # bottom i, bottom i + 1, top i
    hi = np.stack((i + 1, i + 1 + m, i + m), 1)             # bottom i + 1, top i + 1, top i
    f = np.stack((lo, hi), 1).reshape(-1, 3)[:n]
    if closed:
        f = np.where(f == m - 1, 0, np.where(f == 2 * m - 1, m, f))
    return v, f.astype(np.int32)


def doubled_face():
    """One face listed twice: each of its edge keys occurs exactly twice, in two faces."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 2]], np.int32)


SPHERES = (((-0.45, -0.4, -0.3), 0.40), ((0.5, 0.45, 0.2), 0.25), ((0.55, -0.5, 0.5), 0.12), ((-0.6, 0.6, 0.6), 0.06),
           ((0.0, 0.7, -0.7), 0.20))


def five_spheres():
    """max_i (r_i - |p - c_i|) on mc_ref._grid(40), level 0: five closed surfaces of very different size."""
    import mc_ref
    (X, Y, Z), o, sp = mc_ref._grid(40)
    field = np.max([r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) for c, r in SPHERES], 0)
    return mc_ref.marching_cubes(field.astype(np.float32), 0.0, o, sp)


def open_surface():
    """sin(3x + 1) + sin(4y) + sin(5z + 2) at level 0.3 on mc_ref._grid(20): one sheet that leaves the grid."""
    import mc_ref
    (X, Y, Z), o, sp = mc_ref._grid(20)
    field = np.sin(3 * X + 1) + np.sin(4 * Y) + np.sin(5 * Z + 2)
    return mc_ref.marching_cubes(field.astype(np.float32), 0.3, o, sp)


def random_surface():
    import mc_ref
    vol, o, sp, _ = mc_ref.random_field(32, seed=0)
    return mc_ref.marching_cubes(vol, 0.0, o, sp)


HAND_BUILT = {"two_octahedra": two_octahedra, "touching_tetrahedra": touching_tetrahedra, "fan": fan,
              "open_strip": lambda: strip(7), "doubled_face": doubled_face}
