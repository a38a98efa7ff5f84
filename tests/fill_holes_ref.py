"""Host restatement of csrc/mesh_holes.hip (the reference's mesh.fill_holes(), trimesh.repair.fill_holes, under the definition of
include/dns_hip.h), with numpy, written the other way round from the kernels: the 3F edge keys are sorted and counted
(np.unique) where the kernels hash them, and the loops are collected by one sweep over the boundary vertices in ascending order
that marks what it has visited, where the kernels walk from every vertex.

    An undirected edge exactly one face edge holds is a boundary edge, directed as its face winds it.  A vertex is simple iff one
    boundary edge leaves it and one enters it.  A loop of 3 .. max_edges edges whose vertices are all simple gets the fan
    (v0, v[i+1], v[i]), i = 1 .. L-2, from its smallest vertex v0; loops in ascending order of v0.
"""
from __future__ import annotations

import numpy as np

INFO_KEYS = ("faces_added", "loops_filled", "boundary_edges", "nonmanifold_edges", "vertices_skipped", "degenerate", "bad_index")


def boundary(faces, n_verts):
    """-> (a, b: int64 [B] the directed boundary half-edges a -> b, nonmanifold_edges, degenerate)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((f < 0) | (f >= n_verts)).any():
        raise ValueError(f"fill_holes_ref: a face holds a vertex index outside [0, {n_verts})")
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                # face edge 3 f + k
    ok = a != b
    a, b = a[ok], b[ok]
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    _, first, count = np.unique(key, return_index=True, return_counts=True)
    once = first[count == 1]
    return a[once], b[once], int((count >= 3).sum()), int((~ok).sum())


def simple_loops(a, b, n_verts):
    """-> (loops: the closed walks through simple vertices, each a list that starts at its smallest vertex, in ascending order of
    it, of ANY length; vertices_skipped)."""
    n_out, n_in = np.bincount(a, minlength=n_verts), np.bincount(b, minlength=n_verts)
    simple = (n_out == 1) & (n_in == 1)
    skipped = int(((n_out + n_in > 0) & ~simple).sum())
    from_simple = simple[a]
    succ = dict(zip(a[from_simple].tolist(), b[from_simple].tolist()))
    is_simple = set(np.nonzero(simple)[0].tolist())
    visited, loops = set(), []
    for v in sorted(succ):
        if v in visited:
            continue
        walk, u = [v], succ[v]
        visited.add(v)
        while u in is_simple and u not in visited:
            visited.add(u)
            walk.append(u)
            u = succ[u]
        if u == v:
            loops.append(walk)
    return loops, skipped


def fill_holes(faces, n_verts, max_edges=4):
    """-> (added int32 [A,3], info dict with INFO_KEYS and ``watertight``)."""
    if not 3 <= int(max_edges) <= 32:
        raise ValueError(f"fill_holes_ref: max_edges {max_edges}")
    a, b, nonmanifold, degenerate = boundary(faces, n_verts)
    loops, skipped = simple_loops(a, b, n_verts)
    added, filled = [], 0
    for lp in loops:
        if 3 <= len(lp) <= max_edges:
            filled += 1
            added += [(lp[0], lp[i + 1], lp[i]) for i in range(1, len(lp) - 1)]
    info = dict(faces_added=len(added), loops_filled=filled, boundary_edges=int(len(a)), nonmanifold_edges=nonmanifold,
                vertices_skipped=skipped, degenerate=degenerate, bad_index=0)
    info["watertight"] = info["boundary_edges"] == 0 and nonmanifold == 0
    return np.asarray(added, np.int32).reshape(-1, 3), info


def canon(faces):
    """Each face rotated to start at its smallest index (the winding kept), the rows sorted: equality up to rotation and order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = f.argmin(1)
    r = np.stack((f[np.arange(len(f)), k], f[np.arange(len(f)), (k + 1) % 3], f[np.arange(len(f)), (k + 2) % 3]), 1)
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


def directed_edges_paired(faces):
    """True iff every directed edge occurs once and its reverse occurs once: watertight and consistently wound."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    fwd, cnt = np.unique((a << 32) | b, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(fwd, np.unique((b << 32) | a)))


# ---- meshes: faces int32 [F,3] over n vertices ----------------------------------------------------------------------------------
TETRAHEDRON = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)                  # outward over (0,0,0), x, y, z
OCTAHEDRON = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)


def cone_fan(n):
    """n faces (apex n, rim i, rim i + 1 mod n): one boundary loop 0 -> 1 -> ... -> n - 1 -> 0 of the n rim vertices."""
    i = np.arange(n)
    return np.stack((np.full(n, n), i, (i + 1) % n), 1).astype(np.int32), n + 1


def _fan_from_zero(n):
    return [[0, i + 1, i] for i in range(1, n - 1)]


def _case(faces, n_verts, added, max_edges=4, **info):
    return dict(faces=np.asarray(faces, np.int32).reshape(-1, 3), n_verts=n_verts, max_edges=max_edges,
                added=np.asarray(added, np.int32).reshape(-1, 3), info=info)


# name -> faces, n_verts, max_edges, the added faces written out, and the info entries worth pinning
HAND_CASES = {
    # the missing face (1, 2, 3) comes back, outward, from its smallest vertex
    "tetrahedron_minus_face": _case(TETRAHEDRON[[0, 1, 3]], 4, [[1, 2, 3]], loops_filled=1, boundary_edges=3, vertices_skipped=0),
    # faces (0,2,4) and (2,1,4) gone: the quad 0 -> 4 -> 1 -> 2, diagonal from 0
    "octahedron_minus_adjacent": _case(OCTAHEDRON[2:], 6, [[0, 1, 4], [0, 2, 1]], loops_filled=1, boundary_edges=4),
    # faces (0,2,4) and (3,1,5) gone: both come back, owner 0 before owner 1
    "octahedron_minus_opposite": _case(OCTAHEDRON[[1, 2, 3, 4, 5, 7]], 6, [[0, 2, 4], [1, 5, 3]], loops_filled=2, boundary_edges=6),
    # faces (0,2,4) and (1,3,4) gone: the two holes touch in vertex 4
    "octahedron_minus_touching": _case(OCTAHEDRON[[1, 3, 4, 5, 6, 7]], 6, [], loops_filled=0, boundary_edges=6, vertices_skipped=1),
    "cone_32_of_32": _case(cone_fan(32)[0], 33, _fan_from_zero(32), 32, faces_added=30, loops_filled=1, boundary_edges=32),
    "cone_33_of_32": _case(cone_fan(33)[0], 34, [], 32, loops_filled=0, boundary_edges=33, vertices_skipped=0),
    "cone_5_of_4": _case(cone_fan(5)[0], 6, [], loops_filled=0, boundary_edges=5, vertices_skipped=0),
    "cone_5_of_5": _case(cone_fan(5)[0], 6, [[0, 2, 1], [0, 3, 2], [0, 4, 3]], 5, loops_filled=1),
    # three faces on the edge (0, 1): not a boundary edge; 0 and 1 each have two boundary edges one way
    "three_on_an_edge": _case([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5, [], nonmanifold_edges=1, boundary_edges=6, vertices_skipped=2,
                              loops_filled=0),
    # the tetrahedron's 3-hole with the face (0, 2, 1) next to it flipped: two boundary edges leave 1, two enter 2
    "flipped_next_to_hole": _case([[0, 1, 2], [0, 1, 3], [0, 3, 2]], 4, [], loops_filled=0, boundary_edges=3, vertices_skipped=2),
    "lone_triangle": _case([[0, 1, 2]], 3, [[0, 2, 1]], loops_filled=1, boundary_edges=3),
    # (3, 3, 4): one degenerate edge, and 3 -> 4, 4 -> 3 hold one key twice
    "repeated_index": _case([[0, 1, 2], [3, 3, 4]], 5, [[0, 2, 1]], degenerate=1, boundary_edges=3, loops_filled=1, vertices_skipped=0),
    "closed_octahedron": _case(OCTAHEDRON, 6, [], watertight=True, boundary_edges=0, nonmanifold_edges=0, loops_filled=0),
}


def torus(n, m, seed=None):
    """The n x m quad torus, each cell (i, j) cut into the lower face 2 c = (v00, v10, v11) and the upper face 2 c + 1 =
    (v00, v11, v01), c = i m + j, vertex (i, j) = i m + j; with ``seed`` the vertices are relabelled by a seeded permutation.
    -> (faces int32 [2 n m, 3], n m)."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    i1, j1 = (i + 1) % n, (j + 1) % m
    v00, v10, v11, v01 = i * m + j, i1 * m + j, i1 * m + j1, i * m + j1
    f = np.stack((np.stack((v00, v10, v11), 1), np.stack((v00, v11, v01), 1)), 1).reshape(-1, 3)
    if seed is not None:
        f = np.random.default_rng(seed).permutation(n * m)[f]
    return f.astype(np.int32), n * m


def torus_holes(faces, n_verts, seed, n_tri=12, n_quad=12, n_hex=4):
    """A seeded set of holes in a torus whose vertices are all simple afterwards: single faces, both faces of a cell and the six
    faces round a vertex, no two holes sharing a vertex; a candidate is kept only if the restatement then reports
    vertices_skipped == 0.  -> {"tri": [face], "quad": [(f, f + 1)], "hex": [(six faces)]}."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces)
    used = np.zeros(n_verts, bool)
    removed = np.zeros(len(f), bool)
    out = {"tri": [], "quad": [], "hex": []}
    want = {"tri": n_tri, "quad": n_quad, "hex": n_hex}
    for kind in ("hex", "quad", "tri"):
        for _ in range(2000):
            if len(out[kind]) == want[kind]:
                break
            if kind == "tri":
                ids = (int(rng.integers(len(f))),)
            elif kind == "quad":
                c = int(rng.integers(len(f) // 2))
                ids = (2 * c, 2 * c + 1)
            else:
                ids = tuple(np.nonzero((f == f[int(rng.integers(len(f))), 0]).any(1))[0].tolist())
            vs = np.unique(f[list(ids)])
            if used[vs].any():
                continue
            trial = removed.copy()
            trial[list(ids)] = True
            if fill_holes(f[~trial], n_verts)[1]["vertices_skipped"] != 0:
                continue
            removed, used[vs] = trial, True
            out[kind].append(ids[0] if kind == "tri" else ids)
    return out


def holes_mask(n_faces, holes):
    """bool [F]: the faces ``torus_holes`` removed."""
    gone = np.zeros(n_faces, bool)
    gone[list(holes["tri"])] = True
    for ids in holes["quad"] + holes["hex"]:
        gone[list(ids)] = True
    return gone
