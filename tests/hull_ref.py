"""The yardstick of ops.convex_hull: scipy's ConvexHull (Qhull) and the acceptance a hull is held to.

With L the largest absolute coordinate and r = 1e-9 L (float64 plane evaluation errs by a few ulp of L, about 1e-15 L; r leaves
room for sliver faces and is still far below any eps in use):
  (a) max_outside <= eps + r, recomputed here in numpy over all points and faces;
  (b) every vertex v of scipy's hull has max_f (n_f . v + d_f) >= -(eps + r): the hull under-approximates by at most eps;
  (c) structure: every directed edge has exactly one twin, normals are unit and finite, each face's own vertices lie within r of
      its plane, and the mean of the hull vertices is strictly inside.
"""
import numpy as np
from scipy.spatial import ConvexHull


def scipy_hull(points):
    return ConvexHull(np.asarray(points, np.float64))


def plane_values(planes, pts):
    """[P,F]: ((n0 x + n1 y) + n2 z) + d, the order ops.convex_hull and meshing.inside_planes evaluate."""
    return ((pts[:, None, 0] * planes[None, :, 0] + pts[:, None, 1] * planes[None, :, 1]) + pts[:, None, 2] * planes[None, :, 2]) + planes[None, :, 3]


def max_over_faces(planes, pts, chunk=64):
    """[P]: the largest plane value per point.  A matrix product here (its rounding differs from plane_values' by a few ulp of L,
    far inside r): the checks that use it compare against r or exclude the points within r of a plane."""
    out = np.full(pts.shape[0], -np.inf)
    for s in range(0, planes.shape[0], chunk):
        out = np.maximum(out, (pts @ planes[s:s + chunk, :3].T + planes[s:s + chunk, 3]).max(1))
    return out


def accept(points, eps, vertex_index, faces, planes, max_outside, hull=None):
    """Asserts (a)-(c); returns the figures it measured."""
    pts = np.asarray(points, np.float64)
    vi, fc, pl = np.asarray(vertex_index), np.asarray(faces), np.asarray(planes, np.float64)
    L = float(np.abs(pts).max())
    r = 1e-9 * L
    # (c)
    assert fc.ndim == 2 and fc.shape[1] == 3 and pl.shape == (fc.shape[0], 4) and fc.shape[0] >= 4
    assert fc.min() >= 0 and fc.max() < pts.shape[0]
    assert np.array_equal(vi, np.unique(fc)), "vertex_index is not the ascending set of the faces' vertices"
    assert np.isfinite(pl).all()
    nl = np.sqrt((pl[:, :3] ** 2).sum(1))
    assert np.abs(nl - 1.0).max() < 1e-12, nl
    de = np.concatenate((fc[:, [0, 1]], fc[:, [1, 2]], fc[:, [2, 0]]))
    key = de[:, 0].astype(np.int64) * pts.shape[0] + de[:, 1]
    twin = de[:, 1].astype(np.int64) * pts.shape[0] + de[:, 0]
    assert np.unique(key).size == key.size, "a directed edge is held twice"
    assert np.array_equal(np.sort(key), np.sort(twin)), "a directed edge has no twin"
    own = np.abs(np.stack([((pl[:, 0] * pts[fc[:, k], 0] + pl[:, 1] * pts[fc[:, k], 1]) + pl[:, 2] * pts[fc[:, k], 2]) + pl[:, 3]
                           for k in range(3)]))
    assert own.max() <= r, (own.max(), r)
    centre = pts[vi].mean(0)
    assert plane_values(pl, centre[None]).max() < 0.0, "the mean of the hull vertices is not strictly inside"
    # (a)
    mo = float(max_over_faces(pl, pts).max())
    assert mo <= eps + r, (mo, eps, r)
    assert max_outside <= eps + r and abs(max_outside - mo) <= r, (max_outside, mo)
    # (b)
    hull = hull if hull is not None else scipy_hull(pts)
    deepest = float(max_over_faces(pl, pts[hull.vertices]).min())
    assert deepest >= -(eps + r), (deepest, eps, r)
    return {"L": L, "max_outside": mo, "deepest_scipy_vertex": deepest, "faces": int(fc.shape[0]), "vertices": int(vi.size),
            "scipy_vertices": int(hull.vertices.size)}


def scaled_planes(points, scale, hull=None):
    """The reference's bound as half-spaces: scipy's hull of ``points`` scaled by ``scale`` about the mean c of its vertices; a
    face (n, d) becomes (n, s d + (s - 1) n . c)."""
    pts = np.asarray(points, np.float64)
    hull = hull if hull is not None else scipy_hull(pts)
    c = pts[hull.vertices].mean(0)
    eq = hull.equations
    nc = (eq[:, 0] * c[0] + eq[:, 1] * c[1]) + eq[:, 2] * c[2]
    return np.concatenate((eq[:, :3], (scale * eq[:, 3] + (scale - 1.0) * nc)[:, None]), 1), c
