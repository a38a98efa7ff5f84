"""Host reference of dns_slam_amd/evaluation.py and csrc/mesh_eval.hip (the reference's eval_3d.py / cull_mesh.py) with numpy
and scipy, in float64, plus the small meshes and clouds the tests share.

    nearest:         cKDTree(ref).query(query) on float64 copies of the fp32 inputs
    sample_surface:  trimesh's sample_surface from given uniforms u [n,3]
    check_proj:      the frustum test of eval_3d.py:62-88 for every pose, with the quantities it compares
    accuracy / completion / completion_ratio: eval_3d.py:24-42
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial import cKDTree

DIST_RTOL = 2.0 ** -20          # |dist - ref| <= 2^-20 ref: 16 units of 2^-24 (differences, squares, sum, root: < 4; min of rounded
                                # squares: < 5 more); the reference against its own fp32 restatement showed 1.8 units


def nearest(ref, query):
    """-> (dist float64 [N], idx [N]) of the nearest reference point of each query."""
    r = np.asarray(ref, np.float32).astype(np.float64).reshape(-1, 3)
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    d, i = cKDTree(r).query(q)
    return d, i


def accuracy(gt, rec):
    return nearest(gt, rec)[0].mean()


def completion(gt, rec):
    return nearest(rec, gt)[0].mean()


def completion_ratio(gt, rec, dist_th=0.05):
    return (nearest(rec, gt)[0] < dist_th).astype(np.float64).mean()


def face_areas(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)


def sample_surface(verts, faces, u):
    """-> (points float64 [n,3], face_idx [n], cdf [F], picks [n] = u0 * total)."""
    u = np.asarray(u, np.float64)
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    cdf = np.cumsum(face_areas(verts, faces))
    pick = u[:, 0] * cdf[-1]
    face = np.searchsorted(cdf, pick, side="left")
    r = u[:, 1:3].copy()
    r[r.sum(1) > 1.0] -= 1.0
    r = np.abs(r)
    t = tri[face]
    pts = t[:, 0] + r[:, 0:1] * (t[:, 1] - t[:, 0]) + r[:, 1:2] * (t[:, 2] - t[:, 0])
    return pts, face, cdf, pick


def sample_ambiguous(cdf, pick):
    """bool [n]: u0 * total within F 2^-52 total of a CDF entry (the order of a cumulative sum may decide those)."""
    tol = len(cdf) * 2.0 ** -52 * cdf[-1]
    j = np.clip(np.searchsorted(cdf, pick), 0, len(cdf) - 1)
    near = np.abs(cdf[j] - pick) <= tol
    near |= np.abs(cdf[np.maximum(j - 1, 0)] - pick) <= tol
    return near


def barycentric_min(verts, faces, pts, face):
    """The smallest barycentric coordinate of each point in its face (float64)."""
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)[face]]
    e1, e2, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], np.asarray(pts, np.float64) - tri[:, 0]
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    w1, w2 = (w * e1).sum(1), (w * e2).sum(1)
    den = d11 * d22 - d12 * d12
    a, b = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
    return np.minimum(np.minimum(a, b), 1.0 - a - b)


def world_to_camera(c2w, flip_yz=True):
    c = np.array(c2w, np.float64).reshape(-1, 4, 4)
    if flip_yz:
        c[:, :3, 1] *= -1.0
        c[:, :3, 2] *= -1.0
    return np.linalg.inv(c).astype(np.float32)


def check_proj(points, w2c, H, W, fx, fy, cx, cy):
    """float64 on the fp32 points and fp32 w2c [K,4,4] -> (seen [P] bool: some pose sees the point, near [P] bool: for some pose
    u, v or z' lies within a relative 1e-4 of a bound it is tested against)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    seen = np.zeros(len(p), bool)
    near = np.zeros(len(p), bool)
    for m in np.asarray(w2c, np.float32).astype(np.float64):
        cam = p @ m[:3, :3].T + m[:3, 3]
        x, z = -cam[:, 0], cam[:, 2] + 1e-5
        u = (fx * x + cx * cam[:, 2]) / z
        v = (fy * cam[:, 1] + cy * cam[:, 2]) / z
        seen |= (0 <= -z) & (u < W) & (u > 0) & (v < H) & (v > 0)
        near |= (np.abs(u) <= 1e-4 * W) | (np.abs(u - W) <= 1e-4 * W) | (np.abs(v) <= 1e-4 * H) | (np.abs(v - H) <= 1e-4 * H)
        near |= np.abs(z) <= 1e-4 * np.maximum(np.abs(cam[:, 2]), 1.0)
    return seen, near


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def plane(n_quads, z=0.0):
    """The unit square at height z as n x n quads of two triangles: (verts float32 [(n+1)^2, 3], faces int32 [2 n^2, 3])."""
    n = int(n_quads)
    ax = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(ax, ax, indexing="ij")
    v = np.stack((X.ravel(), Y.ravel(), np.full(X.size, float(z))), 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    f = np.concatenate((np.stack((a, a + n + 1, a + 1), 1), np.stack((a + 1, a + n + 1, a + n + 2), 1)))
    return v, f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def sphere(r=0.6, n=32):
    """mc_ref's marching-cubes sphere of radius r on an n^3 grid over [-1, 1]^3."""
    import mc_ref
    vol, o, sp, _ = mc_ref.sphere_field(n, r)
    v, f = mc_ref.marching_cubes(vol, 0.0, o, sp)
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def five_spheres():
    import mesh_cc_ref
    v, f = mesh_cc_ref.five_spheres()
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def plane_with_degenerate_faces():
    """plane(6) with zero-area faces mixed in: a repeated vertex, three collinear vertices, one at the front and one at the
    end of the list."""
    v, f = plane(6)
    deg = np.array([[0, 0, 1], [0, 1, 2], [8, 8, 8], [7, 14, 21]], np.int32)      # 0, 1, 2 and 7, 14, 21 are collinear
    f = np.concatenate((deg[:1], f[:10], deg[1:3], f[10:], deg[3:]))
    return v, f.astype(np.int32)


SAMPLING_CASES = {"sphere": (lambda: sphere(0.6, 32), 4001, 3), "five_spheres": (five_spheres, 3000, 4),
                  "degenerate_faces": (plane_with_degenerate_faces, 2500, 5)}


def sampling_case(name):
    """-> (verts, faces, u [n,3] float64)."""
    mesh, n, seed = SAMPLING_CASES[name]
    v, f = mesh()
    return v, f, np.random.default_rng(seed).random((n, 3))


# ---- the frustum case: a sphere seen from a handful of poses inside it -----------------------------------------------------
FRUSTUM_CAM = dict(H=68, W=120, fx=60.0, fy=60.0, cx=59.5, cy=33.5)


def frustum_poses(k=5, seed=11):
    """k camera-to-world matrices [k,4,4] float64: random rotations, centres within 0.2 of the origin."""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (k, 1, 1))
    for i in range(k):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1.0
        out[i, :3, :3] = q
        out[i, :3, 3] = rng.uniform(-0.2, 0.2, 3)
    return out


# ---- clouds for the nearest-point tests: name -> (ref float32 [M,3], query float32 [N,3]) ---------------------------------
def cloud_uniform(M=5000, N=5000, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((M, 3)).astype(np.float32), rng.random((N, 3)).astype(np.float32)


def cloud_clusters():
    """Two clusters of extent 0.01 that lie 100 extents apart; queries inside them, in the gap and 1000 box extents outside."""
    rng = np.random.default_rng(1)
    a = rng.random((700, 3)) * 0.01
    b = rng.random((600, 3)) * 0.01 + np.array([1.0, 0.3, -0.2])
    ref = np.concatenate((a, b)).astype(np.float32)
    inside = np.concatenate((rng.random((150, 3)) * 0.01, rng.random((150, 3)) * 0.01 + np.array([1.0, 0.3, -0.2])))
    gap = np.array([0.0, 0.0, 0.0]) + rng.random((200, 1)) * np.array([1.0, 0.3, -0.2]) + rng.normal(size=(200, 3)) * 0.02
    far = rng.normal(size=(100, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * 1000.0 + 0.5
    return ref, np.concatenate((inside, gap, far)).astype(np.float32)


def cloud_lattice():
    """The integer lattice {0..16}^3 padded with repeats of its own points to M = 17000: the kernel's grid over this cloud is
    32^3 cells of edge 0.5 (floor(cbrt(2 M)) = 32 cells per axis), so every lattice point sits on a cell boundary.  Queries: the
    lattice points (distance exactly 0) and cell centres."""
    ax = np.arange(17, dtype=np.float64)
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(2)
    ref = np.concatenate((lat, lat[rng.integers(0, len(lat), 17000 - len(lat))]))
    c = 0.25 + 0.5 * np.arange(32)
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(32 ** 3)[:3000]]
    return ref.astype(np.float32), np.concatenate((lat, centres)).astype(np.float32)


def cloud_single():
    rng = np.random.default_rng(3)
    return np.array([[0.25, -1.5, 3.0]], np.float32), (rng.normal(size=(300, 3)) * 4).astype(np.float32)


def cloud_identical():
    rng = np.random.default_rng(4)
    q = np.concatenate((rng.normal(size=(200, 3)), [[0.5, 0.5, 0.5]]))
    return np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (64, 1)), q.astype(np.float32)


def cloud_coplanar():
    rng = np.random.default_rng(5)
    ref = rng.random((1000, 3))
    ref[:, 2] = 0.375
    q = rng.random((600, 3)) * 1.4 - 0.2
    return ref.astype(np.float32), q.astype(np.float32)


def cloud_copies():
    rng = np.random.default_rng(6)
    ref = rng.normal(size=(3000, 3)).astype(np.float32)
    return ref, ref[rng.integers(0, 3000, 1500)].copy()


CLOUDS = {"uniform": cloud_uniform, "clusters": cloud_clusters, "lattice": cloud_lattice, "single": cloud_single,
          "identical": cloud_identical, "coplanar": cloud_coplanar, "copies": cloud_copies}
SIZES_N, SIZES_M = (1, 63, 65, 257), (1, 63, 65, 1000)
