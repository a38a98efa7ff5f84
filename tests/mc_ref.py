"""Vectorised numpy marching cubes with the table of tools/gen_mc_table.py: the test-side restatement of csrc/mesh.hip's
dns_mc_count / dns_mc_emit (the same vertex set, order and arithmetic; the same faces in the same order).

    vol [nx, ny, nz] float32, vol[i, j, k] at origin + (i, j, k) * spacing; a corner is inside iff v > level
    vertices: one per grid edge (p, axis) whose ends straddle the level, ordered by 3 * (C-order index of p) + axis, at
              p0 + t (p1 - p0), t = (level - v0) / (v1 - v0) in float32, positions in float64, stored as float32
    faces:    int32 [F, 3], ordered by cube, then table order
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TABLES = None


def tables():
    """(ntri [256], tri [256, 3 * MAX] edge ids (-1 padded), edge [12, 4] = start offset xyz + axis)."""
    global _TABLES
    if _TABLES is None:
        g = load_generator()
        t = g.build_table()
        m = max(len(r) for r in t)
        ntri = np.array([len(r) for r in t], np.int64)
        tri = np.full((256, 3 * m), -1, np.int64)
        for c, r in enumerate(t):
            flat = [e for tr in r for e in tr]
            tri[c, :len(flat)] = flat
        edge = np.array([list(g.corner_pos(g.edge_corners(e)[0])) + [e // 4] for e in range(12)], np.int64)
        _TABLES = ntri, tri, edge
    return _TABLES


def marching_cubes(vol, level, origin, spacing):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    N = vol.size
    lvl = np.float32(level)
    origin = np.asarray(origin, np.float64)
    spacing = np.asarray(spacing, np.float64)
    inside = vol > lvl
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1
    e = np.nonzero(flat)[0]
    p, a = e // 3, e % 3
    i, j, k = np.unravel_index(p, (nx, ny, nz))
    idx = np.stack((i, j, k), 1)
    step = np.eye(3, dtype=np.int64)[a]
    q = idx + step
    v0 = vol[i, j, k]
    v1 = vol[q[:, 0], q[:, 1], q[:, 2]]
    t = ((lvl - v0) / (v1 - v0)).astype(np.float32)
    p0 = origin + idx.astype(np.float64) * spacing
    p1 = origin + q.astype(np.float64) * spacing
    verts = (p0 + t.astype(np.float64)[:, None] * (p1 - p0)).astype(np.float32)

    ntri, tri, edge = tables()
    if min(nx, ny, nz) < 2 or len(e) == 0:
        return verts.reshape(-1, 3), np.zeros((0, 3), np.int32)
    ins = inside.astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] << c
    case = case.reshape(-1)
    m = tri.shape[1] // 3
    sel = np.arange(m)[None, :] < ntri[case][:, None]               # [cubes, MAX]: (cube, triangle) pairs in C order
    cube, tt = np.nonzero(sel)
    ci, cj, ck = np.unravel_index(cube, (nx - 1, ny - 1, nz - 1))
    ce = tri[case[cube][:, None], 3 * tt[:, None] + np.arange(3)[None, :]]   # [F, 3] cube edge ids
    off = edge[ce]                                                   # [F, 3, 4]
    gp = ((ci[:, None] + off[..., 0]) * ny + (cj[:, None] + off[..., 1])) * nz + (ck[:, None] + off[..., 2])
    faces = vid[3 * gp + off[..., 3]]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)


def check_manifold(faces):
    """(every undirected edge in exactly two faces, every directed edge exactly once)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    n = int(f.max()) + 1 if f.size else 1
    dk = d[:, 0] * n + d[:, 1]
    directed_once = np.unique(dk).size == dk.size
    u = np.sort(d, 1)
    _, cnt = np.unique(u[:, 0] * n + u[:, 1], return_counts=True)
    return bool((cnt == 2).all()), bool(directed_once)


def euler(verts, faces):
    f = np.asarray(faces, np.int64)
    d = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), 1)
    n_e = np.unique(d[:, 0] * (len(verts) + 1) + d[:, 1]).size
    n_v = np.unique(f).size
    return n_v - n_e + len(f)


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])


def area(verts, faces):
    return 0.5 * np.linalg.norm(face_normals(verts, faces), axis=1).sum()


# ---- analytic test fields: (vol, origin, spacing, gradient at world points) -----------------------------------------
def _grid(n, lo=-1.0, hi=1.0):
    n = (n,) * 3 if isinstance(n, int) else n
    ax = [np.linspace(lo, hi, m) for m in n]
    return np.meshgrid(*ax, indexing="ij"), (lo, lo, lo), [a[1] - a[0] for a in ax]


def sphere_field(n=64, r=0.6):
    (X, Y, Z), o, sp = _grid(n)
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), o, sp, lambda p: -p


def torus_field(n=(96, 80, 72), R=0.55, r=0.2):
    (X, Y, Z), o, sp = _grid(n)
    f = (r - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2)).astype(np.float32)

    def grad(p):
        q = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
        c = np.stack((p[:, 0] / q * R, p[:, 1] / q * R, np.zeros_like(q)), 1)
        return -(p - c)
    return f, o, sp, grad


def random_field(n=48, seed=0):
    rng = np.random.default_rng(seed)
    (X, Y, Z), o, sp = _grid(n)
    waves = [(rng.normal(size=3) * 3, rng.uniform(0, 6)) for _ in range(6)]
    f = sum(np.sin(k[0] * X + k[1] * Y + k[2] * Z + ph) for k, ph in waves)

    def grad(p):
        return sum(np.cos(p @ k + ph)[:, None] * k[None, :] for k, ph in waves)
    f = f.astype(np.float32)
    for sl in (np.s_[0], np.s_[-1]):                  # a -100 shell: the surface closes inside the grid
        f[sl] = -100
        f[:, sl] = -100
        f[:, :, sl] = -100
    return f, o, sp, grad


def read_ply(path):
    """Test-side reader of the binary little-endian PLY files Mesher writes -> (vertex record array, faces [F,3] int32)."""
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n"
        assert f.readline() == b"format binary_little_endian 1.0\n"
        elems, cur = [], None
        while True:
            line = f.readline().decode("ascii").strip()
            if line == "end_header":
                break
            w = line.split()
            if w[0] == "element":
                cur = [w[1], int(w[2]), []]
                elems.append(cur)
            elif w[0] == "property":
                cur[2].append(w[1:])
        body = f.read()
    (vn, V, vp), (fn, F, fp) = elems
    assert vn == "vertex" and fn == "face" and fp == [["list", "uchar", "int", "vertex_indices"]]
    vdt = np.dtype([(p[1], types[p[0]]) for p in vp])
    verts = np.frombuffer(body, vdt, V)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    fd = np.frombuffer(body, fdt, F, offset=V * vdt.itemsize)
    assert (fd["n"] == 3).all() and len(body) == V * vdt.itemsize + F * fdt.itemsize
    return verts, fd["i"].copy()
