"""Host reference of csrc/mesh_raster.hip (dns_rasterize_depth): numpy float64, brute force over pixels x triangles, plus the
small scenes the tests share.

The rule (include/dns_hip.h): camera space v = ((r0 x + r1 y) + r2 z) + t in fp32; ray d = ((j - cx) / fx, (i - cy) / fy, 1);
per edge, vertices ordered by index a < b, c = v_a x v_b with the winding's sign, E = (d.x c.x + d.y c.y) + c.z; covered iff all
E >= 0 or all E <= 0; depth t = (n . v0) / (n . d), n = (v1 - v0) x (v2 - v0); accepted iff z_near <= t <= z_far; the pixel is
the minimum.  ``camera_vertices_f32`` evaluates the transform in numpy float32 in the kernel's order (the kernel is compiled
without contraction, so its camera-space vertices are these bits); everything after it starts from those fp32 values, in float64.

``render`` returns per view three images: D (the rule in float64), D_grown (edge tests loosened to E >= -m: depth <= D) and
D_shrunk (tightened to E >= +m: depth >= D), background = +inf.  The per-edge margin is m = 16 u |v_a| |v_b| |d|, u = 2^-24, which
bounds the fp32 rounding of E: a component of c is two rounded products and a rounded difference, |dc_k| <= u (|p1| + |p2|) +
u |c_k| <= 2 u |v_a| |v_b| (Cauchy-Schwarz on the two-component sub-vectors); d.x and d.y carry two roundings each (the
difference and the quotient), 2 u relative; the three-term dot adds two products and two sums, at most 3 u (|d.x c.x| + |d.y c.y|
+ |c.z|).  With |d.x| + |d.y| + 1 <= sqrt(3) |d| and |c| <= |v_a| |v_b| the sum is (2 sqrt(3) + 2 + 3 sqrt(3)) u |v_a| |v_b| |d| <
10.7 u |v_a| |v_b| |d|, under 16 u.  The z_near / z_far comparisons are loosened / tightened by a relative 2^-20.

A pixel is unambiguous when the three images select the same triangle (or all three are background) and that triangle is not
grazing there: |n . d| >= 0.05 |n| |d|.

``render_f32`` restates the whole rule in numpy float32 in the kernel's order of operations (no boxes and no culling: they never
change a pixel).  DEPTH_RTOL comes from it, never from the kernel.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
EDGE_MARGIN = 16.0 * U
Z_RTOL = 2.0 ** -20
GRAZING = 0.05
# The worst relative difference of render_f32 from D over the unambiguous pixels of all SCENES (tests/test_raster_ref.py
# measures it again and holds it to this figure).  DEPTH_RTOL is four times it: the factor covers the device's division, which
# need not be correctly rounded, and nothing else.
DEPTH_ERR_MEASURED = 3.7e-7               # 3.656e-07, a pixel of the soup
DEPTH_RTOL = 4.0 * DEPTH_ERR_MEASURED
_CHUNK = 256


def camera_vertices_f32(verts, w2c):
    """verts [P,3], w2c [4,4] -> float32 [P,3]: ((r0 x + r1 y) + r2 z) + t per row, every operation rounded to fp32."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    m = np.asarray(w2c, np.float32).reshape(4, 4)
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3]
    return out


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def _rays(H, W, fx, fy, cx, cy, dt):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dx = (j.ravel().astype(dt) - dt(cx)) / dt(fx)
    dy = (i.ravel().astype(dt) - dt(cy)) / dt(fy)
    return dx, dy


def _triangles(verts, faces, w2c, dt):
    """-> (tri [F,3,3] camera space in dt, usable [F]: finite in world and camera space, ids [F,3])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    w = np.asarray(verts, np.float32).reshape(-1, 3)
    vc = camera_vertices_f32(w, w2c)
    ok = (np.isfinite(w).all(1) & np.isfinite(vc).all(1))[f].all(1) if len(f) else np.zeros(0, bool)
    return vc.astype(dt)[f], ok, f


def _edges(tri, ids):
    """Signed edge vectors c [F,3,3] (edge k = vertices k, k+1) and |v_a| |v_b| [F,3]."""
    cs, mags = [], []
    for k in range(3):
        a, b = tri[:, k], tri[:, (k + 1) % 3]
        swap = ids[:, k] > ids[:, (k + 1) % 3]
        lo = np.where(swap[:, None], b, a)
        hi = np.where(swap[:, None], a, b)
        c = _cross(lo, hi)
        cs.append(np.where(swap[:, None], -c, c))
        mags.append(np.sqrt((a.astype(np.float64) ** 2).sum(1) * (b.astype(np.float64) ** 2).sum(1)))
    return np.stack(cs, 1), np.stack(mags, 1)


def _merge(best, arg, t, base):
    k = t.argmin(0)
    v = t[k, np.arange(t.shape[1])]
    upd = v < best
    best[upd] = v[upd]
    arg[upd] = k[upd] + base


def render_view(verts, faces, w2c, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0):
    """One view -> dict of [H,W] arrays: D, D_grown, D_shrunk (float64, +inf background), tri (the triangle D selects, -1 for
    background), unambiguous (bool)."""
    dt = np.float64
    intr = [float(np.float32(x)) for x in (fx, fy, cx, cy)]
    zn, zf = float(np.float32(z_near)), float(np.float32(z_far))
    dx, dy = _rays(H, W, *intr, dt)
    dn = np.sqrt(dx * dx + dy * dy + 1.0)
    tri, ok, ids = _triangles(verts, faces, w2c, dt)
    N = H * W
    best = [np.full(N, np.inf) for _ in range(3)]
    arg = [np.full(N, -1, np.int64) for _ in range(3)]
    graze = [np.zeros(N, bool) for _ in range(3)]
    with np.errstate(all="ignore"):
        for lo in range(0, len(tri), _CHUNK):
            t3, good, id3 = tri[lo:lo + _CHUNK], ok[lo:lo + _CHUNK], ids[lo:lo + _CHUNK]
            t3 = np.where(good[:, None, None], t3, 0.0)
            c, mag = _edges(t3, id3)
            n = _cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
            good = good & (n != 0.0).any(1)
            num = (n[:, 0] * t3[:, 0, 0] + n[:, 1] * t3[:, 0, 1]) + n[:, 2] * t3[:, 0, 2]
            den = (n[:, 0:1] * dx + n[:, 1:2] * dy) + n[:, 2:3]
            t = num[:, None] / den
            E = [(dx * c[:, k, 0:1] + dy * c[:, k, 1:2]) + c[:, k, 2:3] for k in range(3)]
            m = [EDGE_MARGIN * mag[:, k:k + 1] * dn for k in range(3)]
            gz = np.abs(den) < GRAZING * np.sqrt((n * n).sum(1))[:, None] * dn
            covers = (
                ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)),
                ((E[0] >= -m[0]) & (E[1] >= -m[1]) & (E[2] >= -m[2])) | ((E[0] <= m[0]) & (E[1] <= m[1]) & (E[2] <= m[2])),
                ((E[0] >= m[0]) & (E[1] >= m[1]) & (E[2] >= m[2])) | ((E[0] <= -m[0]) & (E[1] <= -m[1]) & (E[2] <= -m[2])))
            zs = ((t >= zn) & (t <= zf), (t >= zn * (1 - Z_RTOL)) & (t <= zf * (1 + Z_RTOL)),
                  (t >= zn * (1 + Z_RTOL)) & (t <= zf * (1 - Z_RTOL)))
            for q in range(3):
                tq = np.where(covers[q] & zs[q] & good[:, None], t, np.inf)
                before = arg[q].copy()
                _merge(best[q], arg[q], tq, lo)
                ch = arg[q] != before
                graze[q][ch] = gz[arg[q][ch] - lo, np.nonzero(ch)[0]]
    same = (arg[0] == arg[1]) & (arg[0] == arg[2])
    return {"D": best[0].reshape(H, W), "D_grown": best[1].reshape(H, W), "D_shrunk": best[2].reshape(H, W),
            "tri": arg[0].reshape(H, W), "unambiguous": (same & ~graze[0]).reshape(H, W)}


def render_view_f32(verts, faces, w2c, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0):
    """The kernel's arithmetic in numpy float32, operation by operation -> depth [H,W] float32 (+inf background)."""
    dt = np.float32
    dx, dy = _rays(H, W, fx, fy, cx, cy, dt)
    zn, zf = dt(z_near), dt(z_far)
    tri, ok, ids = _triangles(verts, faces, w2c, dt)
    best = np.full(H * W, np.inf, dt)
    with np.errstate(all="ignore"):
        for lo in range(0, len(tri), _CHUNK):
            t3, good, id3 = tri[lo:lo + _CHUNK], ok[lo:lo + _CHUNK], ids[lo:lo + _CHUNK]
            t3 = np.where(good[:, None, None], t3, dt(0))
            c, _ = _edges(t3, id3)
            n = _cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
            good = good & (n != 0).any(1)
            num = (n[:, 0] * t3[:, 0, 0] + n[:, 1] * t3[:, 0, 1]) + n[:, 2] * t3[:, 0, 2]
            den = (n[:, 0:1] * dx + n[:, 1:2] * dy) + n[:, 2:3]
            t = num[:, None] / den
            E = [(dx * c[:, k, 0:1] + dy * c[:, k, 1:2]) + c[:, k, 2:3] for k in range(3)]
            cover = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
            tq = np.where(cover & (t >= zn) & (t <= zf) & good[:, None], t, dt(np.inf))
            assert tq.dtype == np.float32
            best = np.minimum(best, tq.min(0))
    return best.reshape(H, W)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose(axis=(0, 1, 0), deg=0.0, centre=(0, 0, 0)):
    """Camera-to-world [4,4] float64: rotation about ``axis`` by ``deg``, camera centre ``centre``."""
    m = np.eye(4)
    m[:3, :3] = _rot(axis, deg)
    m[:3, 3] = centre
    return m


def w2c_f32(c2w):
    return np.linalg.inv(np.asarray(c2w, np.float64).reshape(-1, 4, 4)).astype(np.float32)


ROOM_LO, ROOM_HI = np.array([-1.5, -1.0, -1.25]), np.array([2.0, 1.3125, 2.5])


def box_mesh(lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]],
                 np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 4, 5], [0, 5, 1], [1, 5, 6], [1, 6, 2], [2, 6, 7], [2, 7, 3],
                  [3, 7, 4], [3, 4, 0]], np.int32)
    return v, f


def uv_sphere(radius, centre, n_lat=50, n_lon=50):
    """A latitude / longitude sphere: 2 n_lon (n_lat - 1) triangles."""
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.stack((np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.full_like(ph, np.cos(t))), 1) for t in th])
    v = np.concatenate(([[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]])) * radius + np.asarray(centre, np.float64)
    f = []
    idx = lambda r, k: 1 + r * n_lon + k % n_lon
    for k in range(n_lon):
        f.append([0, idx(0, k), idx(0, k + 1)])
        f.append([len(v) - 1, idx(n_lat - 2, k + 1), idx(n_lat - 2, k)])
    for r in range(n_lat - 2):
        for k in range(n_lon):
            f.append([idx(r, k), idx(r + 1, k), idx(r + 1, k + 1)])
            f.append([idx(r, k), idx(r + 1, k + 1), idx(r, k + 1)])
    return v.astype(np.float32), np.array(f, np.int32)


LATTICE = dict(j0=30, i0=25, nx=24, ny=16, z=2.0)


def lattice_mesh(z=2.0, cam=None):
    """A planar grid of 2 x (24 x 16) triangles at depth z facing the camera; with fx = fy = 32 and z = 2 the spacing 1/16 puts
    every vertex exactly on a pixel centre (all coordinates are small dyadic numbers: every product of the rule is exact)."""
    cam = SCENE_CAMS["lattice"] if cam is None else cam
    L = LATTICE
    j = np.arange(L["j0"], L["j0"] + L["nx"] + 1)
    i = np.arange(L["i0"], L["i0"] + L["ny"] + 1)
    X, Y = np.meshgrid((j - cam["cx"]) / cam["fx"] * 2.0, (i - cam["cy"]) / cam["fy"] * 2.0, indexing="xy")    # [ny+1, nx+1]
    v = np.stack((X.ravel(), Y.ravel(), np.full(X.size, z)), 1).astype(np.float32)
    a = (np.arange(L["ny"])[:, None] * (L["nx"] + 1) + np.arange(L["nx"])[None, :]).ravel()
    s = L["nx"] + 1
    f = np.concatenate((np.stack((a, a + 1, a + s + 1), 1), np.stack((a, a + s + 1, a + s), 1)))
    return v, f.astype(np.int32)


SOUP_CENTRES = ((0.0, 0.0, 0.0), (0.1, 0.0, -0.1), (0.0, 0.2, 0.1))     # the camera centres of the soup's views
SOUP_MIN_COS = 0.06


def _soup_group(rng, n, dist, size):
    """n random triangles: centres at a distance drawn from ``dist`` in a random direction, vertices spread by ``size``.  A
    candidate whose plane passes one of SOUP_CENTRES at less than SOUP_MIN_COS of its farthest vertex is drawn again: from such a
    centre every ray meets it at a cosine under that, where t = (n . v0) / (n . d) loses 1 / cosine of its fp32 digits -- the
    grazing pixels the sphere's silhouette supplies in moderation would dominate the scene."""
    out = []
    while len(out) < n:
        d = rng.normal(size=3)
        c = d / np.linalg.norm(d) * rng.uniform(*dist)
        t = c + rng.normal(size=(3, 3)) * rng.uniform(*size)
        nrm = np.cross(t[1] - t[0], t[2] - t[0])
        nrm /= np.linalg.norm(nrm)
        if all(abs(nrm @ (t[0] - np.array(o))) >= SOUP_MIN_COS * np.linalg.norm(t - np.array(o), axis=1).max() for o in SOUP_CENTRES):
            out.append(t)
    return np.stack(out)


def soup_mesh(seed=7):
    """2000 random triangles of mixed size round the camera: some cross z_near, some lie beyond z_far, with zero-area ones
    (a repeated vertex) and exact duplicates."""
    rng = np.random.default_rng(seed)
    tri = np.concatenate((_soup_group(rng, 900, (0.3, 6.0), (0.02, 0.3)), _soup_group(rng, 600, (0.3, 6.0), (0.3, 3.0)),
                          _soup_group(rng, 150, (0.02, 0.3), (0.02, 0.3)), _soup_group(rng, 250, (15.0, 30.0), (0.5, 8.0))))
    n = len(tri)
    v = tri.reshape(-1, 3)
    f = np.arange(3 * n).reshape(n, 3)
    zero = f[rng.integers(0, n, 50)].copy()
    zero[:, 2] = zero[:, 0]                                       # a repeated vertex: n = 0 exactly
    dup = f[rng.integers(0, n, 50)].copy()
    f = np.concatenate((f, zero, dup))
    return v.astype(np.float32), f[rng.permutation(len(f))].astype(np.int32)


SCENE_CAMS = {
    "room": dict(H=37, W=50, fx=30.0, fy=30.0, cx=24.5, cy=18.0),
    "sphere": dict(H=48, W=64, fx=60.0, fy=60.0, cx=31.5, cy=23.5),
    "lattice": dict(H=80, W=96, fx=32.0, fy=32.0, cx=47.5, cy=39.5),
    "soup": dict(H=60, W=80, fx=50.0, fy=55.0, cx=39.5, cy=29.5),
    "behind": dict(H=24, W=32, fx=30.0, fy=30.0, cx=15.5, cy=11.5),
    "empty": dict(H=24, W=32, fx=30.0, fy=30.0, cx=15.5, cy=11.5),
}
SCENES = tuple(SCENE_CAMS)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (verts float32 [P,3], faces int32 [F,3], w2c float32 [V,4,4], cam dict)."""
    cam = SCENE_CAMS[name]
    if name == "room":
        v, f = box_mesh(ROOM_LO, ROOM_HI)
        c2w = [pose(), pose((0.3, 1.0, 0.2), 75.0, (0.4, -0.2, 0.6)), pose((1.0, 0.2, -0.4), 160.0, (-0.7, 0.5, 1.1))]
    elif name == "sphere":
        v, f = uv_sphere(0.5, (0.1, -0.05, 3.0))
        c2w = [pose(), pose((0, 1, 0), 25.0, (-1.2, 0.1, 0.3)), pose((1.0, 0.5, 0.0), -20.0, (0.3, -1.0, 0.2))]
    elif name == "lattice":
        v, f = lattice_mesh()
        c2w = [pose(), pose(centre=(0.25 / 16, 0.375 / 16, 0.0))]
    elif name == "soup":
        v, f = soup_mesh()
        c2w = [pose(), pose((0.2, 1.0, 0.1), 130.0, SOUP_CENTRES[1]), pose((1.0, 0.0, 0.3), -70.0, SOUP_CENTRES[2])]
    elif name == "behind":
        v, f = uv_sphere(0.5, (0.0, 0.0, -3.0), 8, 10)
        c2w = [pose(), pose((0, 1, 0), 10.0)]
    elif name == "empty":
        v, f = np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)
        c2w = [pose(), pose((0, 1, 0), 10.0)]
    else:
        raise KeyError(name)
    return v, f, w2c_f32(np.stack(c2w)), cam


def _cam_args(cam):
    return cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]


@functools.lru_cache(maxsize=None)
def render(name, z_near=0.01, z_far=20.0):
    """The reference images of a scene: dict of [V,H,W] arrays (D, D_grown, D_shrunk, tri, unambiguous), computed once."""
    v, f, w2c, cam = scene(name)
    views = [render_view(v, f, m, *_cam_args(cam), z_near, z_far) for m in w2c]
    return {k: np.stack([r[k] for r in views]) for k in views[0]}


@functools.lru_cache(maxsize=None)
def render_f32(name, z_near=0.01, z_far=20.0):
    v, f, w2c, cam = scene(name)
    return np.stack([render_view_f32(v, f, m, *_cam_args(cam), z_near, z_far) for m in w2c])


def room_depth_analytic(w2c, cam):
    """Ray-box exit distance of the room seen from inside, as camera-space z [H,W] (float64, from the fp32 pose)."""
    m = np.asarray(w2c, np.float32).astype(np.float64)
    R, t = m[:3, :3], m[:3, 3]
    o = -R.T @ t
    H, W = cam["H"], cam["W"]
    dx, dy = _rays(H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], np.float64)
    w = np.stack((dx, dy, np.ones_like(dx)), 1) @ R                # world direction of each ray: R^T d
    with np.errstate(all="ignore"):
        far = np.where(w > 0, (ROOM_HI - o) / w, np.where(w < 0, (ROOM_LO - o) / w, np.inf))
    return far.min(1).reshape(H, W)
