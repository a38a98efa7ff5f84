"""Host reference of csrc/mesh_render.hip (dns_render_mesh): numpy float64, brute force over pixels x triangles and over the
points, with the bounds inside which a correct fp32 evaluation of the rule must lie.  It starts, like tests/raster_ref.py, from
``raster_ref.camera_vertices_f32`` (the kernel is compiled without contraction: its camera-space vertices and points are those
bits) and evaluates everything after that in float64.  u = 2^-24; bounds are first-order in u, and every constant below is
rounded up from the count to absorb the higher orders.

The rule (include/dns_hip.h).  Coverage, depth, z_near / z_far and the skipped triangles are raster_ref's.  Per pixel the winner
is the minimum of (depth, id): faces by their index, then points; a face is kept under cull="back" iff num < 0 and under
cull="front" iff num > 0, num = n . v0.  Face pixel: S = (E0 + E1) + E2, weights w0 = E1 / S, w1 = E2 / S, w2 = E0 / S, colour =
(w0 c0 + w1 c1) + w2 c2; shade="headlight" multiplies by L = ambient + (1 - ambient) |den| / (|n| |d|), den = n . d.  Point: p in
camera space, accepted iff z_near <= p.z <= z_far, a = fx (p.x / p.z) + cx - s/2, b = fy (p.y / p.z) + cy - s/2, columns ceil(a)
.. ceil(a) + s - 1, rows ceil(b) .. ceil(b) + s - 1.

Facing rule.  e1 = v1 - v0, e2 = v2 - v0 are one rounding each (u |e| per component); a component of n = e1 x e2 is two products
of such numbers (3 u each) and a rounded difference: |dn_k| <= 4 u (|p1| + |p2|) <= 4 u |e1| |e2| (Cauchy-Schwarz on the
two-component sub-vectors).  num = (n.x v0.x + n.y v0.y) + n.z v0.z: from dn at most 4 u |e1| |e2| (|v0.x| + |v0.y| + |v0.z|) <=
4 sqrt(3) u |e1| |e2| |v0|, from the two products and two sums of the dot 3 u sum |n_k v0_k| <= 3 u |e1| |e2| |v0|: together
9.93 u, under NUM_MARGIN = 16 u |e1| |e2| |v0|.  A face with |num| <= that is UNCERTAIN-FACING: the kernel may see either sign.
den = (n.x d.x + n.y d.y) + n.z likewise: 4 sqrt(3) u from dn (|d.x| + |d.y| + 1 <= sqrt(3) |d|), 2 u |n| |d| from the two
roundings d.x and d.y carry, 3 u |n| |d| from the dot: 11.93 u, under DEN_MARGIN = 16 u |e1| |e2| |d|.

Pixel ambiguity, faces.  A pixel is compared only when it is unambiguous: (1) as in raster_ref -- the rule and its grown and
shrunk coverage (edge margin m_k = EDGE_MARGIN |v_a| |v_b| |d|) select the same face or all the background, and the face is not
grazing; (2) under a culling mode, no uncertain-facing face passes the grown coverage test there; (3) no other face that passes
the grown tests can come out nearer in fp32: with the depth error terr = t (NUM_MARGIN / |num| + DEN_MARGIN / |den| + 2 u) of
t = num / den (the quotient's own rounding is the 2 u), a face f' with t' - terr' <= t + terr makes the pixel ambiguous --
except a face with the winner's three vertex indices in the winner's order, which evaluates the same fp32 numbers and loses or
wins by its index alone (the reference picks the lower index, as the kernel must); (4) the colour bound below is finite.

Colour bound.  The fp32 edge functions differ from E_k by at most m_k (raster_ref's derivation), S by at most M = m0 + m1 + m2
plus its two sums, 2 u sum |E_k|.  With w_k = E_k' / S: the computed weight differs by (a_k' S - E_k' dS) / (S S^), |a_k'| <=
m_k', which for weights in [0, 1] (every compared pixel passes the shrunk test: all E_k of one sign) is at most
WB = (M + 2 u sum |E_k|) / (|S| - M - 2 u sum |E_k|), plus u for the quotient: the issue's "sum of the three margins over |den|".
Per channel |colour error| <= (WB + u) sum_k |c_k| + 3 u sum_k |w_k c_k| (three products, two sums).
Shading factor: the cosine |den| / (sqrt(nn) sqrt(dd)) carries DEN_MARGIN / |den| from den, 4 sqrt(3) u |e1| |e2| / |n| from dn
in |n| (d(|n|^2) = 2 n . dn), 1.5 u + 3.5 u from the dots under the roots (dd's terms carry 2 u each from d.x, d.y), and one
rounding each for the two roots, the product and the quotient -- 2 u allowed for each root and the quotient, the device's need
not be correctly rounded: 12 u, taken as 16 u.  L = ambient + (1 - ambient) cosine adds three roundings: |dL| <= (1 - ambient)
cosine (DEN_MARGIN / |den| + 4 sqrt(3) u |e1| |e2| / |n| + 16 u) + 3 u L.  Shaded colour: |d(colour L)| <= |dcolour| L +
|colour| |dL| + u |colour| L, with |colour| taken as sum_k |w_k c_k|.

Pixel ambiguity, points.  p, and so the z tests and the key depth, are exact (the same fp32 bits on both sides).  a is a
quotient, a product, a sum and a difference: |da| <= u (2 A + (A + C) + (A + C + h)) <= 4 u (A + C + h), A = |fx p.x / p.z|,
C = |cx|, h = s / 2: POINT_MARGIN.  Where a - margin and a + margin have different ceilings the square may start at either column:
the columns only one of the two squares holds are ambiguous for that point (rows likewise): the "grown" square is the union,
the "shrunk" one the intersection, and a pixel is ambiguous when the three images select differently.  A pixel of a point's grown
square is also ambiguous when the face layer under it is ambiguous, or within Z_RTOL of the point's depth (relative:
D_grown (1 - Z_RTOL) <= p.z <= D_shrunk (1 + Z_RTOL)), unless a point of the shrunk image lies clearly in front of all of that.
Between two points the comparison is exact (depth, then index) and nothing is ambiguous.

``render_view_f32`` restates the kernel in numpy float32, operation by operation; tests/test_mesh_render_ref.py holds it, and
deliberately wrong variants of it, to the bounds.  No tolerance here comes from the kernel under test.
"""
from __future__ import annotations

import functools

import numpy as np

import raster_ref as R

U = R.U
NUM_MARGIN = 16.0 * U
DEN_MARGIN = 16.0 * U
COS_ROUNDINGS = 16.0 * U
POINT_MARGIN = 4.0 * U
CULLS = (None, "back", "front")
SHADES = (None, "headlight")
_CHUNK = 256
_SQ3 = np.sqrt(3.0)


def _norm(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).sum(-1))


def _face_data(verts, faces, w2c):
    """Per-face float64 quantities of one view, from the fp32 camera-space vertices."""
    tri, ok, ids = R._triangles(verts, faces, w2c, np.float64)
    tri = np.where(ok[:, None, None], tri, 0.0)
    c, mag = R._edges(tri, ids) if len(tri) else (np.zeros((0, 3, 3)), np.zeros((0, 3)))
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = R._cross(e1, e2)
    good = ok & (n != 0.0).any(1)
    num = (n[:, 0] * tri[:, 0, 0] + n[:, 1] * tri[:, 0, 1]) + n[:, 2] * tri[:, 0, 2]
    ee = _norm(e1) * _norm(e2)
    canon = np.zeros(len(ids), np.int64)
    if len(ids):
        _, first, inv = np.unique(ids, axis=0, return_index=True, return_inverse=True)
        order = np.full(len(first), len(ids), np.int64)
        np.minimum.at(order, inv.ravel(), np.arange(len(ids)))
        canon = order[inv.ravel()]
    return dict(tri=tri, ids=ids, c=c, mag=mag, n=n, nn=_norm(n), num=num, ee=ee, good=good, canon=canon,
                num_margin=NUM_MARGIN * ee * _norm(tri[:, 0]))


def keep_mask(fd, cull):
    """The faces the float64 rule draws under ``cull`` and the uncertain-facing ones."""
    if cull is None:
        return fd["good"].copy(), np.zeros(len(fd["good"]), bool)
    keep = fd["good"] & ((fd["num"] < 0.0) if cull == "back" else (fd["num"] > 0.0))
    return keep, fd["good"] & (np.abs(fd["num"]) <= fd["num_margin"])


def _chunks(fd, dx, dy, dn, zn, zf):
    """Per chunk of faces: (lo, hi, t, covers[3], zs[3], grazing, terr), arrays [faces of the chunk, pixels]."""
    with np.errstate(all="ignore"):
        for lo in range(0, len(fd["tri"]), _CHUNK):
            s = slice(lo, lo + _CHUNK)
            c, mag, n, num = fd["c"][s], fd["mag"][s], fd["n"][s], fd["num"][s]
            den = (n[:, 0:1] * dx + n[:, 1:2] * dy) + n[:, 2:3]
            t = num[:, None] / den
            E = [(dx * c[:, k, 0:1] + dy * c[:, k, 1:2]) + c[:, k, 2:3] for k in range(3)]
            m = [R.EDGE_MARGIN * mag[:, k:k + 1] * dn for k in range(3)]
            gz = np.abs(den) < R.GRAZING * fd["nn"][s][:, None] * dn
            covers = (
                ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)),
                ((E[0] >= -m[0]) & (E[1] >= -m[1]) & (E[2] >= -m[2])) | ((E[0] <= m[0]) & (E[1] <= m[1]) & (E[2] <= m[2])),
                ((E[0] >= m[0]) & (E[1] >= m[1]) & (E[2] >= m[2])) | ((E[0] <= -m[0]) & (E[1] <= -m[1]) & (E[2] <= -m[2])))
            zs = ((t >= zn) & (t <= zf), (t >= zn * (1 - R.Z_RTOL)) & (t <= zf * (1 + R.Z_RTOL)),
                  (t >= zn * (1 + R.Z_RTOL)) & (t <= zf * (1 - R.Z_RTOL)))
            terr = np.abs(t) * (fd["num_margin"][s][:, None] / np.abs(num)[:, None]
                                + DEN_MARGIN * fd["ee"][s][:, None] * dn / np.abs(den) + 2.0 * U)
            yield lo, min(lo + _CHUNK, len(fd["tri"])), t, covers, zs, gz, terr


def _merge(best, arg, aux, t, base, extra):
    """min over the chunk's faces (the first of equal minima: the lowest index), merged with strict <."""
    k = t.argmin(0)
    cols = np.arange(t.shape[1])
    v = t[k, cols]
    upd = v < best
    best[upd] = v[upd]
    arg[upd] = k[upd] + base
    for a, e in zip(aux, extra):
        a[upd] = e[k[upd], cols[upd]]


def _face_layer(fd, culls, H, W, intr, zn, zf):
    """-> {cull: dict(D, Dg, Ds [N] float64 (+inf background), tri [N], unamb [N] bool, terr [N])} for one view."""
    dx, dy = R._rays(H, W, *intr, np.float64)
    dn = np.sqrt(dx * dx + dy * dy + 1.0)
    N = H * W
    st = {}
    for cull in culls:
        keep, unc = keep_mask(fd, cull)
        st[cull] = dict(keep=keep, unc=unc, best=[np.full(N, np.inf) for _ in range(3)], arg=[np.full(N, -1, np.int64) for _ in range(3)],
                        graze=np.zeros(N, bool), terr=np.zeros(N), unc_hit=np.zeros(N, bool), rival=np.full(N, np.inf))
    for lo, hi, t, covers, zs, gz, terr in _chunks(fd, dx, dy, dn, zn, zf):
        for cull in culls:
            s = st[cull]
            kp = s["keep"][lo:hi, None]
            for q in range(3):
                tq = np.where(covers[q] & zs[q] & kp, t, np.inf)
                _merge(s["best"][q], s["arg"][q], (s["graze"], s["terr"]) if q == 0 else (), tq, lo, (gz, terr) if q == 0 else ())
            if s["unc"][lo:hi].any():
                s["unc_hit"] |= (covers[1] & s["unc"][lo:hi, None]).any(0)
    # the nearest a rival (another face that passes the grown tests, not a copy of the winner) can come out in fp32
    for lo, hi, t, covers, zs, gz, terr in _chunks(fd, dx, dy, dn, zn, zf):
        for cull in culls:
            s = st[cull]
            win = s["arg"][0]
            wc = np.where(win >= 0, fd["canon"][np.maximum(win, 0)], -1)
            other = fd["canon"][lo:hi, None] != wc[None, :]
            lb = np.where(covers[1] & zs[1] & s["keep"][lo:hi, None] & other, t - terr, np.inf)
            s["rival"] = np.minimum(s["rival"], lb.min(0))
    out = {}
    for cull in culls:
        s = st[cull]
        same = (s["arg"][0] == s["arg"][1]) & (s["arg"][0] == s["arg"][2])
        hit = s["arg"][0] >= 0
        tie = hit & (s["rival"] <= s["best"][0] + s["terr"])
        out[cull] = dict(D=s["best"][0], Dg=s["best"][1], Ds=s["best"][2], tri=s["arg"][0],
                         unamb=same & ~s["graze"] & ~s["unc_hit"] & ~tie, plain=same & ~s["graze"])
    return out, (dx, dy, dn)


def _shade(fd, colors, tri, rays, ambient):
    """Colours and bounds of the face pixels: tri [N] (the winner, -1 elsewhere) -> {shade: (color [N,3], bound [N,3])}."""
    dx, dy, dn = rays
    N = len(tri)
    hit = tri >= 0
    f = np.maximum(tri, 0)
    col = np.zeros((N, 3))
    bnd = np.zeros((N, 3))
    out = {s: (col.copy(), bnd.copy()) for s in SHADES}
    if not hit.any():
        return out
    with np.errstate(all="ignore"):
        c, mag, n = fd["c"][f], fd["mag"][f], fd["n"][f]
        E = [(dx * c[:, k, 0] + dy * c[:, k, 1]) + c[:, k, 2] for k in range(3)]
        m = [R.EDGE_MARGIN * mag[:, k] * dn for k in range(3)]
        S = (E[0] + E[1]) + E[2]
        sE = np.abs(E[0]) + np.abs(E[1]) + np.abs(E[2])
        dS = (m[0] + m[1] + m[2]) + 2.0 * U * sE
        room = np.abs(S) - dS
        wb = np.where(room > 0, dS / room, np.inf) + U
        w = [E[1] / S, E[2] / S, E[0] / S]
        cv = [np.asarray(colors, np.float32).astype(np.float64)[fd["ids"][f, k]] for k in range(3)]
        plain = (w[0][:, None] * cv[0] + w[1][:, None] * cv[1]) + w[2][:, None] * cv[2]
        sabs = np.abs(cv[0]) + np.abs(cv[1]) + np.abs(cv[2])
        swc = np.abs(w[0][:, None] * cv[0]) + np.abs(w[1][:, None] * cv[1]) + np.abs(w[2][:, None] * cv[2])
        b_plain = wb[:, None] * sabs + 3.0 * U * swc
        den = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
        nn = fd["nn"][f]
        cosv = np.abs(den) / (nn * dn)
        rel = DEN_MARGIN * fd["ee"][f] * dn / np.abs(den) + 4.0 * _SQ3 * U * fd["ee"][f] / nn + COS_ROUNDINGS
        a = float(np.float32(ambient))
        L = a + (1.0 - a) * cosv
        dL = (1.0 - a) * cosv * rel + 3.0 * U * L
        lit = plain * L[:, None]
        b_lit = b_plain * L[:, None] + swc * dL[:, None] + U * swc * L[:, None]
    for s, (cc, bb) in ((None, (plain, b_plain)), ("headlight", (lit, b_lit))):
        out[s][0][hit] = cc[hit]
        out[s][1][hit] = np.where(np.isfinite(bb[hit]), bb[hit], np.inf)
    return out


def point_squares(points, w2c, H, W, intr, zn, zf, size):
    """Per accepted point: (index, z, (j0, i0) by the rule, column range pair (lo, hi) of the first column, row range pair)."""
    fx, fy, cx, cy = intr
    pw = np.asarray(points, np.float32).reshape(-1, 3)
    pc = R.camera_vertices_f32(pw, w2c).astype(np.float64)
    fin = np.isfinite(pw).all(1) & np.isfinite(pc).all(1)
    h = size * 0.5
    out = []
    with np.errstate(all="ignore"):
        for k in np.nonzero(fin & (pc[:, 2] >= zn) & (pc[:, 2] <= zf))[0]:
            x, y, z = pc[k]
            A, B = fx * (x / z), fy * (y / z)
            a, b = A + cx - h, B + cy - h
            ma, mb = POINT_MARGIN * (abs(A) + abs(cx) + h), POINT_MARGIN * (abs(B) + abs(cy) + h)
            if not (np.isfinite(a) and np.isfinite(b)) or max(abs(a), abs(b)) > 1e9:
                continue
            out.append((int(k), float(z), (int(np.ceil(a)), int(np.ceil(b))),
                        (int(np.ceil(a - ma)), int(np.ceil(a + ma))), (int(np.ceil(b - mb)), int(np.ceil(b + mb)))))
    return out, ~fin


def _paint(best, ident, H, W, z, k, j0, j1, i0, i1):
    """Point k at depth z over the columns j0..j1 and rows i0..i1 (inclusive, clipped here) of the key images best / ident [H,W]:
    ident holds the face index, or -2 - point."""
    j0, j1, i0, i1 = max(j0, 0), min(j1, W - 1), max(i0, 0), min(i1, H - 1)
    if j0 > j1 or i0 > i1:
        return
    b, d = best[i0:i1 + 1, j0:j1 + 1], ident[i0:i1 + 1, j0:j1 + 1]
    win = (z < b) | ((z == b) & (d <= -2) & (-2 - d > k))         # a face at the same depth stays; so does a lower point
    b[win] = z
    d[win] = -2 - k


def render_view(verts, faces, colors, w2c, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0, culls=CULLS, ambient=0.3,
                background=(1, 1, 1), points=None, point_colors=None, point_size=4):
    """One view -> {cull: dict(index [H,W] int64 (face, -1 background, -2 - point), D [H,W] float64 (+inf background), color and
    bound {shade: [H,W,3] float64}, unambiguous [H,W] bool, covered [H,W] bool (by anything), face_unambiguous: the face layer's)}
    plus key "nonfinite_points" [N] bool."""
    intr = [float(np.float32(x)) for x in (fx, fy, cx, cy)]
    zn, zf = float(np.float32(z_near)), float(np.float32(z_far))
    fd = _face_data(verts, faces, w2c)
    layer, rays = _face_layer(fd, culls, H, W, intr, zn, zf)
    bg = np.asarray(background, np.float32).astype(np.float64)
    sq, bad_pts = point_squares(points, w2c, H, W, intr, zn, zf, point_size) if points is not None else ([], np.zeros(0, bool))
    pcol = None if points is None else np.asarray(point_colors, np.float32).astype(np.float64).reshape(-1, 3)
    out = {"nonfinite_points": bad_pts, "nonfinite_faces": bool((~R._triangles(verts, faces, w2c, np.float64)[1]).any())}
    for cull in culls:
        ly = layer[cull]
        sh = _shade(fd, colors, ly["tri"], rays, ambient)
        ident = [np.where(ly["tri"] >= 0, ly["tri"], -1).reshape(H, W).copy() for _ in range(3)]
        best = [ly[k].reshape(H, W).copy() for k in ("D", "Dg", "Ds")]
        unamb = ly["unamb"].reshape(H, W).copy()
        s = point_size
        near = np.zeros((H, W), bool)                             # a grown square over an ambiguous or too-near face layer
        for k, z, (j0, i0), (ja, jb), (ia, ib) in sq:
            _paint(best[0], ident[0], H, W, z, k, j0, j0 + s - 1, i0, i0 + s - 1)
            _paint(best[1], ident[1], H, W, z, k, ja, jb + s - 1, ia, ib + s - 1)
            _paint(best[2], ident[2], H, W, z, k, jb, ja + s - 1, ib, ia + s - 1)
            j_lo, j_hi, i_lo, i_hi = max(ja, 0), min(jb + s - 1, W - 1), max(ia, 0), min(ib + s - 1, H - 1)
            if j_lo <= j_hi and i_lo <= i_hi:
                win = (slice(i_lo, i_hi + 1), slice(j_lo, j_hi + 1))
                dg, ds = ly["Dg"].reshape(H, W)[win], ly["Ds"].reshape(H, W)[win]
                close = (z >= dg * (1 - R.Z_RTOL)) & (z <= ds * (1 + R.Z_RTOL))
                behind_ok = ly["unamb"].reshape(H, W)[win] & (z > ds * (1 + R.Z_RTOL))     # clearly hidden by a certain face
                front_ok = z < dg * (1 - R.Z_RTOL)                                           # clearly in front of any face
                near[win] |= close | ~(behind_ok | front_ok)
        if sq:
            same = (ident[0] == ident[1]) & (ident[0] == ident[2])
            is_pt = ident[0] <= -2
            # a point of the shrunk image clearly in front of the face layer settles the pixel whatever the layer's state
            settled = is_pt & same & (best[0] < ly["Dg"].reshape(H, W) * (1 - R.Z_RTOL))
            unamb = np.where(settled, True, same & unamb & ~near)
        idx = ident[0]
        color, bound = {}, {}
        for shade in SHADES:
            c = sh[shade][0].reshape(H, W, 3).copy()
            b = sh[shade][1].reshape(H, W, 3).copy()
            c[idx == -1] = bg
            if sq:
                p = idx <= -2
                c[p] = pcol[-2 - idx[p]]
                b[p] = 0.0
            b[idx == -1] = 0.0
            color[shade], bound[shade] = c, b
        unamb = unamb & np.isfinite(bound["headlight"]).all(-1)
        out[cull] = dict(index=idx, D=best[0], color=color, bound=bound, unambiguous=unamb, covered=idx != -1,
                         face_index=ly["tri"].reshape(H, W), face_D=ly["D"].reshape(H, W), plain=ly["plain"].reshape(H, W))
    return out


def compare(ref, index, depth, color, shade):
    """The images of a renderer against one cull entry of ``render_view`` -> dict of counts: covered (by the reference),
    compared (covered and unambiguous), bad_index, bad_depth, bad_color (pixels among the unambiguous ones, background
    included) and the worst colour error over its bound."""
    un = ref["unambiguous"]
    idx = np.asarray(index).astype(np.int64)
    d = np.asarray(depth).astype(np.float64)
    c = np.asarray(color).astype(np.float64)
    bad_index = un & (idx != ref["index"])
    want_d = np.where(np.isfinite(ref["D"]), ref["D"], 0.0)
    tol = np.where(ref["index"] >= 0, R.DEPTH_RTOL * want_d, 0.0)          # points and the background: exact
    with np.errstate(all="ignore"):
        bad_depth = un & ~(np.abs(d - want_d) <= tol)
        err = np.abs(c - ref["color"][shade])
        bad_color = un & ~(err <= ref["bound"][shade]).all(-1)
        ratio = np.where(un[..., None] & (ref["bound"][shade] > 0), err / ref["bound"][shade], 0.0)
    return dict(covered=int(ref["covered"].sum()), compared=int((un & ref["covered"]).sum()), bad_index=int(bad_index.sum()),
                bad_depth=int(bad_depth.sum()), bad_color=int(bad_color.sum()), worst=float(ratio.max()) if ratio.size else 0.0)


# ---- the kernel's arithmetic in numpy float32 -------------------------------------------------------------------------------
WRONG = ("affine", "rotate", "cull", "noabs", "shift")


def render_view_f32(verts, faces, colors, w2c, H, W, fx, fy, cx, cy, z_near=0.01, z_far=20.0, cull=None, shade=None, ambient=0.3,
                    background=(1, 1, 1), points=None, point_colors=None, point_size=4, wrong=None):
    """dns_render_mesh in numpy float32, operation by operation -> (index [H,W] int64, depth [H,W] fp32, color [H,W,3] fp32).
    ``wrong``: one of WRONG, a deliberately broken renderer -- affine (screen-space) weights, weights rotated by one vertex,
    reversed culling, shading without the absolute value, point squares shifted by one pixel."""
    dt = np.float32
    assert wrong is None or wrong in WRONG
    dx, dy = R._rays(H, W, fx, fy, cx, cy, dt)
    zn, zf = dt(z_near), dt(z_far)
    tri, ok, ids = R._triangles(verts, faces, w2c, dt)
    N = H * W
    best = np.full(N, np.inf, dt)
    arg = np.full(N, -1, np.int64)
    if wrong == "cull" and cull is not None:
        cull = "front" if cull == "back" else "back"
    with np.errstate(all="ignore"):
        tri = np.where(ok[:, None, None], tri, dt(0))
        c_all = R._edges(tri, ids)[0] if len(tri) else np.zeros((0, 3, 3), dt)
        n_all = R._cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        num_all = (n_all[:, 0] * tri[:, 0, 0] + n_all[:, 1] * tri[:, 0, 1]) + n_all[:, 2] * tri[:, 0, 2]
        good = ok & (n_all != 0).any(1)
        if cull is not None:
            good = good & ((num_all < 0) if cull == "back" else (num_all > 0))
        for lo in range(0, len(tri), _CHUNK):
            s = slice(lo, lo + _CHUNK)
            c, n, num = c_all[s], n_all[s], num_all[s]
            den = (n[:, 0:1] * dx + n[:, 1:2] * dy) + n[:, 2:3]
            t = num[:, None] / den
            E = [(dx * c[:, k, 0:1] + dy * c[:, k, 1:2]) + c[:, k, 2:3] for k in range(3)]
            cover = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
            tq = np.where(cover & (t >= zn) & (t <= zf) & good[s, None], t, dt(np.inf))
            assert tq.dtype == dt
            _merge(best, arg, (), tq, lo, ())
        # points
        ident = arg.reshape(H, W).copy()
        key = best.reshape(H, W).copy()
        if points is not None:
            pw = np.asarray(points, dt).reshape(-1, 3)
            pc = R.camera_vertices_f32(pw, w2c)
            fin = np.isfinite(pw).all(1) & np.isfinite(pc).all(1)
            half = dt(point_size) * dt(0.5)
            for k in np.nonzero(fin & (pc[:, 2] >= zn) & (pc[:, 2] <= zf))[0]:
                x, y, z = pc[k]
                u = dt(fx) * (x / z) + dt(cx)
                w = dt(fy) * (y / z) + dt(cy)
                fj, fi = np.ceil(u - half), np.ceil(w - half)
                if not (fj <= W - 1 and fj + (point_size - 1) >= 0 and fi <= H - 1 and fi + (point_size - 1) >= 0):
                    continue
                j0, i0 = int(fj) + (1 if wrong == "shift" else 0), int(fi)
                _paint(key, ident, H, W, z, int(k), j0, j0 + point_size - 1, i0, i0 + point_size - 1)
        # shade
        idx = ident.ravel()
        color = np.empty((N, 3), dt)
        color[:] = np.asarray(background, dt)
        depth = np.where(idx == -1, dt(0), key.ravel()).astype(dt)
        hit = idx >= 0
        f = np.maximum(idx, 0)
        if hit.any():
            c, n = c_all[f], n_all[f]
            E = [(dx * c[:, k, 0] + dy * c[:, k, 1]) + c[:, k, 2] for k in range(3)]
            den = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
            S = (E[0] + E[1]) + E[2]
            w = [E[1] / S, E[2] / S, E[0] / S]
            if wrong == "rotate":
                w = [w[1], w[2], w[0]]
            if wrong == "affine":
                z = [tri[f, k, 2] for k in range(3)]
                tot = (w[0] * z[0] + w[1] * z[1]) + w[2] * z[2]
                w = [w[k] * z[k] / tot for k in range(3)]
            cv = [np.asarray(colors, dt)[ids[f, k]] for k in range(3)]
            col = (w[0][:, None] * cv[0] + w[1][:, None] * cv[1]) + w[2][:, None] * cv[2]
            if shade == "headlight":
                nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
                dd = (dx * dx + dy * dy) + dt(1)
                top = den if wrong == "noabs" else np.abs(den)
                light = dt(ambient) + (dt(1) - dt(ambient)) * (top / (np.sqrt(nn) * np.sqrt(dd)))
                col = col * light[:, None]
            assert col.dtype == dt
            color[hit] = col[hit]
        if points is not None:
            p = idx <= -2
            color[p] = np.asarray(point_colors, dt).reshape(-1, 3)[-2 - idx[p]]
    return ident, depth.reshape(H, W), color.reshape(H, W, 3)


# ---- the shared scenes, coloured ---------------------------------------------------------------------------------------------
PARITY = (("room", (0, 1, 2)), ("sphere", (0, 1, 2)), ("soup", (0, 1, 2)), ("lattice", (1,)))
MIN_COMPARED = 0.85


@functools.lru_cache(maxsize=None)
def scene_colors(name):
    """Vertex colours of a raster_ref scene: fp32 [P,3] in [0, 1), drawn once per scene."""
    v = R.scene(name)[0]
    seed = sum(ord(ch) for ch in name)
    return np.random.default_rng(seed).uniform(0.0, 1.0, (len(v), 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def render(name, view, ambient=0.3):
    """The reference images of view ``view`` of a raster_ref scene under every culling mode, computed once."""
    v, f, w2c, cam = R.scene(name)
    return render_view(v, f, scene_colors(name), w2c[view], *R._cam_args(cam), ambient=ambient)


# ---- points: camera actors about the lattice wall -----------------------------------------------------------------------------
def camera_actor_ref(scale, n=100):
    """The reference's create_camera_actor (utils/viz.py:14-42) written out point by point: 12 lines of n samples."""
    corner = [(0, 0, 0), (-1, -1, 1.5), (1, -1, 1.5), (1, 1, 1.5), (-1, 1, 1.5), (-0.5, 1, 1.5), (0.5, 1, 1.5), (0, 1.2, 1.5)]
    lines = [(1, 2), (2, 3), (3, 4), (4, 1), (1, 3), (2, 4), (1, 0), (0, 2), (3, 0), (0, 4), (5, 7), (7, 6)]
    out = []
    for a, b in lines:
        for k in range(n):
            t = np.linspace(0.0, 1.0, n)[k]
            out.append([scale * corner[a][x] * (1.0 - t) + scale * corner[b][x] * t for x in range(3)])
    return np.array(out, np.float64)


ACTOR_FRONT, ACTOR_BEHIND, ACTOR_BORDER = (-0.171, -0.203, 1.013), (-0.171, -0.203, 2.207), (-1.75, 0.311, 1.013)


@functools.lru_cache(maxsize=None)
def actor_cloud(where, scale=0.3):
    """A camera actor (no rotation) with its apex at ``where`` in the lattice scene: in front of the wall (z = 2), behind it, or
    across the left image border -> (points fp32 [1200,3], colours fp32 [1200,3]: a ramp, so that every point is told apart)."""
    p = (camera_actor_ref(scale) + np.asarray(where, np.float64)).astype(np.float32)
    c = np.stack((np.linspace(0.0, 1.0, len(p)), np.linspace(1.0, 0.0, len(p)), np.full(len(p), 0.25)), 1).astype(np.float32)
    return p, c


@functools.lru_cache(maxsize=None)
def render_actor(where, size, view=1):
    """The reference images (cull None) of the lattice wall with one actor cloud of point size ``size``."""
    v, f, w2c, cam = R.scene("lattice")
    p, c = actor_cloud(where)
    return render_view(v, f, scene_colors("lattice"), w2c[view], *R._cam_args(cam), culls=(None,), points=p, point_colors=c,
                       point_size=size)
