"""Generates dns_slam_amd/csrc/mc_table.hpp, the marching-cubes triangle table of csrc/mesh.hip.

    python tools/gen_mc_table.py            # rewrite the header
    python tools/gen_mc_table.py --check    # exit 1 if the committed header differs

Numbering (the header repeats it):
  corner c in 0..7     : offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z); case bit c = corner c is INSIDE (v > level)
  edge   e in 0..11    : axis a = e // 4 (0 x, 1 y, 2 z); its start corner has offsets (o1, o2) = (e & 1, (e >> 1) & 1) along the
                         two other axes in increasing order, 0 along a; it ends at the start corner + 1 along a
  grid edge            : (point p = (i, j, k), axis a) -- the edge from p to p + 1 along a; its linear index is 3 * (C-order index
                         of p) + a, the order of the output vertices

Rule.  On each of the cube's six faces the sign-changing edges pair into segments: two crossings pair with each other; four
crossings (an ambiguous face: two diagonal inside corners) pair around each inside corner, so the inside corners stay
separated.  The decision reads the face's four signs only, so the two cubes that share a face draw the same segments.  Each
segment is oriented so that, seen from outside the face, the surface's normal points from the inside corners to the outside
ones ("descent": from high values to low); a neighbouring cube sees the face from the other side and runs the segment the
other way.  Every crossing edge lies on two faces, so the segments chain into closed loops; each loop is fan-triangulated
from an apex chosen so that no fan diagonal joins two points of one cube face (such a chord would be drawn by the
neighbouring cube as well).
"""
from __future__ import annotations

import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "dns_slam_amd", "csrc", "mc_table.hpp")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(start corner, end corner) of cube edge e."""
    a = e // 4
    others = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = e & 1, (e >> 1) & 1
    c0 = off[0] | (off[1] << 1) | (off[2] << 2)
    return c0, c0 | (1 << a)


def edge_mid(e):
    c0, c1 = edge_corners(e)
    return tuple((p + q) / 2 for p, q in zip(corner_pos(c0), corner_pos(c1)))


def faces():
    """The six cube faces as (outward normal, ring of 4 corners in cyclic order, the 4 edges between consecutive ring corners)."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            ring = []
            for ob, oc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[a], off[b], off[c] = s, ob, oc
                ring.append(off[0] | (off[1] << 1) | (off[2] << 2))
            edges = []
            for r in range(4):
                pair = {ring[r], ring[(r + 1) % 4]}
                edges.append(next(e for e in range(12) if set(edge_corners(e)) == pair))
            n = [0, 0, 0]
            n[a] = 1 if s else -1
            out.append((tuple(n), ring, edges))
    return out


FACES = faces()


def _sub(p, q):
    return tuple(x - y for x, y in zip(p, q))


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(p, q):
    return sum(x * y for x, y in zip(p, q))


def face_segments(case, face):
    """Directed segments (edge_from, edge_to) of one face for a case."""
    n, ring, edges = face
    inside = [(case >> c) & 1 for c in ring]
    # edge r joins ring[r] and ring[r + 1]
    cross = [r for r in range(4) if inside[r] != inside[(r + 1) % 4]]
    if not cross:
        return []
    if len(cross) == 2:
        pairs = [(edges[cross[0]], edges[cross[1]], next(ring[r] for r in range(4) if inside[r]))]
    else:
        # ambiguous face: each inside corner r is cut off by the segment of its two adjacent edges (r - 1 and r)
        pairs = [(edges[(r - 1) % 4], edges[r], ring[r]) for r in range(4) if inside[r]]
    segs = []
    for ea, eb, cin in pairs:
        A, B, I = edge_mid(ea), edge_mid(eb), _sub(corner_pos(cin), edge_mid(ea))
        d = _sub(B, A)
        # direction T = N x n_f with N the in-face direction from inside to outside: A -> B iff n_f . (I x d) > 0
        segs.append((ea, eb) if _dot(n, _cross(I, d)) > 0 else (eb, ea))
    return segs


def case_segments(case):
    return [s for f in FACES for s in face_segments(case, f)]


def edge_faces(e):
    return {fi for fi, (_, _, edges) in enumerate(FACES) if e in edges}


def case_loops(case):
    nxt = {}
    for a, b in case_segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case       # every crossing edge: one segment in, one out
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, case
        loops.append(loop)
    return loops


def fan(loop):
    """Fan triangles of one loop from the first apex whose diagonals never join two points of one cube face."""
    L = len(loop)
    for r in range(L):
        lp = loop[r:] + loop[:r]
        diagonals = [(lp[0], lp[i]) for i in range(2, L - 1)]
        if all(not (edge_faces(a) & edge_faces(b)) for a, b in diagonals):
            return [(lp[0], lp[i], lp[i + 1]) for i in range(1, L - 1)]
    raise AssertionError(f"no admissible fan apex for loop {loop}")


def build_table():
    """[256] lists of triangles (edge ids, wound by the rule)."""
    return [[t for loop in case_loops(case) for t in fan(loop)] for case in range(256)]


def render(table) -> str:
    max_tri = max(len(t) for t in table)
    assert max_tri == 5, max_tri                          # the row width below is sized from this
    lines = [
        "// Marching-cubes triangle table of csrc/mesh.hip.  GENERATED by tools/gen_mc_table.py -- do not edit.",
        "// corner c: offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); case bit c = corner c inside (v > level).",
        "// edge e: axis e / 4 (x, y, z); start offsets (e & 1, (e >> 1) & 1) along the other two axes in increasing order.",
        "// Triangles are wound so that the right-hand normal points from inside (high values) to outside.",
        "#pragma once",
        "#ifndef MC_TABLE_SPACE",
        "#define MC_TABLE_SPACE",
        "#endif",
        f"#define MC_MAX_TRI {max_tri}",
        "",
        "// triangles per case",
        "MC_TABLE_SPACE static const unsigned char mc_ntri[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// edge ids of the triangles of each case, 3 per triangle, -1 padded")
    lines.append("MC_TABLE_SPACE static const signed char mc_tri[256][3 * MC_MAX_TRI] = {")
    for c in range(256):
        flat = [e for t in table[c] for e in t] + [-1] * (3 * (max_tri - len(table[c])))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},")
    lines.append("};")
    lines.append("")
    # the cube edge -> (corner offset of its start point, axis) map: grid edge = (cube point + offset, axis)
    lines.append("// cube edge e -> grid edge (start-point offset dx, dy, dz, axis)")
    lines.append("MC_TABLE_SPACE static const unsigned char mc_edge[12][4] = {")
    for e in range(12):
        c0, _ = edge_corners(e)
        x, y, z = corner_pos(c0)
        lines.append(f"    {{{x}, {y}, {z}, {e // 4}}},")
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render(build_table())
    if "--check" in argv:
        with open(OUT) as f:
            same = f.read() == text
        print("mc_table.hpp up to date" if same else "mc_table.hpp differs from the generator")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
