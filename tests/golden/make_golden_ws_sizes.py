"""Generate tests/golden/ws_sizes.json: what the exported dns_*_ws_bytes functions return, as plain data.

Run only when a workspace layout is changed on purpose, against a build of the commit whose sizes are to be pinned (the
functions are host arithmetic: no GPU is needed):

    DNS_HIP_LIB=<that build's libdns_hip.so> python tests/golden/make_golden_ws_sizes.py

tests/test_ws_sizes.py holds the built library to the table; it never runs this file.  Every argument list holds the smallest
accepted size, the block boundaries of the unit with their two neighbours, one size in the millions, the largest accepted
value and every refusal threshold with the value just below it (a refusal is recorded as 0).
"""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

P28, P29, P31, P32 = 1 << 28, 1 << 29, 1 << 31, 1 << 32
AROUND = (63, 64, 65, 255, 256, 257)              # a wave, a workgroup
LIST = 1 << 24                                    # dev_raster.hpp: RS_LIST_CAP (triangle, view) pairs
TILE = 1024                                       # mesh_eval.hip: one scan tile of 2048 cells is 1024 reference points
CELLS = 1 << 20                                   # ... and the cell count stops growing at 2^21 cells


def _points(limit):
    return [1, *AROUND, 1000003, limit - 1, limit]


def _raster():
    args = [(0, 0, 1, 1), (1, 1, 1, 1), (1000, 3, 48, 64), (2000000, 3, 480, 640)]
    args += [(f, 1, 48, 64) for f in (LIST - 1, LIST, LIST + 1)] + [(4096, 4095, 8, 8), (4096, 4096, 8, 8), (4097, 4096, 8, 8)]
    args += [(P31 - 1, P32 - 1, 1, 1), (P31, 1, 1, 1), (P31 - 1, 65536, 32768, 32768)]
    args += [(1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 32768, 1), (1, 1, 32769, 1), (1, 1, 1, 32768), (1, 1, 1, 32769)]
    return args


def _clouds(empty):
    args = [(1, 1), (1000, 777), (3000000, 2000000), (P31 - 1, P31 - 1), (P31, 1), (P31 - 1, 1), (1, P31), (1, P31 - 1)]
    args += [(m, 5) for m in (TILE - 1, TILE, TILE + 1, CELLS - 1, CELLS, CELLS + 1)] + [(5, n) for n in AROUND]
    return args + list(empty)


CASES = {
    "dns_mc_ws_bytes": [(4, 4, 4), (128, 128, 128), (2048, 2048, 512), (2048, 2048, 1024), (0, 1, 1), (1, 0, 1), (1, 1, 0)]
                       + [(n, 1, 1) for n in _points(P31)] + [(1, 1, n) for n in AROUND],
    "dns_mesh_cc_ws_bytes": [(f,) for f in [0, *_points(P29), 1 << 20, P32 - 1]],
    "dns_mesh_holes_ws_bytes": [(0, 3), (1, 0), (1, 3), (2000000, 1000003), (P29 - 1, P31 - 1), (P29 - 1, 3), (P29, 3), (1, P31 - 1),
                                (1, P31)] + [(f, 100) for f in AROUND] + [(100, v) for v in AROUND],
    "dns_nearest_ws_bytes": _clouds([(0, 0), (0, 5), (5, 0)]),
    "dns_icp_ws_bytes": _clouds([(0, 0), (0, 1), (1, 0)]),
    "dns_rasterize_ws_bytes": _raster(),
    "dns_render_mesh_ws_bytes": _raster(),
    "dns_convex_hull_ws_bytes": [(0, 0), (4, 4), (1000, 64), (3000000, 4096), (P31 - 1, P28 - 1), (P31, 4), (P31 - 1, 4), (4, P28),
                                 (4, P28 - 1)] + [(n, 64) for n in AROUND] + [(1000, c) for c in AROUND],
    # the control: image_metrics.hip is not carved into 256-byte parts
    "dns_ms_ssim_ws_bytes": [(1, 161, 161), (1, 160, 200), (1, 200, 160), (0, 161, 161), (10, 1080, 1920), (65535, 161, 161),
                             (65536, 161, 161), (1, 32768, 32768), (1, 32769, 161), (1, 161, 32769)],
}


def main():
    sys.path.insert(0, ROOT)
    from dns_slam_amd import _lib
    table = {name: [[list(a), int(getattr(_lib.lib, name)(*a))] for a in args] for name, args in CASES.items()}
    with open(os.path.join(OUT, "ws_sizes.json"), "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n' + ",\n".join("  " + json.dumps(row) for row in rows) + "\n ]"
                                   for name, rows in table.items()) + "\n}\n")
    print(f"ws_sizes.json: {sum(len(r) for r in table.values())} calls of {len(table)} functions from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
