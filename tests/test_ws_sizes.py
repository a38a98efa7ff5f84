"""CPU: the byte-workspace sizes of the C ABI are the recorded ones (host arithmetic, no launch).

Python allocates exactly what dns_*_ws_bytes returns and the launch wrappers carve that allocation by the same layout function
(csrc/ws_carve.hpp), so a size that moves is a layout that moved.  tests/golden/ws_sizes.json holds, for each of the nine
functions, the smallest accepted size, the units' block boundaries and their neighbours, a size in the millions, the largest
accepted value and every refusal threshold with the value below it.  The table is regenerated
(tests/golden/make_golden_ws_sizes.py) only when a layout is changed on purpose; this test never runs the generator."""
import json
import os

import pytest

_TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_sizes.json")))
_SPOT = {"dns_mc_ws_bytes": ((4, 4, 4), 528), "dns_mesh_cc_ws_bytes": ((1,), 772), "dns_mesh_holes_ws_bytes": ((1, 3), 2304),
         "dns_nearest_ws_bytes": ((1000, 777), 51200), "dns_icp_ws_bytes": ((1000, 777), 200192),
         "dns_rasterize_ws_bytes": ((1000, 3, 48, 64), 286208), "dns_render_mesh_ws_bytes": ((1000, 3, 48, 64), 359936),
         "dns_convex_hull_ws_bytes": ((1000, 64), 48128)}


def test_table_is_the_one_that_was_recorded():
    assert len(_TABLE) == 9 and set(_SPOT) | {"dns_ms_ssim_ws_bytes"} == set(_TABLE)
    for name, (args, value) in _SPOT.items():
        assert [list(args), value] in _TABLE[name], name
    for name, rows in _TABLE.items():
        values = [v for _, v in rows]
        assert len(rows) >= 10 and values.count(0) >= 2 and max(values) > 1 << 20, name       # refusals and large sizes are in it


@pytest.mark.parametrize("name", sorted(_TABLE))
def test_sizes_are_the_recorded_ones(name):
    from dns_slam_amd import _lib
    fn = getattr(_lib.lib, name)
    got = [[args, int(fn(*args))] for args, _ in _TABLE[name]]
    assert got == _TABLE[name]
