"""CPU: the byte rules of ops.vis_panels as tests/vis_panels_ref.py restates them, against matplotlib (what fig_plot's imshow calls
compute for a pixel), and the committed plasma table against matplotlib's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_panels_ref as vr  # noqa: E402

matplotlib = pytest.importorskip("matplotlib")
from matplotlib import cm, colormaps  # noqa: E402
from matplotlib.colors import Normalize  # noqa: E402


def _mpl_scalar(x, vmax):
    """imshow(x, cmap="plasma", vmin=0, vmax=vmax)'s colour of every element, as bytes."""
    return colormaps["plasma"](Normalize(vmin=0, vmax=vmax)(x), bytes=True)[..., :3]


def test_committed_header_is_matplotlibs_table():
    want = (np.asarray(colormaps["plasma"].colors, dtype=np.float64) * 255).astype(np.uint8)
    assert np.array_equal(vr.header_table(), want)
    # ... and what the colour map returns for the centre of every table cell
    centres = (np.arange(256) + 0.5) / 256
    assert np.array_equal(colormaps["plasma"](centres, bytes=True)[:, :3], want)


@pytest.mark.parametrize("vmax", [1.0, 5.7341, 101.0, 0.013])
def test_scalar_rule_is_matplotlibs(vmax):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-0.1 * vmax, 1.2 * vmax, size=200000).astype(np.float32),
                        np.linspace(0, vmax, 4097, dtype=np.float32),                      # the cell borders k / 256 and around
                        np.array([0.0, vmax, np.nextafter(np.float32(vmax), np.float32(0)), 2 * vmax, -vmax], dtype=np.float32)])
    table = vr.header_table()
    got = vr.scalar_panel(x, np.float32(vmax), table, 255)
    assert np.array_equal(got, _mpl_scalar(x, np.float32(vmax)))


def test_integer_labels_rule_is_matplotlibs():
    lab = np.arange(0, 140, dtype=np.int64)
    got = vr.scalar_panel(lab.astype(np.float32), 101, vr.header_table(), 255)
    assert np.array_equal(got, _mpl_scalar(lab, 101))


def test_zero_vmax_is_index_zero():
    x = np.array([0.0, 1.0, -1.0], dtype=np.float32)
    got = vr.scalar_panel(x, np.float32(0.0), vr.header_table(), 255)
    assert (got == vr.header_table()[0]).all()
    assert np.array_equal(got, _mpl_scalar(x, np.float32(0.0)))


def test_colour_rule_is_matplotlibs():
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.3, 1.3, size=(64, 64, 3)).astype(np.float32)
    x[0, 0] = [0.0, 1.0, 0.5]
    want = cm.ScalarMappable(cmap="plasma").to_rgba(np.clip(x, 0, 1), bytes=True)[..., :3]     # imshow of an RGB float image
    assert np.array_equal(vr.colour_panel(x), want)


def test_non_finite_scalars_take_the_background():
    """The stated deviation: matplotlib draws its transparent "bad" colour there."""
    x = np.array([np.nan, np.inf, -np.inf, 1.0], dtype=np.float32)
    got = vr.scalar_panel(x, np.float32(2.0), vr.header_table(), 200)
    assert (got[:3] == 200).all() and not (got[3] == 200).all()
    assert vr.depth_vmax(np.array([[np.nan, np.inf, 3.0, -4.0]], dtype=np.float32)) == np.float32(3.0)
    assert vr.depth_vmax(np.array([[np.nan, 0.0]], dtype=np.float32)) == np.float32(0.0)


def test_sheet_layout_and_label_table():
    H, W, gap = 5, 7, 3
    gc, ec, gd, ed, gl, el = vr.make_inputs(H, W, 0)
    lut = np.array([40, 3, 17, 99, 0, 1, 2, 120], dtype=np.int32)
    s, vmax = vr.sheet(gc, ec, gd, ed, gl, el, label_lut=lut, gap=gap, background=9)
    assert s.shape == (3 * H + 2 * gap, 3 * W + 2 * gap, 3) and s.dtype == np.uint8 and vmax == gd.max()
    assert (s[H:H + gap] == 9).all() and (s[:, W:W + gap] == 9).all() and (s[:, 2 * W + gap:2 * (W + gap)] == 9).all()
    table = vr.header_table()
    assert np.array_equal(s[:H, :W], _mpl_scalar(gd, vmax))
    assert np.array_equal(s[:H, 2 * (W + gap):], _mpl_scalar(np.abs(gd - ed), vmax))
    assert np.array_equal(s[2 * (H + gap):, W + gap:2 * W + gap], _mpl_scalar(lut[el], 101))
    assert np.array_equal(s[2 * (H + gap):, 2 * (W + gap):], _mpl_scalar(np.abs(lut[gl] - lut[el]), 101))
    assert np.array_equal(s[H + gap:2 * H + gap, :W], vr.colour_panel(gc))
    # without the table the labels are drawn as they are
    s2, _ = vr.sheet(gc, ec, gd, ed, gl, el, gap=gap, background=9, table=table)
    assert np.array_equal(s2[2 * (H + gap):, :W], _mpl_scalar(gl, 101))
