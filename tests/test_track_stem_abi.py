"""CPU: the argument block of the fused tracker iteration (ABI v25, the stem form's fields appended) has the size the library was
built with, and shapes outside the stem form are refused with the library's message by host arithmetic alone -- no launch
(dns_track_fused_ws_floats runs track.hip's shape checks and the plan of csrc/track_stem_plan.hpp)."""
import ctypes as C


def _block():
    """A DnsTrackFused of the supported stem shape (64 x 2 networks, 47 samples, two views of 64 channels); the pointers are
    placeholders that the shape checks compare with NULL and test for alignment, never follow."""
    from dns_slam_amd import _lib, ops
    a = _lib.DnsTrackFused()
    meta = ops.GridMeta(14, 32)
    a.meta = C.pointer(meta.c)
    a.n_uniform, a.n_surface, a.n_rays, a.n_bins = 32, 15, 249, 16
    a.n_neurons, a.n_hidden_layers, a.hidden, a.n_feat, a.n_class = 64, 2, 32, 64, 8
    a.maps, a.w2c, a.origin, a.w_merge, a.merge_bound = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.follow_mask, a.n_views, a.map_c, a.map_h, a.map_w = 2, 2, 64, 30, 40
    a.merge_in, a.merge_out, a.merge_bins = 3 * 16 + 64, 32, 16
    return a, meta


def _ws(a):
    from dns_slam_amd import _lib
    n = int(_lib.lib.dns_track_fused_ws_floats(C.byref(a)))
    return n, _lib.lib.dns_last_error().decode()


def test_argument_block_size():
    from dns_slam_amd import _lib
    assert C.sizeof(_lib.DnsTrackFused) == int(_lib.lib.dns_track_fused_args_bytes())


def test_stem_form_is_sized_and_grows_the_workspace():
    a, meta = _block()
    n_stem, _ = _ws(a)
    a.maps = 0
    n_plain, _ = _ws(a)
    assert n_plain > 0 and n_stem > n_plain
    # 125 workgroups of two rays: rows [2 x 94][112] + latents and their gradient [188][32] each + d OneBlob [188][48] + 2 x [188][3]
    assert n_stem - n_plain >= 125 * 188 * (112 + 32 + 32 + 48 + 6)


def test_shapes_outside_the_stem_form_are_refused_with_a_message():
    a, meta = _block()
    a.map_c, a.merge_in = 6, 3 * 16 + 6
    n, msg = _ws(a)
    assert n == 0 and "stem channels" in msg, msg
    a, meta = _block()
    a.n_uniform = 50                                             # S = 65
    n, msg = _ws(a)
    assert n == 0 and "1..64 samples" in msg, msg
    a, meta = _block()
    a.code, a.code_dim = 0x6000, 32
    n, msg = _ws(a)
    assert n == 0 and "both set" in msg, msg
    a, meta = _block()
    a.merge_out = 16
    n, msg = _ws(a)
    assert n == 0 and "output width" in msg, msg
    a, meta = _block()
    a.n_views, a.follow_mask = 9, 0
    n, msg = _ws(a)
    assert n == 0 and "reference views" in msg, msg
    a, meta = _block()
    a.maps = 0x1004
    n, msg = _ws(a)
    assert n == 0 and "16-byte aligned" in msg, msg
    a, meta = _block()
    a.merge_bins, a.merge_in = 24, 3 * 24 + 64                   # 136 columns
    n, msg = _ws(a)
    assert n == 0 and "(64, 128]" in msg, msg
