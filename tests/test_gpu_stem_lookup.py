"""GPU: the spellings of the feature branch's stem-map lookup, held to each other bit for bit.  dns_feature_gather (both lane
forms), dns_feature_gather_frames (both lane forms) and dns_kf_pair_rows all read the map through csrc/dev_feature.hpp; what can
still differ between them is the wiring -- ``h`` for ``H``, a view offset applied twice, the FRAMES index, the row stride.  (The
fused frame-codes kernel does not expose its stem columns: tests/test_gpu_frame_codes.py holds it.)

Frames of 24 x 32 (tap scales 15/31 and 11/23) and 23 x 31 (exactly 1/2) over maps [3, 12, 16, C]; C = 64, and C = 8 with fewer
float4s than the 16 lanes of a pair.  600 points: 300 back-projected from view 0 at INTEGER pixel centres and depths 0.3 .. 3.3 --
the first 16 are every (u, v) of {0, 1, W-2, W-1} x {0, 1, H-2, H-1}, 64 more have one coordinate on such a border -- 60 behind
the camera of view 0, 240 uniform in a box around the cameras."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
h, w, R, P, N0, PAD = 12, 16, 3, 600, 300, 12
FX = 24.0
_CACHE = {}


def backproject(c2w, cx, cy, u, v, d):
    """World points that view ``c2w`` projects to pixel (u, v) at depth d (feature_matching's convention: y and z flipped), as
    tests/test_gpu_frame_codes.py's."""
    x = (u - cx) / FX * d
    y = -(v - cy) / FX * d
    pc = torch.stack((x, y, -d, torch.ones_like(d)), -1)
    return (pc @ c2w.T)[:, :3]


def inputs(H, W, Cc):
    """The case's tensors, on the host."""
    g = torch.Generator().manual_seed(1000 * H + Cc)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    K = torch.tensor([[FX, 0.0, cx], [0.0, FX, cy], [0.0, 0.0, 1.0]])
    # three poses: a rotation of up to ~0.2 rad about a random axis, a translation of ~0.2
    a = torch.randn(R, 3, generator=g, dtype=torch.float64) * 0.12
    skew = torch.zeros(R, 3, 3, dtype=torch.float64)
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -a[:, 2], a[:, 1], -a[:, 0]
    c2w = torch.eye(4, dtype=torch.float64).repeat(R, 1, 1)
    c2w[:, :3, :3] = torch.matrix_exp(skew - skew.transpose(1, 2))
    c2w[:, :3, 3] = torch.randn(R, 3, generator=g, dtype=torch.float64) * 0.2
    w2c = torch.stack([torch.inverse(m) for m in c2w]).float().contiguous()
    c2w = c2w.float()
    ub, vb = torch.tensor([0, 1, W - 2, W - 1]), torch.tensor([0, 1, H - 2, H - 1])
    ri = lambda n, hi: torch.randint(0, hi, (n,), generator=g)
    n_rest = N0 - 16 - 64
    u = torch.cat((ub.repeat_interleave(4), ub[ri(32, 4)], ri(32, W), ri(n_rest, W))).float()
    v = torch.cat((vb.repeat(4), ri(32, H), vb[ri(32, 4)], ri(n_rest, H))).float()
    d = torch.rand(N0, generator=g) * 3.0 + 0.3
    n_back = P // 10
    ahead = backproject(c2w[0], cx, cy, u, v, d)
    behind = backproject(c2w[0], cx, cy, torch.rand(n_back, generator=g) * W, torch.rand(n_back, generator=g) * H,
                         -(torch.rand(n_back, generator=g) * 3.0 + 0.3))
    box = c2w[0, :3, 3] + (torch.rand(P - N0 - n_back, 3, generator=g) - 0.5) * torch.tensor([6.0, 5.0, 7.0])
    pts = torch.cat((ahead, behind, box), 0).float().contiguous()
    feat = torch.randn(R, h, w, Cc, generator=g)
    return {"H": H, "W": W, "C": Cc, "K": K, "K9": (C.c_float * 9)(*K.reshape(-1).tolist()), "u": u, "v": v,
            "inside": (u > 0) & (u < W - 1) & (v > 0) & (v < H - 1), "pts": pts, "w2c": w2c, "origin": c2w[:, :3, 3].contiguous(),
            "feat": feat}


def setup(H, W, Cc):
    key = (H, W, Cc)
    if key in _CACHE:
        return _CACHE[key]
    from dns_slam_amd import ops
    s = inputs(H, W, Cc)
    for k in ("pts", "w2c", "origin", "feat"):
        s[k] = s[k].to(DEV)
    # the plain gather in the library's default lane form: what every other entry point is held to
    s["code"], s["mask"] = ops.feature_gather(s["pts"], s["w2c"], s["K"], s["feat"], H, W)
    _CACHE[key] = s
    return s


def frames_entry(s):
    """dns_feature_gather_frames as launch.Stem2D calls it: one frame of P points, R views, the code behind PAD other columns."""
    from dns_slam_amd import ops
    from dns_slam_amd._lib import check, ptr, stream_ptr
    buf = torch.full((R * P, PAD + s["C"]), 7.0, device=DEV)
    rel = torch.full((R * P, 3), 7.0, device=DEV)
    check(ops.lib.dns_feature_gather_frames(ptr(s["pts"]), ptr(s["w2c"]), ptr(s["origin"]), s["K9"], ptr(s["feat"]), 1, R, P, s["C"],
                                            h, w, s["H"], s["W"], C.c_void_p(buf.data_ptr() + 4 * PAD), PAD + s["C"], ptr(rel),
                                            stream_ptr()), "dns_feature_gather_frames")
    return buf, rel


def pair_rows(s, records):
    """dns_kf_pair_rows as ops.keyframe_codes calls it: records [n, 4] = {point, view, u, v}."""
    from dns_slam_amd import ops
    from dns_slam_amd._lib import check, ptr, stream_ptr
    n = records.shape[0]
    records = records.to(torch.int32).contiguous().to(DEV)
    buf = torch.full((n, PAD + s["C"]), 7.0, device=DEV)
    rel = torch.full((n, 3), 7.0, device=DEV)
    check(ops.lib.dns_kf_pair_rows(ptr(records), n, ptr(s["pts"]), P, ptr(s["origin"]), R, ptr(s["feat"]), s["C"], h, w, s["H"], s["W"],
                                   ptr(rel), C.c_void_p(buf.data_ptr() + 4 * PAD), PAD + s["C"], stream_ptr()), "dns_kf_pair_rows")
    return buf, rel


CASES = [(24, 32, 64), (24, 32, 8), (23, 31, 64), (23, 31, 8)]


@pytest.mark.parametrize("H,W,Cc", CASES)
def test_known_pixels(H, W, Cc):
    """(a) A point back-projected from an integer pixel of view 0 is valid there iff 0 < u < W - 1 and 0 < v < H - 1."""
    s = setup(H, W, Cc)
    # float64, the convention's unrounded pixel: every such point lies within 1e-3 px of its centre, so its rounding is known
    p64 = torch.cat((s["pts"][:N0].cpu().double(), torch.ones(N0, 1, dtype=torch.float64)), -1)
    cam = s["w2c"][0].cpu().double() @ p64.T
    q = s["K"].double() @ torch.stack((cam[0], -cam[1], -cam[2]))
    off = torch.maximum((q[0] / (q[2] + 1e-5) - s["u"].double()).abs(), (q[1] / (q[2] + 1e-5) - s["v"].double()).abs())
    print(f"{H} x {W}: largest distance from the pixel centre {float(off.max()):.3e} px, smallest depth {float((-cam[2]).min()):.3f}")
    assert float(off.max()) < 1e-3 and float((-cam[2]).min()) > 0.29
    share = float(s["inside"].float().mean())
    print(f"valid by construction: {int(s['inside'].sum())} of {N0} ({100 * share:.1f} %)")
    assert share >= 0.40
    assert torch.equal(s["mask"][0, :N0].cpu(), s["inside"])
    assert float(s["code"][0, :N0][s["inside"].to(DEV)].abs().max()) > 0
    n_back = P // 10
    assert not bool(s["mask"][0, N0:N0 + n_back].any())                  # behind the camera of view 0


@pytest.mark.parametrize("lanes", ["float4", "scalar"])
@pytest.mark.parametrize("H,W,Cc", CASES)
def test_frames_entry_equals_plain_gather(H, W, Cc, lanes, monkeypatch):
    """(b) One frame through dns_feature_gather_frames, in both lane forms."""
    s = setup(H, W, Cc)
    if lanes == "scalar":
        monkeypatch.setenv("DNS_FEATURE_GATHER_LANES", "1")
    else:
        monkeypatch.delenv("DNS_FEATURE_GATHER_LANES", raising=False)
    buf, rel = frames_entry(s)
    assert torch.equal(buf[:, PAD:], s["code"].reshape(R * P, Cc))
    assert bool((buf[:, :PAD] == 7.0).all())
    assert torch.equal(rel.reshape(R, P, 3), s["pts"][None] - s["origin"][:, None])


@pytest.mark.parametrize("H,W,Cc", CASES)
def test_pair_rows_equal_plain_gather(H, W, Cc, monkeypatch):
    """(c) The valid back-projected points as records {p, 0, u, v} through dns_kf_pair_rows."""
    s = setup(H, W, Cc)
    monkeypatch.delenv("DNS_FEATURE_GATHER_LANES", raising=False)
    idx = torch.nonzero(s["inside"])[:, 0]
    assert idx.numel() >= 0.4 * N0
    rec = torch.stack((idx, torch.zeros_like(idx), s["u"][idx].long(), s["v"][idx].long()), 1)
    buf, rel = pair_rows(s, rec)
    assert torch.equal(buf[:, PAD:], s["code"][0, idx.to(DEV)])
    assert bool((buf[:, :PAD] == 7.0).all())
    assert torch.equal(rel, frames_entry(s)[1][idx.to(DEV)])             # view 0: the first P rows of (b)'s rel


@pytest.mark.parametrize("H,W,Cc", CASES)
def test_pair_rows_at_the_map_edge(H, W, Cc):
    """(d) The last pixel, which feature_gather rejects and dns_kf_pair_rows accepts: sx = w - 1 and sy = h - 1 exactly, so
    lx = ly = 0, every tap is the map's last pixel (this is where the clamp of x0 / y0 and the x1 / y1 edge rule act) and the row
    is that pixel's bits."""
    s = setup(H, W, Cc)
    buf, _ = pair_rows(s, torch.tensor([[5, 0, W - 1, H - 1]]))
    assert torch.equal(buf[0, PAD:], s["feat"][0, h - 1, w - 1])
