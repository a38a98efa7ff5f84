"""GPU: ops.frame_codes -- the 2-D code of a frame's samples in one kernel (csrc/frame_codes.hip) -- against the composition of
launches it replaces (common.feature_matching: the path of the parent commit), against the oracle, on planted edge cases, for
determinism, for the ``keep`` mask with non-finite map values, and its refusals.

Set-up as in tests/test_gpu_features.py: camera 24 x 32, stem maps 12 x 16 x 64 of ResNet(seed=3), a randomised Merge network.
677 points = five full tiles of 128 and one of 37 (tile=128; the library's own choice at this size is 128 for one view, 64 for three); half of them are back-projections of random pixels of view 0 at random depths
(view 0 sees them), the rest are uniform in 1.2 x the bound."""
import pytest
import torch

from oracle import feature_ref as fr
from util import assert_close, randomise_

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, P = 24, 32, 677
_CACHE = {}


def backproject(c2w, cam, u, v, d):
    """World points that view ``c2w`` projects to pixel (u, v) at depth d (feature_matching's convention: y and z flipped)."""
    x = (u - cam["cx"]) / cam["fx"] * d
    y = -(v - cam["cy"]) / cam["fy"] * d
    pc = torch.stack((x, y, -d, torch.ones_like(d)), -1)
    return (pc @ c2w.T)[:, :3]


def setup(nn=32, nl=1, dtype="fp32", pixel_dim=64):
    key = (nn, nl, dtype, pixel_dim)
    if key in _CACHE:
        return _CACHE[key]
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.encoder import ResNet
    cam = synthetic.camera(H=H, W=W, fx=24.0, fy=24.0)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=3)
    cfg = synthetic.default_cfg(n_pixels=200, hash_size=14, voxel_size=0.08, smooth_pts=10, n_neurons=nn, n_hidden_layers=nl,
                                mlp_dtype=dtype)
    cfg["model"]["pixel_dim"] = pixel_dim
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    randomise_(dec.merge, 21)
    stem = ResNet(seed=3).to(DEV)
    images = frames["gt_color"][:3]
    maps = stem(images[None].to(DEV))[0].detach()                     # [3, 64, 12, 16]
    nhwc = maps.permute(0, 2, 3, 1).contiguous()
    c2w = frames["est_c2w"][:3].float()
    w2c = torch.inverse(c2w).contiguous()                             # (a batched inverse comes back column-major)
    g = torch.Generator().manual_seed(17)
    n0 = P // 2
    u = torch.rand(n0, generator=g) * (W - 3) + 1.0
    v = torch.rand(n0, generator=g) * (H - 3) + 1.0
    d = torch.rand(n0, generator=g) * 3.0 + 0.3
    b = torch.as_tensor(bound).float()
    mid, ext = (b[:, 0] + b[:, 1]) / 2, b[:, 1] - b[:, 0]
    rest = mid + (torch.rand(P - n0, 3, generator=g) - 0.5) * 1.2 * ext
    pts = torch.cat((backproject(c2w[0], cam, u, v, d), rest), 0).float()
    out = {"cam": cam, "bound": bound, "frames": frames, "cfg": cfg, "dec": dec, "stem": stem, "images": images, "maps": maps,
           "nhwc": nhwc, "c2w": c2w, "w2c": w2c, "pts": pts, "mid": mid, "ext": ext}
    _CACHE[key] = out
    return out


def codes(s, R, method, pts=None, **kw):
    from dns_slam_amd import ops
    pts = s["pts"] if pts is None else pts
    return ops.frame_codes(pts.to(DEV), s["w2c"][:R].to(DEV), kw.pop("nhwc", s["nhwc"])[:R], s["cam"], H, W, s["dec"].merge,
                           method=method, **kw)


def valid_mask(s, R, pts=None):
    from dns_slam_amd import ops
    pts = s["pts"] if pts is None else pts
    K = torch.tensor([[s["cam"]["fx"], 0.0, s["cam"]["cx"]], [0.0, s["cam"]["fy"], s["cam"]["cy"]], [0.0, 0.0, 1.0]])
    return ops.feature_gather(pts.to(DEV), s["w2c"][:R].to(DEV), K, s["nhwc"][:R], H, W)[1].cpu()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("net", [(32, 1), (64, 2)])
def test_fused_equals_the_launches(R, net):
    """The path of the parent commit (feature_gather -> encode -> cat -> Merge -> mean) and the fused kernel share every
    expression: assert_close at its defaults, no outliers.  Largest difference measured on an MI355X: DESIGN 4.20."""
    s = setup(*net)
    assert float(valid_mask(s, R).float().mean()) >= 0.10
    b = codes(s, R, "launches")
    assert float(b.abs().max()) > 0
    for tile in (128, 0):                                              # five full tiles and one of 37; the library's choice
        a = codes(s, R, "fused", tile=tile)
        assert a.shape == (P, 32) and a.dtype == torch.float32
        print(f"R {R} net {net} tile {tile}: max |fused - launches| = {float((a - b).abs().max()):.3e} of max "
              f"{float(b.abs().max()):.3e}, {int((a != b).sum())} of {a.numel()} values differ")
        assert_close(a.cpu(), b.cpu(), what=f"frame_codes fused vs launches R={R} net={net} tile={tile}")


@pytest.mark.parametrize("net", [(32, 1), (64, 2)])
def test_fused_matches_the_oracle(net):
    """oracle.feature_ref.feature_matching + merge_forward on the maps of fr.stem_forward.  Points whose unrounded pixel
    coordinate (float64) lies within 1e-3 px of a half-integer in any view, or whose depth there is within 1e-3 of zero, may round
    to another pixel or flip validity in fp32: dropped first, at most 5 % of them."""
    s = setup(*net)
    R, cam = 3, s["cam"]
    sd = s["stem"].conv_blocks.state_dict()
    fo = fr.stem_forward(s["images"][None], sd["conv1.weight"].cpu(), sd["bn1.weight"].cpu(), sd["bn1.bias"].cpu(),
                         sd["bn1.running_mean"].cpu(), sd["bn1.running_var"].cpu())[0]
    K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])
    params = s["dec"].merge.decoder.params.detach().cpu()
    merge = lambda p_, o_, c_: fr.merge_forward(params, s["bound"], p_, o_, c_, n_neurons=net[0], n_hidden_layers=net[1])
    want = fr.feature_matching(H, W, K, s["pts"], s["w2c"], fo, merge)
    got = codes(s, R, "fused").cpu()
    p64 = torch.cat((s["pts"].double(), torch.ones(P, 1, dtype=torch.float64)), -1)
    v = torch.matmul(s["w2c"].double(), p64.T)                         # [R, 4, P]
    cx_, cy_, cz_ = v[:, 0], -v[:, 1], -v[:, 2]
    q = torch.matmul(K.double()[None], torch.stack((cx_, cy_, cz_), 1))
    uu, vv = q[:, 0] / (q[:, 2] + 1e-5), q[:, 1] / (q[:, 2] + 1e-5)
    near_half = lambda t: ((t - torch.floor(t)) - 0.5).abs() < 1e-3
    drop = (near_half(uu) | near_half(vv) | (cz_.abs() < 1e-3)).any(0)
    share = float(drop.float().mean())
    print(f"net {net}: dropped {int(drop.sum())} of {P} points ({100 * share:.2f} %)")
    assert share <= 0.05
    assert_close(got[~drop], want[~drop], what=f"frame_codes fused vs oracle net={net}")


def planted_points(s):
    """-> (points, what each is).  View 0 (a camera on a circle, looking outward) at pixel row 12."""
    cam, c2w = s["cam"], s["c2w"]
    one = lambda u, d: backproject(c2w[0], cam, torch.tensor([float(u)]), torch.tensor([12.0]), torch.tensor([float(d)]))
    pts = [one(16, -1.0),                                              # behind view 0
           one(0, 1.5), one(1, 1.5), one(W - 2, 1.5), one(W - 1, 1.5),  # u rounds to 0 (invalid), 1, W-2 (valid), W-1 (invalid)
           (s["mid"] + 10.0 * s["ext"])[None],                         # far outside the bound: rel outside the OneBlob range
           c2w[:3, :3, 3].mean(0, keepdim=True)]                       # between the outward-looking cameras: behind all of them
    return torch.cat(pts, 0).float(), ("behind", "u0", "u1", "uW-2", "uW-1", "far", "unseen")


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("net", [(32, 1), (64, 2)])
def test_planted_cases(R, net):
    s = setup(*net)
    pl, names = planted_points(s)
    m = valid_mask(s, R, pl)
    assert [bool(x) for x in m[0, :5]] == [False, False, True, True, False], m[0]
    assert not bool(m[:, 6].any())                                     # no view sees the last point
    pts = torch.cat((pl, s["pts"][:150]), 0)                           # more than one tile, the plants first
    a, b = codes(s, R, "fused", pts, tile=128), codes(s, R, "launches", pts)
    assert torch.equal(a, codes(s, R, "fused", pts))
    assert_close(a.cpu(), b.cpu(), what=f"frame_codes planted cases R={R} net={net}")
    assert torch.isfinite(a).all()
    # all views invalid: the network's output on OneBlob + a zero code per view, not zeros
    assert float(a[6].abs().max()) > 0 and float(a[0].abs().max()) > 0


def test_determinism_splits_and_out():
    from dns_slam_amd import ops
    s = setup()
    a = codes(s, 3, "fused")
    assert torch.equal(a, codes(s, 3, "fused"))
    parts = [codes(s, 3, "fused", s["pts"][i:j]) for i, j in ((0, 129), (129, 300), (300, P))]
    assert torch.equal(a, torch.cat(parts, 0))
    for tile in (32, 64, 128):                                         # every tile size: 22, 11 and 6 tiles, the last one partial
        assert torch.equal(a, codes(s, 3, "fused", tile=tile)), tile
        parts = [codes(s, 3, "fused", s["pts"][i:j], tile=tile) for i, j in ((0, 129), (129, 300), (300, P))]
        assert torch.equal(a, torch.cat(parts, 0)), tile
    with pytest.raises(ValueError):
        codes(s, 3, "fused", tile=48)
    org = torch.inverse(s["w2c"].to(DEV))[:, :3, 3].contiguous()       # the origins handed over, as render_frame does
    assert torch.equal(a, codes(s, 3, "fused", origins=org))
    assert torch.equal(codes(s, 3, "launches"), codes(s, 3, "launches", origins=org))
    assert torch.equal(codes(s, 3, None), codes(s, 3, ops.FRAME_CODES_DEFAULT))
    big = torch.full((P + 11, 32), 7.0, device=DEV)
    r = codes(s, 3, "fused", out=big[5:5 + P])
    assert r.data_ptr() == big[5:5 + P].data_ptr() and torch.equal(big[5:5 + P], a)
    assert bool((big[:5] == 7.0).all()) and bool((big[5 + P:] == 7.0).all())
    wide = torch.full((P, 80), 7.0, device=DEV)
    codes(s, 3, "fused", out=wide[:, 16:48])
    assert torch.equal(wide[:, 16:48], a) and bool((wide[:, :16] == 7.0).all()) and bool((wide[:, 48:] == 7.0).all())
    odd = torch.full((P, 37), 7.0, device=DEV)                         # rows the kernel cannot address: through a copy
    codes(s, 3, "fused", out=odd[:, 3:35])
    assert torch.equal(odd[:, 3:35], a) and bool((odd[:, :3] == 7.0).all())
    assert ops.frame_codes(s["pts"][:0].to(DEV), s["w2c"].to(DEV), s["nhwc"], s["cam"], H, W, s["dec"].merge).shape == (0, 32)


@pytest.mark.parametrize("net", [(32, 1), (64, 2)])
def test_keep(net):
    s = setup(*net)
    R = 3
    g = torch.Generator().manual_seed(5)
    keep = (torch.rand(P, generator=g) < 0.6).to(DEV)
    full = codes(s, R, "fused")
    a = codes(s, R, "fused", keep=keep)
    assert bool((a[~keep] == 0).all()) and torch.equal(a[keep], full[keep])
    assert torch.equal(a, codes(s, R, "fused", keep=keep.to(torch.uint8)))
    assert_close(a.cpu(), codes(s, R, "launches", keep=keep).cpu(), what="frame_codes keep: fused vs launches")
    # a NaN in one map pixel: the points that read it are the rows it reaches in the unmasked call
    bad = s["nhwc"].clone()
    bad[0, 6, 8, :] = float("nan")
    readers = torch.isnan(codes(s, R, "fused", nhwc=bad)).any(1)
    n_read = int(readers.sum())
    print(f"net {net}: {n_read} of {P} points read the planted pixel")
    assert 0 < n_read < P
    # ... read by dropped points only: no NaN anywhere, the dropped rows zero, the rest untouched
    only_dropped = codes(s, R, "fused", nhwc=bad, keep=~readers)
    assert torch.isfinite(only_dropped).all()
    assert bool((only_dropped[readers] == 0).all()) and torch.equal(only_dropped[~readers], full[~readers])
    # ... read by kept, valid pairs: in exactly the rows where the launches have it
    keep2 = keep | readers
    f2, l2 = codes(s, R, "fused", nhwc=bad, keep=keep2), codes(s, R, "launches", nhwc=bad, keep=keep2)
    assert torch.equal(torch.isnan(f2).any(1), readers) and bool(torch.isnan(f2[readers]).all())
    # (assert_close's element-wise criterion compares non-finites in place, its scale-relative one is NaN on them: the places
    #  are compared here, element by element, and the finite rows go through assert_close)
    assert torch.equal(torch.isnan(f2), torch.isnan(l2)) and torch.equal(torch.isinf(f2), torch.isinf(l2))
    assert_close(f2[~readers].cpu(), l2[~readers].cpu(), what="frame_codes keep with a NaN pixel: fused vs launches")


def test_refusals():
    from dns_slam_amd import ops
    from dns_slam_amd.mapping import Mapper
    s = setup()
    mapper = Mapper(s["cfg"], s["dec"], s["bound"], s["cam"], device=DEV)
    fr_, i = s["frames"], 2
    refer = {"stem": s["nhwc"], "est_c2w": s["c2w"]}
    with pytest.raises(ValueError, match="exclusive"):
        mapper.render_frame(fr_["gt_color"][i], fr_["gt_depth"][i], fr_["gt_label"][i], fr_["est_c2w"][i],
                            features=torch.zeros(H * W, 47, 32, device=DEV), refer_frames=refer)
    half = setup(dtype="fp16")
    with pytest.raises(ValueError, match="fused"):
        codes(half, 3, "fused")
    odd = setup(pixel_dim=62)
    with pytest.raises(ValueError, match="fused"):
        codes(odd, 3, "fused", nhwc=s["nhwc"][..., :62].contiguous())
    with pytest.raises(ValueError):
        codes(s, 3, "sideways")
    with pytest.raises(ValueError):
        codes(s, 3, "fused", keep=torch.ones(P - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.frame_codes(s["pts"], s["w2c"], s["nhwc"].cpu(), s["cam"], H, W, s["dec"].merge)      # CPU tensors
    # left at its default, a shape the kernel does not take goes to the launches without comment
    assert torch.equal(codes(half, 3, None), codes(half, 3, "launches"))
