"""GPU: the image stem as the project's own kernels (csrc/stem.hip: ops.stem_forward, encoder.ResNet(backend="hip"),
Mesher.keyframe_stem's out= path) against the float64 restatement tests/stem_ref.py and its derived bounds, in both normalisation
modes.  The stock composition ResNet(backend="torch") is held to the same bounds on the same inputs, so that a failure cannot be the
bound's fault.  No element is skipped anywhere."""
import functools

import pytest
import torch

import stem_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, H, W).  The last one is this file's choice: the workgroup tile is 8 x 32 output pixels, so 35 x 139 -> 18 x 70 outputs has two
# full tiles plus a remainder in each axis, 2 x 3 x 3 = 18 partial-sum rows, and 645 KB of output.
SHAPES = [(1, 1, 1), (1, 2, 7), (2, 13, 18), (3, 37, 50), (1, 70, 150), (2, 35, 139)]
KINDS = ["unit", "byte", "flat"]
WEIGHTS = ["he", "wide"]


@functools.lru_cache(maxsize=None)
def _case(shape, kind, weight):
    """Inputs, parameters and the float64 references of both modes, computed once and shared."""
    n, H, W = shape
    seed = 1000 * SHAPES.index(shape) + 10 * KINDS.index(kind) + WEIGHTS.index(weight) if shape in SHAPES else 7
    params = stem_ref.random_params(seed, weight)
    images = stem_ref.random_images(seed + 1, n, H, W, kind)
    ref = {False: stem_ref.stem_ref(images, params, False)}
    if n * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) > 1:
        ref[True] = stem_ref.stem_ref(images, params, True)
    return images, params, ref


def _dev(params):
    return [params[k].to(DEV) for k in ("conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var")]


def _hip(images, params, batch_stats, **kw):
    from dns_slam_amd import ops
    return ops.stem_forward(images.to(DEV), *_dev(params), batch_stats=batch_stats, **kw)


def _encoder(params, backend, bn):
    from dns_slam_amd.encoder import ResNet
    return ResNet(weights={k: v for k, v in params.items() if k != "eps"}, backend=backend, bn=bn).to(DEV)


def _ratio(got, ref):
    y, bound = ref
    assert got.shape == y.shape and got.dtype == torch.float32
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all())
    return float(((g - y).abs() / bound).max())


@pytest.mark.parametrize("weight", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_modes_inside_the_bounds(shape, kind, weight):
    """Frozen and batch mode of the kernels, and of the stock composition on the GPU, element-wise inside the derived bounds."""
    images, params, ref = _case(shape, kind, weight)
    for batch_stats in (False, True):
        if batch_stats not in ref:                                     # (1,1,1): batch statistics of one value
            with pytest.raises(ValueError):
                _hip(images, params, True)
            continue
        got = _hip(images, params, batch_stats)
        r_hip = _ratio(got, ref[batch_stats])
        if batch_stats:
            again = _hip(images, params, True, batch_apply="recompute")
            assert torch.equal(got, again), "in-place and recomputed normalisation differ"
        enc = _encoder(params, "torch", "batch" if batch_stats else "frozen")
        r_stock = _ratio(enc(images.to(DEV)[None])[0].permute(0, 2, 3, 1), ref[batch_stats])
        print(f"{shape} {kind} {weight} batch_stats={batch_stats}: error / bound hip {r_hip:.4f}, stock {r_stock:.4f}")
        assert r_stock <= 1.0, "the stock composition is outside the bound"
        assert r_hip <= 1.0


def test_batch_statistics_over_more_rows_than_one_reduction_level():
    """300 images of 1 x 3 pixels: 300 partial-sum rows, which the first reduction level adds in runs of two."""
    params = stem_ref.random_params(41, "wide")
    images = stem_ref.random_images(42, 300, 1, 3, "unit")
    got = _hip(images, params, True)
    r = _ratio(got, stem_ref.stem_ref(images, params, True))
    print(f"300 x 1 x 3: error / bound {r:.4f}")
    assert r <= 1.0
    assert torch.equal(got, _hip(images, params, True, batch_apply="recompute"))


def test_bit_identical_across_calls_batches_and_positions():
    images, params, _ = _case((3, 37, 50), "unit", "he")
    for batch_stats in (False, True):
        a, b = _hip(images, params, batch_stats), _hip(images, params, batch_stats)
        assert torch.equal(a, b), f"two calls differ (batch_stats={batch_stats})"
    whole = _hip(images, params, False)
    alone = _hip(images[2:3], params, False)
    assert torch.equal(whole[2:3], alone), "an image's map depends on its batch or position"
    for bn in ("frozen", "batch"):
        enc = _encoder(params, "hip", bn)
        x = images.to(DEV)
        a, b = enc(x[None]), enc(x[:, None])                           # [B,N] = [1,3] and [3,1]: the batch is the whole call
        assert a.shape == (1, 3, 64, 19, 25) and b.shape == (3, 1, 64, 19, 25)
        assert torch.equal(a[0], b[:, 0]), f"[1,3] and [3,1] differ (bn={bn})"
        assert torch.equal(a[0].permute(0, 2, 3, 1), _hip(images, params, bn == "batch"))


def test_out_slice_of_a_stack_leaves_its_neighbours():
    images, params, ref = _case((2, 13, 18), "unit", "he")
    for batch_stats in (False, True):
        stack = torch.full((3, 2, 7, 9, 64), -777.0, device=DEV)
        ret = _hip(images, params, batch_stats, out=stack[1])
        assert ret.data_ptr() == stack[1].data_ptr()
        assert bool((stack[0] == -777.0).all()) and bool((stack[2] == -777.0).all())
        assert torch.equal(stack[1], _hip(images, params, batch_stats))
    one = _case((1, 13, 18), "unit", "he")[0]
    stack = torch.full((3, 7, 9, 64), -777.0, device=DEV)
    _hip(one, params, False, out=stack[1:2])
    assert bool((stack[0] == -777.0).all()) and bool((stack[2] == -777.0).all()) and bool((stack[1] != -777.0).all())


def test_nan_and_inf_pixels_stay_in_their_windows():
    """One NaN pixel and one Inf pixel in a 13 x 18 image, frozen mode: exactly the outputs whose 7 x 7 window covers the NaN pixel
    are NaN in every channel; the Inf pixel gives the non-finite values of the float64 restatement (NaN where products of both
    signs meet, else an infinity or its ReLU); every other element keeps its bits, and no NaN becomes 0."""
    images, params, _ = _case((1, 13, 18), "unit", "wide")
    clean = _hip(images, params, False)
    bad = images.clone()
    bad[0, 2, 3, :] = float("nan")
    bad[0, 10, 14, 1] = float("inf")
    got = _hip(bad, params, False).cpu()
    want, _ = stem_ref.stem_ref(bad, params, False)
    oy, ox = torch.meshgrid(torch.arange(7), torch.arange(9), indexing="ij")
    covers = lambda iy, ix: ((2 * oy - 3 <= iy) & (iy <= 2 * oy + 3) & (2 * ox - 3 <= ix) & (ix <= 2 * ox + 3))
    nan_win, inf_win = covers(2, 3), covers(10, 14)
    assert int(nan_win.sum()) == 12 and int(inf_win.sum()) == 9 and not bool((nan_win & inf_win).any())
    assert bool(torch.isnan(got[0][nan_win]).all()), "a NaN was laundered"
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert bool((torch.isnan(got[0]).any(-1) <= (nan_win | inf_win)).all())
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and int(torch.isinf(got).sum()) > 0
    untouched = ~(nan_win | inf_win)
    assert torch.equal(got[0][untouched], clean.cpu()[0][untouched])
    fin = torch.isfinite(want)
    assert bool(((got.double() - want)[fin].abs() <= 1e-3).all())


def test_argument_errors():
    from dns_slam_amd import ops
    images, params, _ = _case((2, 13, 18), "unit", "he")
    x, p = images.to(DEV), _dev(params)
    ok = ops.stem_forward(x, *p)
    assert ok.shape == (2, 7, 9, 64)
    bad_calls = [
        lambda: ops.stem_forward(x.double(), *p),                                      # dtype
        lambda: ops.stem_forward(x.half(), *p),
        lambda: ops.stem_forward(x.cpu(), *p),                                         # device
        lambda: ops.stem_forward(x, p[0].cpu(), *p[1:]),
        lambda: ops.stem_forward(x[0], *p),                                            # rank
        lambda: ops.stem_forward(x[None], *p),
        lambda: ops.stem_forward(x.permute(0, 3, 1, 2).contiguous(), *p),              # channel count (NCHW handed in)
        lambda: ops.stem_forward(torch.zeros(2, 13, 18, 4, device=DEV), *p),
        lambda: ops.stem_forward(x, p[0][:32].contiguous(), *p[1:]),                   # weight shape
        lambda: ops.stem_forward(x, p[0], p[1][:32].contiguous(), *p[2:]),
        lambda: ops.stem_forward(x.permute(0, 2, 1, 3), *p),                           # non-contiguous images
        lambda: ops.stem_forward(x[:, :, ::2], *p),
        lambda: ops.stem_forward(x, *p, out=torch.empty(2, 7, 9, 32, device=DEV)),     # out of the wrong shape
        lambda: ops.stem_forward(x, *p, out=torch.empty(2, 64, 7, 9, device=DEV)),
        lambda: ops.stem_forward(x, *p, out=torch.empty(2, 7, 9, 128, device=DEV)[..., ::2]),   # non-contiguous out
        lambda: ops.stem_forward(x, *p, out=torch.empty(2, 7, 9, 64, device=DEV, dtype=torch.float64)),
        lambda: ops.stem_forward(x, *p, out=torch.empty(2, 7, 9, 64)),
        lambda: ops.stem_forward(torch.rand(1, 1, 1, 3, device=DEV), *p, batch_stats=True),     # one value per channel
        lambda: ops.stem_forward(torch.rand(1, 2, 2, 3, device=DEV), *p, batch_stats=True),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    assert ops.stem_forward(torch.rand(1, 1, 1, 3, device=DEV), *p).shape == (1, 1, 1, 64)
    assert ops.stem_forward(torch.rand(1, 2, 3, 3, device=DEV), *p, batch_stats=True).shape == (1, 1, 2, 64)


def test_hip_encoder_output_is_read_in_place():
    """forward() returns the reference's logical shape as a view of channels-last storage: features_channels_last, and MapStep's
    re-layout expression, copy nothing; Mapper.optimize's .clone() keeps the layout."""
    from dns_slam_amd import common
    images, params, _ = _case((3, 37, 50), "unit", "he")
    enc = _encoder(params, "hip", "frozen")
    f = enc(images.to(DEV).reshape(1, 3, 37, 50, 3))
    assert f.shape == (1, 3, 64, 19, 25)
    assert common.features_channels_last(f[0]).data_ptr() == f.data_ptr()
    assert f.permute(0, 1, 3, 4, 2).is_contiguous()
    assert f.detach().float().permute(0, 1, 3, 4, 2).contiguous().data_ptr() == f.data_ptr()
    c = f.clone().detach()
    assert c.stride() == f.stride() and common.features_channels_last(c[0]).data_ptr() == c.data_ptr()
    assert torch.equal(common.features_channels_last(c[0]), _hip(images, params, False))
    stock = _encoder(params, "torch", "frozen")(images.to(DEV).reshape(1, 3, 37, 50, 3))
    assert float((stock - f).abs().max()) <= 1e-4 * float(stock.abs().max())


def test_keyframe_stem_writes_the_stack_in_place():
    """Mesher.keyframe_stem with a backend='hip' encoder = ops.stem_forward per keyframe, bit for bit (K = 5, batch = 2), and
    within rounding of the stock encoder's stack."""
    import test_gpu_mesh as tm
    from dns_slam_amd.meshing import Mesher
    cfg, bound, cam, frames, mapper = tm._mapper()
    kfs = tm._keyframes(frames)[:5]
    assert len(kfs) == 5
    params = stem_ref.random_params(77, "he")
    mesher = Mesher(cfg, mapper)
    for bn in ("frozen", "batch"):
        stack = mesher.keyframe_stem(kfs, _encoder(params, "hip", bn), batch=2)
        H, W = kfs[0]["gt_color"].shape[:2]
        assert stack.shape == (5, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64) and stack.is_contiguous()
        for s in range(0, 5, 2):
            img = torch.stack([torch.as_tensor(k["gt_color"]).float() for k in kfs[s:s + 2]])
            if bn == "frozen":
                for j in range(img.shape[0]):
                    assert torch.equal(stack[s + j:s + j + 1], _hip(img[j:j + 1], params, False))
            else:
                assert torch.equal(stack[s:s + 2], _hip(img, params, True))
        stock = mesher.keyframe_stem(kfs, _encoder(params, "torch", bn), batch=2)
        assert float((stock - stack).abs().max()) <= 1e-4 * float(stock.abs().max())


def test_mapping_iteration_loss_with_the_hip_encoder():
    """One mapping iteration's forward loss on the keyframe scene of test_gpu_slam.py's optimize test (stem features feeding the
    2-D branch), same draws, stock and hip encoders in frozen mode: within 1e-4 relative."""
    import test_gpu_slam as ts
    from dns_slam_amd.encoder import ResNet
    from util import randomise_
    cfg, bound, cam, frames, dec, m = ts._setup(n_pixels=400)
    randomise_(dec.merge, 21)
    m.keyframe_selector = lambda color, depth, c2w, kfs, k: [1]
    for k in range(3):
        m.keyframe_list.append(5 * k)
        m.keyframe_dict.append({"gt_color": frames["gt_color"][k], "gt_depth": frames["gt_depth"][k], "gt_label": frames["gt_label"][k],
                                "gt_c2w": frames["gt_c2w"][k], "est_c2w": frames["est_c2w"][k].clone()})
    cur = (frames["gt_color"][3].to(DEV), frames["gt_depth"][3].to(DEV), frames["gt_label"][3].to(DEV), frames["gt_c2w"][3].to(DEV),
           frames["est_c2w"][3].to(DEV))
    idx, tf, rf = m.set_target_refer_frames(*cur)
    assert rf["gt_color"].shape[:2] == (3, 3)
    m.n_target_frame, m.is_BA = len(tf["gt_color"]), True
    m.set_decoder(tf)
    _, ql, Tl = m.set_optimizer(tf)
    prep = m.prepare_frames(tf)
    torch.manual_seed(9)
    pix, jit = m.draw_pixels(prep), m.draw_jitter()
    u_off, u_jit = torch.rand(3), torch.rand((1, 1, 1, 3))
    losses, codes = {}, {}
    for backend in ("torch", "hip"):
        enc = ResNet(seed=1, backend=backend).to(DEV)
        feats = enc(rf["gt_color"].to(DEV)).clone().detach()
        with torch.no_grad():
            s = m.get_target_samples(tf, ql, Tl, refer_frames=rf, features=feats, prep=prep, pix_idx=pix, jitter=jit)
            loss, _ = m.iteration_loss(s, smooth=True, u_offset=u_off, u_jitter=u_jit)
        losses[backend], codes[backend] = float(loss), s["features"]
    assert float(codes["torch"].abs().max()) > 0, "the 2-D code is identically zero: the stem does not reach the loss"
    print(f"loss stock {losses['torch']:.8f}, hip {losses['hip']:.8f}")
    assert abs(losses["hip"] - losses["torch"]) <= 1e-4 * abs(losses["torch"])
