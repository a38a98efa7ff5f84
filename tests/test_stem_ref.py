"""CPU: the float64 restatement of the image stem (tests/stem_ref.py) against the reference module's own outputs
(tests/golden/stem.npz, written by tests/golden/make_golden_stem.py), and ``encoder.ResNet(backend="torch")`` in both ``bn`` modes
against the restatement's bounds."""
import os

import numpy as np
import pytest
import torch

import stem_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem.npz")


def _golden():
    g = np.load(GOLDEN)
    params = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    params["eps"] = float(g["eps"])
    return torch.from_numpy(g["images"]), params, torch.from_numpy(g["y_train"]), torch.from_numpy(g["y_eval"])


def _state_dict(params):
    return {k: v for k, v in params.items() if k != "eps"}


@pytest.mark.parametrize("batch_stats", [True, False])
def test_restatement_equals_the_reference_module(batch_stats):
    """stem_ref on the golden input = the reference's ResNet(BasicBlock, [2,2,2,2]) in float64, as built (train mode) and in
    eval(), to 1e-12 relative."""
    images, params, y_train, y_eval = _golden()
    assert images.shape == (1, 2, 13, 18, 3) and y_train.shape == (1, 2, 64, 7, 9)
    y, bound = stem_ref.stem_ref(images[0], params, batch_stats)
    want = (y_train if batch_stats else y_eval)[0].permute(0, 2, 3, 1)
    err = (y - want).abs().max() / want.abs().max()
    print(f"batch_stats {batch_stats}: max error {float(err):.3e} of the largest value")
    assert float(err) <= 1e-12
    assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((bound > 0).all()) and float(want.abs().max()) > 0.5
    # the two modes are different functions: the golden outputs differ by far more than any bound
    assert float((y_train - y_eval).abs().max()) > 0.1


@pytest.mark.parametrize("bn", ["batch", "frozen"])
def test_torch_backend_is_inside_the_bounds(bn):
    from dns_slam_amd.encoder import ResNet
    images, params, _, _ = _golden()
    enc = ResNet(weights=_state_dict(params), backend="torch", bn=bn)
    rm, rv = enc.conv_blocks.bn1.running_mean.clone(), enc.conv_blocks.bn1.running_var.clone()
    got = enc(images)
    assert got.shape == (1, 2, 64, 7, 9) and got.dtype == torch.float32
    y, bound = stem_ref.stem_ref(images[0], params, bn == "batch")
    ratio = ((got[0].permute(0, 2, 3, 1).double() - y).abs() / bound).max()
    print(f"bn {bn}: worst error / bound {float(ratio):.4f}")
    assert float(ratio) <= 1.0
    # no running-statistics update in either mode
    assert torch.equal(enc.conv_blocks.bn1.running_mean, rm) and torch.equal(enc.conv_blocks.bn1.running_var, rv)
    assert not enc.training


def test_frozen_default_is_the_module_as_it_was():
    """ResNet() and ResNet(backend='torch', bn='frozen') are the former module bit for bit: conv1 -> bn1 in eval() -> ReLU of the
    same seeded parameters."""
    import torch.nn.functional as F
    from dns_slam_amd.encoder import ResNet
    images = stem_ref.random_images(3, 4, 21, 30, "unit").reshape(2, 2, 21, 30, 3)
    a, b = ResNet(seed=5), ResNet(seed=5, backend="torch", bn="frozen")
    assert a.backend == "torch" and a.bn == "frozen"
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    st = a.conv_blocks
    with torch.no_grad():
        x = images.flatten(0, 1).permute(0, 3, 1, 2)
        want = F.relu(F.batch_norm(st.conv1(x), st.bn1.running_mean, st.bn1.running_var, st.bn1.weight, st.bn1.bias, False, 0.1,
                                   st.bn1.eps)).reshape(2, 2, 64, 11, 15)
    assert torch.equal(a(images), want) and torch.equal(b(images), want)
    with pytest.raises(ValueError):
        ResNet(backend="triton")
    with pytest.raises(ValueError):
        ResNet(bn="running")


def test_bounds_reject_wrong_arithmetic():
    """What the bounds are for: an unbiased variance, a product carried to f16 precision and a misplaced tap all fall outside."""
    images, params, _, _ = _golden()
    x = images[0]
    y, bound = stem_ref.stem_ref(x, params, True)
    c, _ = stem_ref.conv64(x, params["conv1.weight"])
    gamma, beta = params["bn1.weight"].double(), params["bn1.bias"].double()
    mean = c.mean((0, 1, 2))
    unbiased = torch.relu(gamma * (c - mean) / torch.sqrt(c.var((0, 1, 2), unbiased=True) + params["eps"]) + beta)
    assert float(((unbiased - y).abs() / bound).max()) > 1.0
    yf, bf = stem_ref.stem_ref(x, params, False)
    half = dict(params)
    half["conv1.weight"] = params["conv1.weight"].half().float()
    assert float(((stem_ref.stem_ref(x, half, False)[0] - yf).abs() / bf).max()) > 1.0
    shifted = dict(params)
    shifted["conv1.weight"] = torch.roll(params["conv1.weight"], 1, 3)
    assert float(((stem_ref.stem_ref(x, shifted, False)[0] - yf).abs() / bf).max()) > 1.0
