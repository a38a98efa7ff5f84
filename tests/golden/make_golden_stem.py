"""Golden vectors of the image stem, from the IMPORTED reference module.

Run once, from the reference's root, in the build container only (the reference never travels):

    cd <reference> && PYTHONDONTWRITEBYTECODE=1 python <repository>/tests/golden/make_golden_stem.py

``models/layers.py`` is imported as it lies and ``ResNet(BasicBlock, [2, 2, 2, 2])`` -- what ``ResNet18(pretrained=False)`` builds, the
stem alone being live (layers.py:56-58,95-98) -- is constructed without the download.  ``bn1``'s weight, bias and running statistics
are randomised so that no term is trivial, the module is widened to float64 and run on a [1, 2, 13, 18, 3] image pair through the
reference's own ``models/encoder.py`` forward (flatten, permute, reshape), first AS BUILT -- train mode, which is how the reference
runs it: slams/mapping.py:33 and slams/tracking.py:30 construct ``ResNet()`` and nothing ever calls ``.eval()`` -- and then in
``.eval()``.  Modules the container lacks get in-memory placeholders, as in make_golden_slam.py.

Output: ``stem.npz`` -- the input, the state dict BEFORE the train-mode call (which updates the running statistics in the module; the
eval-mode output uses the stored ones, restored before it) and both float64 outputs, as plain arrays.
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.getcwd())
try:
    import models.layers as RL      # the reference's
except ImportError as exc:          # a module the container lacks and the stem never touches
    sys.modules[exc.name] = types.ModuleType(exc.name)
    import models.layers as RL


def encoder_forward(conv_blocks, images):
    """models/encoder.py:9-17, whose class cannot be constructed without the download."""
    B, N = images.shape[:2]
    x = images.flatten(0, 1).permute(0, 3, 1, 2)
    features = conv_blocks(x)
    _, C, H, W = features.shape
    return features.reshape(B, N, C, H, W)


def main():
    torch.manual_seed(20)
    net = RL.ResNet(RL.BasicBlock, [2, 2, 2, 2])
    assert net.training, "the reference's stem is built in train mode"
    with torch.no_grad():
        net.bn1.weight.copy_((0.5 + torch.rand(64)) * torch.where(torch.rand(64) < 0.25, -1.0, 1.0))
        net.bn1.bias.copy_(torch.randn(64) * 0.3)
        net.bn1.running_mean.copy_(torch.randn(64) * 0.2)
        net.bn1.running_var.copy_(0.05 + torch.rand(64) * 2.0)
    images = torch.rand(1, 2, 13, 18, 3)
    net = net.double()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        y_train = encoder_forward(net, images.double())
        net.load_state_dict(state)
        y_eval = encoder_forward(net.eval(), images.double())
    arrays = {"images": images.numpy(), "y_train": y_train.numpy(), "y_eval": y_eval.numpy(), "eps": np.float64(net.bn1.eps)}
    for k, v in state.items():
        if k.startswith(("conv1.", "bn1.")) and k != "bn1.num_batches_tracked":
            arrays["sd." + k] = v.float().numpy()           # the fp32 values the module was built with, widened exactly above
    np.savez_compressed(os.path.join(OUT, "stem.npz"), **arrays)
    print({k: (v.shape, v.dtype) for k, v in arrays.items()})


if __name__ == "__main__":
    main()
