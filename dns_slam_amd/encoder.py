"""Mirror of reference models/encoder.py:4-17 (``ResNet``) -- the frozen image stem of the 2-D feature branch.

Only the stem the reference actually executes (models/layers.py:56-58,95-98: conv 7x7 stride 2 + batch-norm + ReLU; the
residual stages are commented out there).  It runs ONCE per ``optimize()`` / per tracked frame, outside the iteration
loop (slams/mapping.py:846, slams/tracking.py:293-296).  ``backend="torch"`` (the default) runs it on stock PyTorch-ROCm
convolution; ``backend="hip"`` on the project's own kernels (csrc/stem.hip), which write the channels-last maps the consumers
read.  ``bn`` chooses the normalisation, and with it WHICH CODES A CHECKPOINT EXPECTS: ``"frozen"`` (the default) is
``nn.BatchNorm2d`` in eval() mode, the running statistics; ``"batch"`` is what the reference actually computes -- it builds
``ResNet()`` (slams/mapping.py:33, slams/tracking.py:30) and never calls ``.eval()``, so its ``bn1`` normalises with the mean and
biased variance of the images of that very call (all B*N of them).  A map trained by the reference expects ``bn="batch"``.  The reference
downloads ImageNet ResNet-18 weights at construction (layers.py:125); there is no network here: pass ``weights`` (a
state dict or a path holding ``conv1.weight``, ``bn1.*``) or get the reference's own fallback initialisation
(layers.py:70-76: He-normal conv, unit batch-norm)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class _Stem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        n = 7 * 7 * 64
        self.conv1.weight.data.normal_(0, math.sqrt(2.0 / n))
        self.bn1.weight.data.fill_(1)
        self.bn1.bias.data.zero_()

    def forward(self, x):
        return self.relu(self.bn1(self.conv1(x)))


class ResNet(nn.Module):
    def __init__(self, weights=None, seed=0, backend="torch", bn="frozen"):
        """``backend``: "torch" (stock convolution; runs on the CPU too) or "hip" (``ops.stem_forward``, GPU only).  ``bn``: "frozen"
        (running statistics, eval() mode) or "batch" (the statistics of the call's own B*N images, biased variance: the reference's
        actual behaviour; the running statistics are neither read nor updated).  The defaults are the module as it always was."""
        super().__init__()
        if backend not in ("torch", "hip"):
            raise ValueError(f"ResNet: backend must be 'torch' or 'hip', got {backend!r}")
        if bn not in ("frozen", "batch"):
            raise ValueError(f"ResNet: bn must be 'frozen' or 'batch', got {bn!r}")
        self.backend, self.bn = backend, bn
        g = torch.random.get_rng_state()
        torch.manual_seed(seed)
        self.conv_blocks = _Stem()
        torch.random.set_rng_state(g)
        if weights is not None:
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            own = self.conv_blocks.state_dict()
            own.update({k: v for k, v in sd.items() if k in own})
            self.conv_blocks.load_state_dict(own)
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    @torch.no_grad()
    def forward_channels_last(self, images, out=None):
        """``backend="hip"`` only: images [n, H, W, 3] -> the channels-last maps [n, h, w, 64] (``out``: written in place)."""
        if self.backend != "hip":
            raise ValueError("ResNet.forward_channels_last needs backend='hip'")
        from . import ops
        st = self.conv_blocks
        return ops.stem_forward(images.float().contiguous(), st.conv1.weight, st.bn1.weight, st.bn1.bias, st.bn1.running_mean,
                                st.bn1.running_var, st.bn1.eps, batch_stats=self.bn == "batch", out=out)

    @torch.no_grad()
    def forward(self, images):
        """images [B, N, H, W, 3] -> features [B, N, 64, H/2, W/2] (models/encoder.py:9-17).  With ``backend="hip"`` the result is
        a permuted view of channels-last storage [B, N, h, w, 64]: ``common.features_channels_last`` and MapStep's re-layout find
        it contiguous already and copy nothing."""
        B, N = images.shape[:2]
        if self.backend == "hip":
            f = self.forward_channels_last(images.flatten(0, 1))
            return f.reshape(B, N, *f.shape[1:]).permute(0, 1, 4, 2, 3)
        x = images.flatten(0, 1).permute(0, 3, 1, 2)
        if self.bn == "batch":
            st = self.conv_blocks
            c = st.conv1(x)
            # PyTorch's own batch-norm kernels, not the vendor library's: its train-mode routine crashed the process on a
            # [1, 64, 35, 75] map (tests/test_gpu_stem.py); the flag has no effect on the CPU
            lib_on = torch.backends.cudnn.enabled
            torch.backends.cudnn.enabled = False
            try:
                f = torch.relu(F.batch_norm(c, None, None, st.bn1.weight, st.bn1.bias, True, 0.0, st.bn1.eps))
            finally:
                torch.backends.cudnn.enabled = lib_on
        else:
            f = self.conv_blocks(x)
        return f.reshape(B, N, *f.shape[1:])
