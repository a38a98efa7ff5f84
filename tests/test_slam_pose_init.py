"""CPU: slam.pose_init (slams/tracking.py:216-227) against the constant-speed rule's fp32 formula, exactly."""
import math

import torch

from dns_slam_amd import synthetic
from dns_slam_amd.slam import pose_init


def _poses():
    a = synthetic.make_pose(0.30, radius=0.50)
    b = synthetic.make_pose(0.37, radius=0.52)
    b[:3, 3] += torch.tensor([0.01, -0.02, 0.005])
    return a, b


def test_constant_speed_is_the_fp32_formula():
    prev2, prev = _poses()
    for idx in (3, 4, 100):
        got = pose_init(prev, prev2, idx)
        pre = prev.float()
        want = (pre @ prev2.float().inverse()) @ pre
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert not torch.equal(got, prev)
    # the motion prev2 -> prev applied once more: a rotation about z by 0.07 rad and the same step
    step = pose_init(prev, prev2, 3) @ torch.inverse(prev)
    assert torch.allclose(step, prev @ torch.inverse(prev2), atol=1e-5)
    assert abs(math.atan2(float(step[1, 0]), float(step[0, 0])) - 0.07) < 1e-4


def test_float64_estimates_are_rounded_first():
    prev2, prev = (p.double() * (1.0 + 1e-9) for p in _poses())
    got = pose_init(prev, prev2, 5)
    pre = prev.float()
    assert got.dtype == torch.float32 and torch.equal(got, (pre @ prev2.float().inverse()) @ pre)


def test_first_frames_take_the_previous_pose():
    prev2, prev = _poses()
    for idx in (0, 1, 2):
        assert torch.equal(pose_init(prev, prev2, idx), prev)
    assert torch.equal(pose_init(prev, prev2, 7, const_speed=False), prev)
