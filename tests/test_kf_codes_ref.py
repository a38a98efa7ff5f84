"""CPU: the torch restatement of get_2d_feature (tests/kf_codes_ref.py) on a case worked out by hand and against a plain double
loop.  The GPU tests of the keyframe codes (tests/test_gpu_mesh_stem.py) compare against this restatement."""
import torch

import kf_codes_ref


def _hand_case():
    """One keyframe at the identity pose, 8 x 10 image, fx = fy = 4, cx = 5, cy = 4.  A camera-frame point (x, y, z) with z < 0
    projects, with the reference's x flip, to u = (fx * -x + cx z) / z, v = (fy y + cy z) / z."""
    cam = {"H": 8, "W": 10, "fx": 4.0, "fy": 4.0, "cx": 5.0, "cy": 4.0}
    depth = torch.full((8, 10), 2.0)
    depth[4, 7] = 0.0                                          # a hole at pixel (iv, iu) = (4, 7)
    kf = {"est_c2w": torch.eye(4), "gt_color": torch.zeros(8, 10, 3), "gt_label": torch.full((8, 10), 3.0), "gt_depth": depth}
    C = 4
    encoder = lambda img: torch.arange(1.0, C + 1).reshape(1, 1, C, 1, 1).expand(1, 1, C, 4, 5).contiguous()
    merge_fn = lambda p, o, ft: ft[0]
    # on the optical axis: u = cx = 5, v = cy = 4 for every z < 0
    pts = torch.tensor([[0.0, 0.0, -2.0],                     # on the surface
                        [0.0, 0.0, -1.9],                     # 0.95 d: the front limit itself is inside
                        [0.0, 0.0, -2.1],                     # 1.05 d: the back limit itself is inside
                        [0.0, 0.0, -1.89],                    # in front of the band
                        [0.0, 0.0, -2.11],                    # behind the band
                        [0.0, 0.0, 2.0],                      # behind the camera
                        [1.0, 0.0, -2.0],                     # u = (4 * -1 + 5 * -2) / -2 = 7, v = 4: the depth hole
                        [10.0, 0.0, -2.0]])                   # u = 25: outside the image
    return pts, [kf], cam, encoder, merge_fn, C


def test_hand_case():
    pts, kfs, cam, encoder, merge_fn, C = _hand_case()
    d = torch.tensor(2.0)
    assert float(-pts[1, 2]) == float(d * 0.95) and float(-pts[2, 2]) == float(d * 1.05)   # the fp32 products themselves
    code, label, count, mask, near = kf_codes_ref.get_2d_feature(pts, kfs, cam, encoder, merge_fn, C)
    want = torch.tensor([1, 1, 1, 0, 0, 0, 0, 0])
    assert count.tolist() == want.float().tolist()
    assert mask.tolist() == [want.bool().tolist()]
    feat = torch.arange(1.0, C + 1)
    for i in range(8):
        # (the up-sampled constant map is the constant up to the rounding of the two bilinear weights)
        assert torch.allclose(code[i], feat if want[i] else torch.zeros(C), rtol=1e-6, atol=0), i
        assert want[i] or torch.equal(code[i], torch.zeros(C))
    # the label needs only `seen`: the hole and the points outside the band carry it, the two unseen points do not
    assert label.tolist() == [3.0, 3.0, 3.0, 3.0, 3.0, 0.0, 3.0, 0.0]
    assert near[1] and near[2] and not near[0] and not near[5]


def test_mean_over_two_keyframes():
    pts, kfs, cam, encoder, merge_fn, C = _hand_case()
    second = dict(kfs[0])
    second["gt_depth"] = torch.full((8, 10), 2.2)             # band [2.09, 2.31]: sees points 2 and 4 only
    enc2 = lambda img: (img.mean() + torch.arange(1.0, C + 1)).reshape(1, 1, C, 1, 1).expand(1, 1, C, 4, 5).contiguous()
    second["gt_color"] = torch.full((8, 10, 3), 2.0)           # second keyframe's map = first + 2
    code, _, count, mask, _ = kf_codes_ref.get_2d_feature(pts, [kfs[0], second], cam, enc2, merge_fn, C)
    assert count.tolist() == [1, 1, 2, 0, 1, 0, 0, 0]
    feat = torch.arange(1.0, C + 1)
    close = lambda a, b_: torch.allclose(a, b_, rtol=1e-6, atol=0)
    assert close(code[2], feat + 1.0) and close(code[4], feat + 2.0) and close(code[0], feat)
    assert mask[1].tolist() == [False, False, True, False, True, False, False, False]


def test_pair_count_equals_double_loop():
    from dns_slam_amd import synthetic
    cam = synthetic.camera(H=60, W=80, fx=60.0, fy=60.0)
    bound, cam, frames = synthetic.make_scene(3, cam=cam, seed=3)
    kfs = [{"est_c2w": frames["est_c2w"][i], "gt_label": frames["gt_label"][i], "gt_depth": frames["gt_depth"][i],
            "gt_color": frames["gt_color"][i]} for i in range(3)]
    g = torch.Generator().manual_seed(11)
    b = bound.float()
    P = 1500
    pts = (torch.rand(P, 3, generator=g) * 1.1 - 0.05) * (b[:, 1] - b[:, 0]) + b[:, 0]
    encoder = lambda img: torch.ones(1, 1, 4, 30, 40)
    _, _, count, mask, near = kf_codes_ref.get_2d_feature(pts, kfs, cam, encoder, lambda p, o, ft: ft[0], 4)
    loops = kf_codes_ref.pair_count_loops(pts, kfs, cam)
    assert torch.equal(mask.sum(0), count.long())
    ok = ~near
    assert float(near.float().mean()) <= 0.05 and int(loops.sum()) > 20    # the flag excuses few points: the cap the GPU test holds
    assert torch.equal(loops[ok], count.long()[ok])
