"""GPU: full-frame rendering of a stem-trained map -- Mapper.render_frame(refer_frames=...), Mapper.vis_refer_frames and
evaluation.render_metrics(stem=...): the 2-D code computed chunk by chunk (ops.frame_codes) against the same render fed the whole
frame's code as one finished tensor (common.feature_matching on the same points)."""
import numpy as np
import pytest
import torch

from util import assert_close, randomise_

pytestmark = pytest.mark.gpu
DEV = "cuda"


def scene(H, W, f):
    """test_render_frame_matches_oracle_chunks' scene with a randomised Merge network and the image stem as the mapper's encoder."""
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd.encoder import ResNet
    from dns_slam_amd.mapping import Mapper
    cam = synthetic.camera(H=H, W=W, fx=f, fy=f)
    bound, cam, frames = synthetic.make_scene(4, cam=cam, seed=3)
    cfg = synthetic.default_cfg(n_pixels=200, hash_size=14, voxel_size=0.08, smooth_pts=10)
    dec = Decoder(cfg["model"], bound, n_class=8).to(DEV)
    mapper = Mapper(cfg, dec, bound, cam, device=DEV)
    mapper.set_decoder(frames)
    randomise_(dec, 5)
    with torch.no_grad():
        dec.pe_fn.grid_fn.params.mul_(2000.0)
    randomise_([mapper.fine_decoders.pool], 6)
    randomise_(dec.merge, 21)
    mapper.encoder = ResNet(seed=3).to(DEV)
    return mapper, frames, cam


def test_render_frame_with_refer_frames_equals_the_finished_code():
    from dns_slam_amd import ops
    from dns_slam_amd.common import feature_matching, get_quad_from_c2w
    H, W = 24, 32
    mapper, frames, cam = scene(H, W, 24.0)
    dec = mapper.decoder
    i, views = 2, [0, 1, 2]
    c2w = frames["est_c2w"][i]
    refer = {"gt_color": frames["gt_color"][views], "est_c2w": frames["est_c2w"][views]}
    torch.manual_seed(1)
    jit = mapper.draw_jitter(1)
    args = (frames["gt_color"][i], frames["gt_depth"][i], frames["gt_label"][i], c2w)
    # the whole small frame's code on the same points (render_frame's ray generation, same jitter)
    f = lambda t: t.to(DEV).float().contiguous()[None]
    res = ops.raygen_sample(get_quad_from_c2w(c2w).to(DEV)[None], c2w[:3, 3].to(DEV).float()[None], torch.arange(H * W, device=DEV),
                            f(args[0]), f(args[1]), f(args[2]), (mapper.fx, mapper.fy, mapper.cx, mapper.cy), mapper.bound,
                            (0, H, 0, W), H * W, mapper.t_uniform, jit[0], jit[1])
    pts, gt_depth, z = res[2], res[4], res[7]
    S = z.shape[1]
    maps = mapper.encoder(refer["gt_color"][None].to(DEV))[0]
    w2c = torch.inverse(refer["est_c2w"].to(DEV).float()).contiguous()
    K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])
    F = feature_matching(H, W, K, pts.reshape(-1, 3), w2c, maps, dec.merge).reshape(H * W, S, -1)
    assert float((F.abs().sum(-1) > 0).float().mean()) > 0.1
    d = gt_depth[:, None]
    mask = (1.0 - (z < d * 0.95).float()) * (1.0 - (z > d * 1.05).float()) * (d > 0.0).float()      # slams/mapping.py:553-556
    assert 0.02 < float(mask.mean()) < 0.98
    stem = {"stem": maps.permute(0, 2, 3, 1).contiguous(), "est_c2w": refer["est_c2w"]}
    zero = mapper.render_frame(*args, n_pts_batch=200, jitter=jit)
    for what, feats, kw in (("refer_frames", F, {"refer_frames": refer, "code_method": "fused"}),
                            ("refer_frames, truncate", F * mask[..., None], {"refer_frames": refer, "truncate": True, "code_method": "fused"}),
                            ("refer_frames['stem']", F, {"refer_frames": stem, "code_method": "fused"}),
                            ("refer_frames, launches", F, {"refer_frames": refer, "code_method": "launches"}),
                            ("refer_frames, default method", F, {"refer_frames": refer})):
        col, dep, lab = mapper.render_frame(*args, n_pts_batch=200, jitter=jit, **kw)
        colF, depF, labF = mapper.render_frame(*args, n_pts_batch=200, jitter=jit, features=feats)
        assert_close(col.cpu(), colF.cpu(), what=f"render_frame({what}) colour")
        assert_close(dep.cpu(), depF.cpu(), what=f"render_frame({what}) depth")
        assert float((lab == labF).float().mean()) > 0.995             # argmax may flip where two logits tie to 1e-4
        if not kw.get("truncate"):                                     # (an untrained map's weights die out in front of the surface,
            assert float((col - zero[0]).abs().max()) > 1e-3           #  where the truncated code is zero) ... not the zero-code render


def test_vis_refer_frames_indices_and_no_random_draws():
    mapper, frames, cam = scene(24, 32, 24.0)
    cur_color, cur_c2w = frames["gt_color"][3], frames["est_c2w"][3]
    for n_kf in (0, 1, 3):
        mapper.keyframe_dict = [{"gt_color": frames["gt_color"][k], "est_c2w": frames["est_c2w"][k]} for k in range(n_kf)]
        mapper.keyframe_list = [10 * k for k in range(n_kf)]
        np_state, cpu_state, gpu_state = np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state()
        refer = mapper.vis_refer_frames(cur_color, cur_c2w)
        assert all(np.array_equal(a, b) for a, b in zip(np_state, np.random.get_state()))
        assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(gpu_state, torch.cuda.get_rng_state())
        last = n_kf - 1
        pair = [max(last - 1, 0), max(last, 0)] if n_kf else []        # set_target_refer_frames' choice for the current frame
        assert refer["kf_idx"] == pair + [-1]
        assert refer["gt_color"].shape == (len(pair) + 1, 24, 32, 3) and refer["est_c2w"].shape == (len(pair) + 1, 4, 4)
        for j, k in enumerate(pair):
            assert torch.equal(refer["est_c2w"][j].cpu(), frames["est_c2w"][k].float())
            assert torch.equal(refer["gt_color"][j].cpu(), frames["gt_color"][k].float())
        assert torch.equal(refer["est_c2w"][-1].cpu(), cur_c2w.float()) and torch.equal(refer["gt_color"][-1].cpu(), cur_color.float())
    # the bundle renders
    col, dep, lab = mapper.render_frame(cur_color, frames["gt_depth"][3], frames["gt_label"][3], cur_c2w, refer_frames=refer)
    assert col.shape == (24, 32, 3) and torch.isfinite(col).all()


def test_render_metrics_stem_self_equals_the_hand_written_loop():
    from dns_slam_amd import evaluation as E
    from dns_slam_amd import ops
    mapper, frames, cam = scene(168, 176, 170.0)                       # MS-SSIM's five scales need 161 pixels a side
    idx = [0, 2]
    torch.manual_seed(1)
    jitters = [mapper.draw_jitter(1) for _ in idx]
    out = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters, stem="self")
    n_class = int(mapper.decoder.n_class)
    for k, i in enumerate(idx):
        refer = {"gt_color": frames["gt_color"][i][None], "est_c2w": frames["est_c2w"][i][None]}
        col, _, lab = mapper.render_frame(frames["gt_color"][i], frames["gt_depth"][i], frames["gt_label"][i], frames["est_c2w"][i],
                                          n_pts_batch=8192, jitter=jitters[k], refer_frames=refer)
        v, m, _, _ = ops.ms_ssim_launch(col, frames["gt_color"][i].to(DEV), frames["gt_depth"][i].to(DEV))
        cf, bad = ops.label_confusion(frames["gt_label"][i].to(DEV).reshape(lab.shape), lab, n_class)
        assert out["ssim"]["per_frame"][k] == float(v) and out["psnr"]["per_frame"][k] == -10.0 * np.log10(float(m))
        sem = E.semantic_metrics(cf.double().cpu().numpy().reshape(n_class, n_class), float(bad))
        for key in ("miou", "fwiou", "class_avg_accuracy", "total_accuracy"):
            assert out[key]["per_frame"][k] == sem[key], (key, i)
    by_call = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters,
                               stem=lambda i: {"gt_color": frames["gt_color"][i][None], "est_c2w": frames["est_c2w"][i][None]})
    assert np.array_equal(by_call["psnr"]["per_frame"], out["psnr"]["per_frame"])
    none = E.render_metrics(mapper, frames, indices=idx, n_pts_batch=8192, jitters=jitters)
    assert (np.abs(none["psnr"]["per_frame"] - out["psnr"]["per_frame"]) > 1e-6).all()          # the zero-code figures are others
    with pytest.raises(ValueError, match="exclusive"):
        E.render_metrics(mapper, frames, indices=idx, stem="self", features=[None, None])
    with pytest.raises(ValueError):
        E.render_metrics(mapper, frames, indices=idx, stem="other")
