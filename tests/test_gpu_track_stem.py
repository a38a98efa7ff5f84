"""The fused tracker iteration on a stem-trained map (csrc/track_fused.inc, DNS_TF_STEM): feature_matching + the
frozen Merge network inside the kernel, and the reference view that follows the pose being optimised (slams/tracking.py:316-319),
against the launch sequence ``TrackStep.step``, the autograd loop and the CPU oracle.  60 x 80 images, stem maps 30 x 40 x 64,
249 rays (a partial last workgroup at two and at four rays per workgroup); the reference views look past part of the tracked
frame's points, so both the valid and the invalid branch of a (point, view) pair run (``_case`` says how and why)."""
import math

import pytest
import torch

from oracle import feature_ref as fr
from oracle import render_math as rm
from oracle import slam_ref as sr
from test_gpu_slam import _setup
from util import oracle_from_product, randomise_

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_RAYS = 249
# (n_neurons, n_hidden_layers, n_uniform, n_surface, views, follow): S = 47, 32, 64
CASES = [(64, 2, 32, 15, 2, (False, True)), (32, 1, 22, 10, 3, (False, False, False)), (64, 2, 48, 16, 1, (True,))]
VIEW_TURNS = ((0.45, (0.05, 0.0, 0.02)), (-0.5, (-0.04, 0.03, 0.0)), (0.3, (0.0, -0.05, 0.05)))   # (yaw in rad, shift) of the views
DEPTH_SCALE = 0.05
MAP_SCALE = 50.0                             # stem maps of the order of 30: the code then outweighs the (random) latent beside it
_cache = {}


def _case(nn, nl, nu, ns, R, follow, cur_frame=2):
    key = (nn, nl, nu, ns, R, follow, cur_frame)
    if key in _cache:
        return _cache[key]
    from dns_slam_amd.encoder import ResNet
    cfg, bound, cam, frames, dec, mapper = _setup(nn, nl, n_pixels=400)
    randomise_(dec.merge, 21)
    cfg["tracking"]["n_pixels"] = N_RAYS
    cfg["training"]["n_samples_ray"], cfg["training"]["n_surface_ray"] = nu, ns
    cur = {k: frames[k][cur_frame] for k in ("gt_color", "gt_depth", "gt_label")}
    # The scene's networks are random: a ray's compositing weight sits on its first few samples, and the samples inside the
    # truncation band -- the only ones whose 2-D code counts -- carry ~1e-7 of it where the band lies mid-ray (measured: zeroing the
    # stem maps moved the loss terms in the 8th digit, in the launch sequence and the fused kernel alike).  Below the top quarter of
    # the image the depth is scaled down: the uniform samples still span [0, 1.2 max depth of the draw], so these rays' bands come
    # right behind their first samples and the code (of maps scaled by MAP_SCALE) decides the rendered colour and logits
    depth = cur["gt_depth"].clone()
    depth[depth.shape[0] // 4:] *= DEPTH_SCALE
    cur["gt_depth"] = depth
    c2w = frames["est_c2w"][cur_frame].clone()
    c2w[:3, 3] += torch.tensor([0.02, -0.01, 0.015], dtype=c2w.dtype)
    # The scene's four frames look 90 degrees apart with a 67 degree field of view: none sees another's points.  The views' IMAGES are
    # other frames'; their POSES are the tracked frame's, turned about the camera's vertical axis and shifted, so that each
    # sees part of the tracked frame's points
    vf = [f for f in range(4) if f != cur_frame][:R]
    stem = ResNet(seed=3).to(DEV)
    with torch.no_grad():
        feats = stem(torch.stack([frames["gt_color"][k] for k in vf])[None].to(DEV)).detach() * MAP_SCALE
    poses = []
    for k in range(R):
        ang, shift = VIEW_TURNS[k]
        turn = torch.eye(4, dtype=torch.float64)
        turn[0, 0], turn[0, 2], turn[2, 0], turn[2, 2] = math.cos(ang), math.sin(ang), -math.sin(ang), math.cos(ang)
        turn[:3, 3] = torch.tensor(shift, dtype=torch.float64)
        poses.append(frames["est_c2w"][cur_frame].double() @ turn)
    refer = {"est_w2c": torch.stack([torch.inverse(p).float() for p in poses]).to(DEV), "follow": follow}
    out = dict(cfg=cfg, bound=bound, cam=cam, frames=frames, dec=dec, cur=cur, c2w=c2w, feats=feats, refer=refer, nu=nu, ns=ns, R=R)
    _cache[key] = out
    return out


def _tracker(c):
    from dns_slam_amd.tracking import Tracker
    t = Tracker(c["cfg"], c["dec"], c["bound"], c["cam"], device=DEV)
    t.border = 5
    t.static_shapes = True
    return t


def _draws(c, n_it, seed=9):
    t = _tracker(c)
    g = torch.Generator().manual_seed(seed)
    H, W, b = t.H, t.W, t.border
    return (torch.randint((H - 2 * b) * (W - 2 * b), (n_it, N_RAYS), generator=g), torch.rand(n_it, c["ns"], generator=g),
            torch.rand(n_it, c["ns"], generator=g))


def _step_run(c, draws, t_surf_forced, n_it, features=None, refer=None):
    """n_it ``TrackStep.step`` calls on the given draws (the forced mid sample as dns_track_fused_begin left it)."""
    from dns_slam_amd.fused_step import TrackStep
    tracker = _tracker(c)
    with tracker.frozen_scene():
        ts = TrackStep(tracker, c["cur"], c["c2w"], features=c["feats"] if features is None else features,
                       refer_frames=c["refer"] if refer is None else refer)
        for k in range(n_it):
            ts.step(draws=(draws[0][k].to(DEV), t_surf_forced[k].contiguous(), draws[2][k].to(DEV)))
        torch.cuda.synchronize()
    return ts


def _fused_run(c, draws, n_it, graph=False, zero_maps=False, features=None, refer=None):
    from dns_slam_amd.fused_step import TrackStep
    tracker = _tracker(c)
    with tracker.frozen_scene():
        ts = TrackStep(tracker, c["cur"], c["c2w"], features=c["feats"] if features is None else features,
                       refer_frames=c["refer"] if refer is None else refer)
        assert not ts.fused_supported() or not ts.stem
        if ts.stem:
            assert ts.fused_supported(stem=True)
            if zero_maps:
                ts.feat_maps.zero_()
        ts.run_fused(n_it, graph=graph, draws=draws)
        torch.cuda.synchronize()
    return ts


def _terms(ts_fused, ts_step):
    """(name, fused, launch sequence) of the last iteration's loss terms: fused out = (p, d, l, total, n_valid), the launch
    sequence's out = (p, d, l, lt, fs, op, total, ...)."""
    fo, so = ts_fused.fused_out.cpu(), ts_step.out.cpu()
    return [(n, float(fo[i]), float(so[j])) for n, i, j in (("p", 0, 0), ("d", 1, 1), ("l", 2, 2), ("total", 3, 6))]


def _grad_dev(g, ref):
    return float((g.cpu() - ref.cpu()).abs().max()) / float(ref.cpu().abs().max())


@pytest.mark.parametrize("nn,nl,nu,ns,R,follow", CASES)
def test_one_fused_stem_iteration_equals_the_launch_sequence(nn, nl, nu, ns, R, follow):
    """One iteration, same draws, same starting pose: the fused kernel's loss terms against ``TrackStep.step``'s at
    2e-5 |ref| + 1e-7, its pose gradient at 2e-5 max|g| (the non-stem kernel with a per-sample code meets that bound for its own
    gradient on these shapes: measured 1.9e-6, 1.5e-5 and 1.5e-6 of max|g| (quaternion), so the bound is not widened; the stem
    form, whose samples and grid cells round as the launch sequence's, measured 1.7e-7, 9.2e-8 and 2.3e-7); between
    5 % and 95 % of the pairs of the views with a stored pose are inside their view (a lone following view sees every point); with zeroed stem maps the total loss moves by more than ten times the tolerance -- which is what a
    kernel that ignores the maps cannot show."""
    c = _case(nn, nl, nu, ns, R, follow)
    draws = _draws(c, 1)
    tf_ = _fused_run(c, draws, 1)
    forced = tf_._fb["keep"]["t_surf"].clone()
    ts = _step_run(c, draws, forced, 1)
    per_view = (ts.stem2d.code_cols.abs().sum(-1) > 0).float().reshape(R, -1).mean(1).cpu()
    print(f"valid pairs per view {[round(float(v), 3) for v in per_view]}")
    stored = [float(per_view[r]) for r in range(R) if not follow[r]]
    if stored:
        assert 0.05 < sum(stored) / len(stored) < 0.95, per_view
    else:
        # a lone FOLLOWING view looks from the pose the rays are cast from: every sample in front of the camera is inside it, so the
        # invalid branch is the other cases' to cover
        assert float(per_view.mean()) > 0.95, per_view
    terms = _terms(tf_, ts)
    for name, a, b in terms:
        print(f"{name}: fused {a:.9g} step {b:.9g} rel {abs(a - b) / max(abs(b), 1e-30):.3g}")
    dq, dt = _grad_dev(tf_.g_quat, ts.g_quat), _grad_dev(tf_.g_trans, ts.g_trans)
    print(f"d quat {dq:.3g} d trans {dt:.3g} of max|g|")
    for name, a, b in terms:
        assert abs(a - b) <= 2e-5 * abs(b) + 1e-7, (name, a, b)
    assert float(ts.g_quat.abs().max()) > 0 and float(ts.g_trans.abs().max()) > 0
    assert dq <= 2e-5 and dt <= 2e-5, (dq, dt)
    tz = _fused_run(c, draws, 1, zero_maps=True)
    total, total0 = terms[3][1], float(tz.fused_out[3])
    print(f"total {total:.9g}, with zeroed maps {total0:.9g}")
    assert abs(total - total0) > 10 * (2e-5 * abs(terms[3][2]) + 1e-7), (total, total0)


@pytest.mark.parametrize("nn,nl,nu,ns,R,follow", CASES[:2])
def test_fused_stem_free_run_equals_the_launch_sequence(nn, nl, nu, ns, R, follow):
    """15 free-running iterations on given draws, eager and replayed from ONE captured iteration, against 15 ``step`` calls: best
    loss to 1e-4, best camera and pose to 2e-4 (the project's criteria for two stem implementations running free: a rounded
    pixel may flip once the poses differ in the last bits).  Two eager runs are bit-identical (no atomics, fixed orders)."""
    c = _case(nn, nl, nu, ns, R, follow)
    n_it = 15
    draws = _draws(c, n_it)
    runs = {m: _fused_run(c, draws, n_it, graph=(m == "graph")) for m in ("eager", "eager2", "graph")}
    forced = runs["eager"]._fb["keep"]["t_surf"].clone()
    ts = _step_run(c, draws, forced, n_it)
    ref_best, ref_cam = float(ts.best_loss[0]), ts.best_cam.cpu()
    for m, r in runs.items():
        best = float(r.best_loss[0])
        print(m, best, ref_best, float((r.best_cam.cpu() - ref_cam).abs().max()), float((r.Q.cpu() - ts.Q.cpu()).abs().max()),
              float((r.T.cpu() - ts.T.cpu()).abs().max()))
        assert abs(best - ref_best) <= 1e-4 * abs(ref_best), (m, best, ref_best)
        assert float((r.best_cam.cpu() - ref_cam).abs().max()) <= 2e-4, (m, r.best_cam, ref_cam)
        assert float((r.Q.cpu() - ts.Q.cpu()).abs().max()) <= 2e-4 and float((r.T.cpu() - ts.T.cpu()).abs().max()) <= 2e-4, m
    a, b = runs["eager"], runs["eager2"]
    assert torch.equal(a.best_cam, b.best_cam) and torch.equal(a.Q, b.Q) and torch.equal(a.T, b.T) and torch.equal(a.fused_out, b.fused_out)
    assert float((ts.T.cpu().reshape(-1) - c["c2w"][:3, 3].float()).abs().max()) > 0               # the pose did move


def _oracle_first_iteration(c, draws, forced, nn, nl):
    """Loss and pose gradient of the first iteration on the CPU oracle: frame_samples on the given draws, feature_matching with
    merge_forward on the sample points (a following view's w2c = inverse(c2w(quad, T)), detached), truncation mask, tracking loss."""
    from dns_slam_amd.common import get_quad_from_c2w
    cfg, bound, cam, dec, cur = c["cfg"], c["bound"], c["cam"], c["dec"], c["cur"]
    tracker = _tracker(c)
    om = oracle_from_product(cfg, bound, dec)
    for p in (om.table, om.coarse, om.color, om.logit):
        p.requires_grad_(False)
    q = get_quad_from_c2w(c["c2w"]).clone().detach().float().requires_grad_(True)
    T = c["c2w"][:3, 3].clone().detach().float().requires_grad_(True)
    img5 = torch.cat((cur["gt_color"], cur["gt_depth"][..., None], cur["gt_label"][..., None]), -1)
    camt = (cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    b = tracker.border
    so = sr.frame_samples(img5, q, T, camt, bound, draws[0][0], forced[0].cpu(), draws[2][0], c["nu"], c["ns"],
                          window=(b, cam["H"] - b, b, cam["W"] - b))
    K = torch.tensor([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])
    w2c = c["refer"]["est_w2c"].cpu().clone()
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    cur_w2c = torch.inverse(torch.cat([torch.cat((rm.rotation_from_quad(q.detach()), T.detach()[:, None]), -1), bottom], 0))
    for r, fl in enumerate(c["refer"]["follow"]):
        if fl:
            w2c[r] = cur_w2c
    params = dec.merge.decoder.params.detach().cpu()
    n_bins = dec.merge.pe_fn.n_bins
    merge = lambda p_, o_, c_: fr.merge_forward(params, bound, p_, o_, c_, n_bins=n_bins, n_neurons=nn, n_hidden_layers=nl)
    S = c["nu"] + c["ns"]
    code = fr.feature_matching(cam["H"], cam["W"], K, so["pts"].flatten(0, 1), w2c, c["feats"][0].cpu(), merge).reshape(N_RAYS, S, -1)
    so = dict(so)
    so["features"] = code * rm.truncation_mask(so["z_vals"], so["gt_depth"])[..., None]
    mask = (so["gt_depth"] > 0.01) & so["inside"]
    loss = sr.tracking_loss(om, so, mask, tracker.lambda_p, tracker.lambda_d, tracker.lambda_l)[0]
    loss.backward()
    return float(loss.detach()), q.grad.clone(), T.grad.clone()


@pytest.mark.parametrize("nn,nl,nu,ns,R,follow", CASES[:2])
def test_first_fused_stem_iteration_matches_the_oracle(nn, nl, nu, ns, R, follow):
    """The first iteration against the CPU oracle: total loss to 5e-4 (the project's stem-against-oracle criterion); the pose
    gradient's deviation from the oracle (max |g - g_oracle| / max |g_oracle|, quaternion and translation) at most twice that
    of ``TrackStep.step`` on the same inputs.

    Measured on an MI355X (quat, trans): 64 x 2, S = 47, R = 2: step 8.0e-7, 7.8e-7; fused 8.0e-7, 6.7e-7.  32 x 1, S = 32, R = 3:
    step 9.2e-8, 6.2e-7; fused 1.8e-7, 6.9e-8 (one and two ulp of the largest component).  Before the stem form's ray directions,
    sample depths and grid cells were made to round as sample.hip's and encode.hip's do (csrc/dev_rn.hpp) the fused figures were
    9.7e-7, 2.3e-6 and 7.4e-6, 7.5e-6: a third of the uniform samples lay one ulp from the oracle's."""
    c = _case(nn, nl, nu, ns, R, follow)
    draws = _draws(c, 1)
    tf_ = _fused_run(c, draws, 1)
    forced = tf_._fb["keep"]["t_surf"].clone()
    ts = _step_run(c, draws, forced, 1)
    lo, gq, gT = _oracle_first_iteration(c, draws, forced, nn, nl)
    lf, ls = float(tf_.fused_out[3]), float(ts.out[6])
    dev = {"step": (_grad_dev(ts.g_quat, gq), _grad_dev(ts.g_trans, gT)), "fused": (_grad_dev(tf_.g_quat, gq), _grad_dev(tf_.g_trans, gT))}
    print(f"loss: oracle {lo:.9g} fused {lf:.9g} step {ls:.9g}; gradient deviation from the oracle (quat, trans): {dev}")
    assert abs(lf - lo) <= 5e-4 * abs(lo), (lf, lo)
    assert dev["fused"][0] <= 2 * dev["step"][0] and dev["fused"][1] <= 2 * dev["step"][1], dev


def test_following_view_in_the_autograd_loop_and_the_launch_sequence():
    """refer_frames['follow'] = (False, True): ``Tracker.track_frame``'s autograd loop and six ``TrackStep.step`` calls against a
    loop written out here that rebuilds est_w2c[1] = inverse(c2w(quad, T)) before every ``get_target_samples`` call
    (slams/tracking.py:316-319), same seed: best loss to 1e-4, best camera to 2e-4.  Without 'follow', or with all flags False,
    the result is bit-identical to the call without the key."""
    from dns_slam_amd import ops
    from dns_slam_amd.common import get_rotation_from_quad
    c = _case(32, 1, 32, 15, 2, (False, True))
    n_it = 6
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=DEV)

    def seed():
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)

    # the loop written out (Tracker._track_frame_eager's body with the reference's two lines in front of the samples)
    tracker = _tracker(c)
    seed()
    with tracker.frozen_scene():
        optimizer, quad, T = tracker.set_optimizer(c["c2w"], fused=True)
        frames = dict(c["cur"])
        frames["est_quad"], frames["est_T"] = quad, T
        prep = tracker.prepare_frame(c["cur"])
        refer = {"est_w2c": c["refer"]["est_w2c"].clone()}
        best_loss, best_cam = float("inf"), None
        for _ in range(n_it):
            optimizer.zero_grad()
            with torch.no_grad():
                cur_c2w = torch.cat([torch.cat((get_rotation_from_quad(quad.detach()), T.detach()[:, None]), -1), bottom], 0)
                refer["est_w2c"][1] = torch.inverse(cur_c2w)
            s = tracker.get_target_samples(frames, refer_frames=refer, features=c["feats"], prep=prep)
            pc, pd, pv, pl = tracker.renderer(s)
            loss, _ = ops.tracking_losses(pc, pd, pv, pl, s["gt_color"], s["gt_depth"], s["gt_label"], s["mask"],
                                          (tracker.lambda_p, tracker.lambda_d, tracker.lambda_l))
            if float(loss) < best_loss:
                best_loss, best_cam = float(loss), torch.cat((quad, T), 0).detach().cpu().clone()
            loss.backward()
            optimizer.step()
    got = {}
    for name, step in (("autograd", False), ("step", True)):
        tracker = _tracker(c)
        tracker.use_track_step = step
        seed()
        cam7, best = tracker.track_frame(c["cur"], c["c2w"], n_iters=n_it, features=c["feats"], refer_frames=c["refer"], fused=True)
        if step:
            assert tracker.last_track_step.steps == n_it and getattr(tracker.last_track_step, "_fb", None) is None
        got[name] = (cam7.detach().cpu().clone(), float(best))
        print(name, float(best), best_loss, float((got[name][0] - best_cam).abs().max()))
    for name, (cam7, best) in got.items():
        assert abs(best - best_loss) <= 1e-4 * abs(best_loss), (name, best, best_loss)
        assert float((cam7 - best_cam).abs().max()) <= 2e-4, (name, cam7, best_cam)
    # the view that follows matters: frozen at the stored pose the run differs
    res = {}
    for key, refer in (("absent", {"est_w2c": c["refer"]["est_w2c"]}), ("all false", {"est_w2c": c["refer"]["est_w2c"], "follow": (False, False)})):
        for step in (False, True):
            tracker = _tracker(c)
            tracker.use_track_step = step
            seed()
            cam7, best = tracker.track_frame(c["cur"], c["c2w"], n_iters=n_it, features=c["feats"], refer_frames=refer, fused=True)
            res[(key, step)] = (cam7.detach().clone(), best.detach().clone())
    for step in (False, True):
        assert torch.equal(res[("absent", step)][0], res[("all false", step)][0]) and torch.equal(res[("absent", step)][1], res[("all false", step)][1])
    assert not torch.equal(res[("absent", False)][0].cpu(), got["autograd"][0])


def test_reset_keeps_the_fused_stem_block_and_its_graph():
    """A second frame on the same TrackStep -- new images, maps, reference poses and initial pose, fused and replayed from the
    graph captured for the first frame -- is bit-identical to a fresh TrackStep on that frame."""
    from dns_slam_amd.fused_step import TrackStep
    nn, nl, nu, ns, R, follow = CASES[0]
    ca, cb = _case(nn, nl, nu, ns, R, follow), _case(nn, nl, nu, ns, R, follow, cur_frame=1)
    n_it = 4
    da, db = _draws(ca, n_it, seed=3), _draws(cb, n_it, seed=4)
    tracker = _tracker(ca)
    with tracker.frozen_scene():
        ts = TrackStep(tracker, ca["cur"], ca["c2w"], features=ca["feats"], refer_frames=ca["refer"])
        ts.run_fused(n_it, graph=True, draws=da)
        block, graph = ts._fb, ts._fb["graph"]
        ts.reset(cb["cur"], cb["c2w"], features=cb["feats"], refer_frames=cb["refer"])
        ts.run_fused(n_it, graph=True, draws=db)
        torch.cuda.synchronize()
        assert ts._fb is block and ts._fb["graph"] is graph
        fresh = TrackStep(_tracker(cb), cb["cur"], cb["c2w"], features=cb["feats"], refer_frames=cb["refer"])
        fresh.run_fused(n_it, graph=True, draws=db)
        torch.cuda.synchronize()
    for name in ("best_cam", "Q", "T", "fused_out", "best_loss"):
        assert torch.equal(getattr(ts, name), getattr(fresh, name)), name
    assert float((ts.T.cpu().reshape(-1) - cb["c2w"][:3, 3].float()).abs().max()) > 0


def test_routing_of_a_stem_tracker():
    """``fused_supported()`` stays False for a stem tracker and is True with ``stem=True``; ``track_frame`` takes the launch
    sequence unless ``tracker.fused_stem`` is set, and the fused kernel when it is; fp16 networks are refused."""
    from dns_slam_amd import ops
    from dns_slam_amd.fused_step import TrackStep
    c = _case(*CASES[0])
    tracker = _tracker(c)
    tracker.use_track_step = True
    assert tracker.fused_stem is False
    tracker.track_frame(c["cur"], c["c2w"], n_iters=2, features=c["feats"], refer_frames=c["refer"])
    ts = tracker.last_track_step
    assert ts.stem and ts.steps == 2 and getattr(ts, "_fb", None) is None and not hasattr(ts, "fused_out")   # the launch sequence ran
    assert not ts.fused_supported() and ts.fused_supported(stem=True)
    tracker.fused_stem = True
    tracker.track_frame(c["cur"], c["c2w"], n_iters=2, features=c["feats"], refer_frames=c["refer"])
    ts = tracker.last_track_step
    assert ts._fb is not None and hasattr(ts, "fused_out") and ts.steps == 2
    with tracker.frozen_scene():
        th = TrackStep(_tracker(c), c["cur"], c["c2w"], features=c["feats"], refer_frames=c["refer"])
        th.fp16 = ops.MLP_FP16_FLAG
        assert not th.fused_supported(stem=True)
