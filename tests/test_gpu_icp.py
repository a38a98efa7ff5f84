"""GPU: ops.icp_point_to_point (csrc/mesh_eval.hip, dns_icp_point_to_point) and evaluation.align_transformation /
apply_transform / calc_3d_metric against the host reference tests/icp_ref.py.

The bound on T (T_ATOL = 1e-8 absolute per entry against the host at the same number of updates): on the host, perturbing every
transformed point by a relative 2^-23 in every pass moved T by 3e-9 to 7e-9 at every count, so an implementation that is one
fp32 rounding off passes, while one wrong pair moves T by about d / n = 3e-5.  Every comparison first asserts, on the host, the
premises under which the fp32 kernels must take the host's decisions (icp_ref.premises): the allowed count is zero."""
import functools

import numpy as np
import pytest
import torch

import icp_ref as I
import mesh_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_ATOL = 1e-8
NAMES = ("d10", "d05", "outliers")


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _clouds(name):
    src, tgt = I.fixture(name)
    return _dev(src), _dev(tgt)


def _run(name, **kw):
    from dns_slam_amd import ops
    s, t = _clouds(name)
    return ops.icp_point_to_point(s, t, max_dist=I.MAX_DIST[name], **kw)


def _assert_rigid(T, what=""):
    T = np.asarray(T, np.float64)
    Rm = T[:3, :3]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-12, what
    assert abs(np.linalg.det(Rm) - 1.0) <= 1e-12, what
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]), what


def _assert_sums(sums, ref_pass, what):
    err = np.abs(np.asarray(sums, np.float64) - ref_pass["sums"])
    rel = (err / np.maximum(ref_pass["mags"], 1e-300)).max()
    print(f"{what}: worst |sum - host| / sum |term| = {rel:.3e}")
    assert (err <= 1e-12 * ref_pass["mags"]).all(), f"{what}: {rel:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_pass_zero_sums(name):
    """max_iter = 0: the correspondences and the 17 sums of the evaluation of init, against the host and against
    ops.nearest_points on the same (identity-transformed) cloud with the threshold applied on the host."""
    from dns_slam_amd import ops
    ref = I.reference(name, 12, True)
    assert I.premises(ref) == (0, 0, 0)
    p0 = ref["passes"][0]
    out = _run(name, max_iter=0)
    assert out["iterations"] == 0 and not out["converged"] and out["stop"] == "max_iter"
    assert out["correspondences"] == p0["n"] and out["sums"][0] == p0["n"]
    _assert_sums(out["sums"], p0, name + " pass 0")
    assert out["fitness"] == p0["n"] / len(I.fixture(name)[0])
    assert abs(out["inlier_rmse"] - p0["rmse"]) <= 1e-12
    assert torch.equal(out["transformation"].cpu(), torch.eye(4, dtype=torch.float64))
    # the same sums from the nearest-point query
    s, t = _clouds(name)
    dist, idx = ops.nearest_points(t, s)
    src, tgt = I.fixture(name)
    ok = dist.cpu().numpy() <= np.float32(I.MAX_DIST[name])
    p, q = src[ok].astype(np.float64), tgt[idx.cpu().numpy()[ok]].astype(np.float64)
    e = p - q
    via = np.concatenate(([float(ok.sum())], p.sum(0), q.sum(0), (q[:, :, None] * p[:, None, :]).sum(0).ravel(), [(e * e).sum()]))
    assert (np.abs(out["sums"] - via) <= 1e-12 * p0["mags"]).all()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("count", [1, 5, 12])
def test_fixed_iteration_counts(name, count):
    ref = I.reference(name, 12, True)
    assert I.premises(ref) == (0, 0, 0)
    out = _run(name, max_iter=count, relative_fitness=0.0, relative_rmse=0.0)
    host = ref["passes"][count]
    T = out["transformation"].cpu().numpy()
    err = np.abs(T - host["T"]).max()
    print(f"{name}, {count} updates: |T - host| = {err:.3e}, n = {out['correspondences']} (host {host['n']})")
    assert out["iterations"] == count and not out["converged"] and out["stop"] == "max_iter"
    assert out["correspondences"] == host["n"]
    assert err <= T_ATOL
    _assert_rigid(T, name)


@pytest.mark.parametrize("name", NAMES)
def test_default_criteria(name):
    ref = I.reference(name)
    assert I.premises(ref) == (0, 0, 0)
    out = _run(name)
    print(f"{name}: {out['iterations']} updates (host {ref['iterations']}), fitness {out['fitness']}, rmse {out['inlier_rmse']}")
    assert out["iterations"] == ref["iterations"] and out["converged"] == ref["converged"] and out["stop"] == ref["stop"]
    assert abs(out["fitness"] - ref["fitness"]) <= 1e-9 and abs(out["inlier_rmse"] - ref["rmse"]) <= 1e-9
    assert np.abs(out["transformation"].cpu().numpy() - ref["T"]).max() <= T_ATOL
    if name == "outliers":
        assert out["fitness"] == 1007 / 1307
    assert np.abs(out["transformation"].cpu().numpy() - I.MOTION).max() < 1e-3


@pytest.mark.parametrize("name", ["d05", "outliers"])
def test_deterministic_and_paths_agree(name):
    """Two calls give the same bits; so does max_rings = 0, which leaves every query the first cell does not decide to the
    all-pairs pass."""
    from dns_slam_amd import ops
    s, t = _clouds(name)
    a, sa = ops.icp_point_to_point_launch(s, t, I.MAX_DIST[name])
    b, sb = ops.icp_point_to_point_launch(s, t, I.MAX_DIST[name])
    c, sc = ops.icp_point_to_point_launch(s, t, I.MAX_DIST[name], max_rings=0)
    assert a.shape == (38,) and a.dtype == torch.float64 and sa.shape == (4,)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(sa, sb)
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    sa, sc = sa.cpu().tolist(), sc.cpu().tolist()
    print(f"{name}: all-pairs queries {sa[1]} (default rings), {sc[1]} (max_rings = 0), status {sa}")
    assert sc[1] > sa[1] and sc[1] > 0 and sa[0] == 0 and sc[3] == sa[3] == 1


@pytest.mark.parametrize("count", [0, 3])
def test_sparse_target_dense_source(count):
    """M = 65 against N = 5000: twenty partial rows, a grid of a few cells per axis, max_dist of several cell widths, a quarter of
    the source outside the radius."""
    from dns_slam_amd import ops
    src, tgt = I.sparse_case()
    ref = I.icp(src, tgt, I.SPARSE_MAX_DIST, None, 3, 0.0, 0.0)
    assert I.premises(ref)[:2] == (0, 0)
    host = ref["passes"][count]
    out = ops.icp_point_to_point(_dev(src), _dev(tgt), I.SPARSE_MAX_DIST, max_iter=count, relative_fitness=0.0, relative_rmse=0.0)
    err = np.abs(out["transformation"].cpu().numpy() - host["T"]).max()
    print(f"sparse, {count} updates: n = {out['correspondences']} (host {host['n']}), |T - host| = {err:.3e}")
    assert out["correspondences"] == host["n"] and out["iterations"] == count
    _assert_sums(out["sums"], host, f"sparse pass {count}")
    assert err <= T_ATOL
    _assert_rigid(out["transformation"].cpu().numpy())


def test_sizes():
    from dns_slam_amd import ops
    rng = np.random.default_rng(11)
    init = I.rigid((0.0, 1.0, 1.0), 10.0, (0.1, 0.0, -0.1))
    for M in (1, 63, 1000):
        for N in (1, 63, 65, 257):
            tgt = rng.normal(size=(M, 3)).astype(np.float32)
            src = rng.normal(size=(N, 3)).astype(np.float32)
            for t0 in (None, init):
                out = ops.icp_point_to_point(_dev(src), _dev(tgt), 1.5, init=t0, max_iter=4)
                T = out["transformation"].cpu().numpy()
                _assert_rigid(T, f"M {M} N {N}")
                p0 = I.evaluate(np.eye(4) if t0 is None else t0, src, tgt.astype(np.float64),
                                I.cKDTree(tgt.astype(np.float64)), 1.5)
                if N == 1 or (p0["n"] < 3 and p0["band_bad"] == 0):
                    assert out["stop"] == "few_correspondences" and out["iterations"] == 0 and not out["converged"]
                    assert np.array_equal(T, np.eye(4) if t0 is None else t0)
                    if p0["band_bad"] == 0:
                        assert out["correspondences"] == p0["n"]
                else:
                    assert out["stop"] in ("max_iter", "converged", "few_correspondences")
                    assert 0 <= out["correspondences"] <= N and 0.0 <= out["fitness"] <= 1.0


def test_init():
    """From the host's converged transformation: one update at the most... and the host's result from the same start."""
    ref = I.reference("d10")
    src, tgt = I.fixture("d10")
    again = I.icp(src, tgt, 0.1, ref["T"])
    assert I.premises(again) == (0, 0, 0)
    for init in (ref["T"], torch.from_numpy(ref["T"])):
        out = _run("d10", init=init)
        print(f"from the converged T: {out['iterations']} updates (host {again['iterations']})")
        assert out["iterations"] <= 1 and out["iterations"] == again["iterations"] and out["converged"]
        assert np.abs(out["transformation"].cpu().numpy() - again["T"]).max() <= T_ATOL
    # pass 0 evaluates init itself
    out = _run("d10", init=ref["T"], max_iter=0)
    assert np.array_equal(out["transformation"].cpu().numpy(), ref["T"])
    assert out["correspondences"] == again["passes"][0]["n"]
    _assert_sums(out["sums"], again["passes"][0], "init, pass 0")


def test_arguments():
    from dns_slam_amd import ops
    s, t = _clouds("d10")
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s.cpu(), t.cpu())
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s[:, :2], t)
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s.reshape(-1), t)
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s[:0], t)
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s, t[:0])
    for md in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.icp_point_to_point(s, t, max_dist=md)
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s, t, init=np.eye(3))
    with pytest.raises(ValueError):
        ops.icp_point_to_point(s, t, init=np.full((4, 4), np.nan))
    for where in ("source", "target"):
        for bad in (float("nan"), float("inf")):
            a, b = s.clone(), t.clone()
            (a if where == "source" else b)[33, 1] = bad
            with pytest.raises(ValueError, match=where):
                ops.icp_point_to_point(a, b)
            res, status = ops.icp_point_to_point_launch(a, b)                 # T = init, nothing evaluated
            assert status.cpu().tolist()[3] == 3
            assert torch.equal(res[:16].cpu().view(4, 4), torch.eye(4, dtype=torch.float64)) and not res[16:].any()


def test_calc_3d_metric_aligns():
    """five_spheres against a rigidly moved copy with 2 mm of noise on its vertices: the figures after the device's alignment
    equal metrics_3d of the mesh aligned on the host (to the distance bound plus what a 1e-8 difference of T moves a point: under
    1e-5 cm), they are smaller than the unaligned ones, and align=False is metrics_3d."""
    from dns_slam_amd import evaluation as E
    vg, fg = R.five_spheres()
    rng = np.random.default_rng(21)
    moved = vg.astype(np.float64) + rng.normal(0.0, 0.002, vg.shape)
    vr = ((moved - I.MOTION[:3, 3]) @ I.MOTION[:3, :3]).astype(np.float32)
    n = 6000
    u_rec, u_gt = _dev(rng.random((n, 3))), _dev(rng.random((n, 3)))
    dv = [_dev(a) for a in (vr, fg, vg, fg)]
    kw = dict(n_samples=n, u_rec=u_rec, u_gt=u_gt)
    host = I.icp(vr, vg, 0.1)
    assert I.premises(host) == (0, 0, 0)
    T = E.align_transformation(dv[0], dv[2])
    assert T.dtype == torch.float64 and T.shape == (4, 4) and T.is_cuda
    assert np.abs(T.cpu().numpy() - host["T"]).max() <= T_ATOL
    # apply_transform: float64, one rounding
    moved_dev = E.apply_transform(dv[0], T)
    assert moved_dev.dtype == torch.float32
    exact = vr.astype(np.float64) @ host["T"][:3, :3].T + host["T"][:3, 3]
    assert np.abs(moved_dev.cpu().numpy().astype(np.float64) - exact).max() <= 2.0 ** -23 * np.abs(exact).max()
    m = E.calc_3d_metric(*dv, **kw)
    assert torch.equal(m["transformation"], T) and m["icp"]["iterations"] == host["iterations"] and m["icp"]["converged"]
    want = E.metrics_3d(_dev(exact.astype(np.float32)), dv[1], dv[2], dv[3], **kw)
    plain = E.metrics_3d(*dv, **kw)
    print("aligned", {k: m[k] for k in want}, "host-aligned", want, "unaligned", plain)
    for k in ("accuracy_cm", "completion_cm"):
        assert abs(m[k] - want[k]) <= R.DIST_RTOL * want[k] + 1e-5
        assert m[k] < plain[k]
    assert abs(m["completion_ratio_pct"] - want["completion_ratio_pct"]) <= 100.0 / n
    off = E.calc_3d_metric(*dv, align=False, **kw)
    assert all(off[k] == plain[k] for k in plain)
    assert torch.equal(off["transformation"].cpu(), torch.eye(4, dtype=torch.float64))
