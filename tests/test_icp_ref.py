"""CPU: the host reference of the ICP alignment (tests/icp_ref.py) against known answers, and the premises under which the GPU
tests (tests/test_gpu_icp.py) hold the kernels to it."""
import numpy as np
import pytest

import icp_ref as I


def test_transform32_is_one_rounding_of_the_float64_value():
    rng = np.random.default_rng(0)
    p = rng.normal(size=(500, 3)).astype(np.float32)
    T = I.rigid((0.2, 1.0, -0.4), 25.0, (0.3, -1.2, 0.7))
    out = I.transform32(T, p)
    exact = p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert out.dtype == np.float32
    assert (np.abs(out.astype(np.float64) - exact) <= 0.5 * np.spacing(np.abs(out)).astype(np.float64) * (1 + 1e-6)).all()
    assert np.array_equal(I.transform32(np.eye(4), p), p)


def test_kabsch_recovers_a_motion_and_never_reflects():
    rng = np.random.default_rng(1)
    p = rng.normal(size=(40, 3))
    G = I.rigid((1.0, -2.0, 0.5), 70.0, (0.4, 0.1, -2.0))
    q = p @ G[:3, :3].T + G[:3, 3]
    assert np.abs(I.kabsch(p, q) - G).max() < 1e-13
    # a mirrored cloud: the best PROPER rotation, not the reflection
    T = I.kabsch(p, q * np.array([1.0, 1.0, -1.0]))
    R = T[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
    # coplanar points (a rank-2 covariance) still give a rotation
    p[:, 2] = 0.0
    q = p @ G[:3, :3].T + G[:3, 3]
    assert np.abs(I.kabsch(p, q) - G).max() < 1e-12


def test_reference_recovers_the_motion_of_the_fixture():
    r = I.reference("d10")
    print("d10:", r["iterations"], "updates, fitness", r["fitness"], "rmse", r["rmse"], "|T - G|", np.abs(r["T"] - I.MOTION).max())
    assert r["converged"] and r["stop"] == "converged" and 2 <= r["iterations"] < 30
    assert r["fitness"] == 1.0 and r["n"] == 1007
    assert 0.003 < r["rmse"] < 0.004                           # 2 mm of noise per axis: sqrt(3) * 2 mm
    assert np.abs(r["T"] - I.MOTION).max() < 1e-3              # the noise of 1007 points, not the 3 degrees / 3 cm of the start
    assert np.abs(np.eye(4) - I.MOTION).max() > 2e-2
    assert r["passes"][0]["rmse"] > 3 * r["rmse"]
    R = r["T"][:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12


def test_reference_radius_and_outliers():
    near = I.reference("d05")
    fit = [p["fitness"] for p in near["passes"]]
    print("d05: fitness per pass", fit)
    assert fit[0] < 0.9 and fit[-1] == 1.0 and all(b >= a for a, b in zip(fit, fit[1:]))
    assert near["converged"] and np.abs(near["T"] - I.MOTION).max() < 1e-3
    out, plain = I.reference("outliers"), I.reference("d10")
    assert out["fitness"] == 1007 / 1307 and out["n"] == 1007
    assert all(p["n"] == 1007 for p in out["passes"])          # the 300 far points never find a correspondence
    assert out["iterations"] == plain["iterations"] and np.abs(out["T"] - plain["T"]).max() < 1e-12


def test_reference_degenerate_stops():
    src, tgt = I.fixture("d10")
    far = src + np.float32(50.0)
    r = I.icp(far, tgt, 0.1)
    assert r["stop"] == "few_correspondences" and r["iterations"] == 0 and r["n"] == 0 and np.array_equal(r["T"], np.eye(4))
    r = I.icp(src, tgt, 0.1, max_iter=0)
    assert r["stop"] == "max_iter" and r["iterations"] == 0 and len(r["passes"]) == 1
    r = I.icp(src, tgt, 0.1, max_iter=3, relative_fitness=0.0, relative_rmse=0.0)
    assert r["iterations"] == 3 and not r["converged"] and len(r["passes"]) == 4


@pytest.mark.parametrize("name", ["d10", "d05", "outliers"])
def test_fixture_premises(name):
    """What the GPU tests assume of every pass they compare: no distance within DIST_RTOL d of the threshold, no inlier whose
    two nearest target points are that close to each other, no stopping delta within 10 % of the criteria.  The allowed count is
    zero; a fixture that misses it gets another seed."""
    for res in (I.reference(name), I.reference(name, 12, True)):
        print(name, "band", min(p["band_min"] for p in res["passes"]), "gap", min(p["gap_min"] for p in res["passes"]),
              "deltas", [(p.get("d_fitness"), p.get("d_rmse")) for p in res["passes"][-2:]])
        assert I.premises(res) == (0, 0, 0)


def test_sparse_case_premises():
    src, tgt = I.sparse_case()
    res = I.icp(src, tgt, I.SPARSE_MAX_DIST, None, 3, 0.0, 0.0)
    print("sparse: n per pass", [p["n"] for p in res["passes"]])
    assert I.premises(res)[:2] == (0, 0)
    assert all(3 < p["n"] < len(src) for p in res["passes"])
