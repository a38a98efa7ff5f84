"""Host reference of ops.icp_point_to_point (csrc/mesh_eval.hip, dns_icp_point_to_point): open3d's point-to-point
registration_icp as the reference's get_align_transformation calls it (eval_3d.py:45-59), restated with numpy and
scipy.spatial.cKDTree.  open3d itself is not a dependency of this project; this restatement is the definition the kernels are
tested against, with the two deliberate differences from open3d the kernels have:

    - pass k searches from p' = fl32(T_k p), T_k the cumulative float64 transformation applied to the ORIGINAL fp32 source
      (open3d transforms its float64 copy of the cloud update by update);
    - a correspondence exists iff the distance is <= max_dist (open3d's radius search is exclusive).

Per pass it also measures how close the pass came to a decision the fp32 kernels could take differently: the number of
distances within DIST_RTOL d of max_dist, and the number of inliers whose two nearest target points are within that bound of each
other; plus the smallest such band and gap.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial import cKDTree

from mesh_eval_ref import DIST_RTOL

N_SUMS = 17                      # n, sum p' [3], sum q [3], sum q p'^T [9, row = q], sum |p' - q|^2


def transform32(T, p):
    """fl32(T p): ((T[i,0] x + T[i,1] y) + T[i,2] z) + T[i,3] in float64 (one rounding per operation), rounded once to fp32."""
    T = np.asarray(T, np.float64)
    p = np.asarray(p, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], 1).astype(np.float32)


def evaluate(T, src, tgt, tree, max_dist):
    """One pass: the correspondences of fl32(T src) in tgt and their sums."""
    md = float(np.float32(max_dist))
    p = transform32(T, src).astype(np.float64)
    k = min(2, len(tgt))
    d, i = tree.query(p, k=k)
    d, i = d.reshape(len(p), k), i.reshape(len(p), k)
    d1, i1 = d[:, 0], i[:, 0]
    ok = d1 <= md
    q = tgt[i1[ok]]
    pp = p[ok]
    n = int(ok.sum())
    e = pp - q
    sums = np.concatenate(([float(n)], pp.sum(0), q.sum(0), (q[:, :, None] * pp[:, None, :]).sum(0).ravel(), [(e * e).sum()]))
    mags = np.concatenate(([float(n)], np.abs(pp).sum(0), np.abs(q).sum(0),
                           (np.abs(q)[:, :, None] * np.abs(pp)[:, None, :]).sum(0).ravel(), [(e * e).sum()]))
    band = np.abs(d1 - md)
    gap = d[ok, 1] - d[ok, 0] if k == 2 else np.full(n, np.inf)
    return {"T": np.array(T, np.float64), "n": n, "fitness": n / len(p), "rmse": float(np.sqrt((e * e).sum() / n)) if n else 0.0,
            "sums": sums, "mags": mags, "p": pp, "q": q, "idx": i1, "ok": ok, "dist": d1,
            "band_min": float(band.min()), "band_bad": int((band <= DIST_RTOL * d1).sum()),
            "gap_min": float(gap.min()) if n else np.inf, "gap_bad": int((gap <= DIST_RTOL * d1[ok]).sum())}


def kabsch(p, q):
    """The rigid motion [4,4] minimising sum |R p + t - q|^2: SVD of the cross-covariance with the determinant fix (Umeyama
    without scale)."""
    mp, mq = p.mean(0), q.mean(0)
    H = (p - mp).T @ (q - mq)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    out = np.eye(4)
    out[:3, :3] = R
    out[:3, 3] = mq - R @ mp
    return out


def icp(src, tgt, max_dist=0.1, init=None, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> {"T", "fitness", "rmse", "n", "iterations", "converged", "stop", "passes": [evaluate(...) of every pass, with "d_fitness"
    and "d_rmse" against the pass before it]}.  registration_icp's loop: evaluate init; then update, evaluate, and stop when both
    deltas are under their criteria; fewer than 3 correspondences stop it with T as it is."""
    src = np.asarray(src, np.float32)
    tgt = np.asarray(tgt, np.float32).astype(np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    passes = [evaluate(T, src, tgt, tree, max_dist)]
    converged, stop, updates = False, "max_iter", 0
    for k in range(max_iter + 1):
        cur = passes[-1]
        if k > 0:
            prev = passes[-2]
            cur["d_fitness"], cur["d_rmse"] = abs(cur["fitness"] - prev["fitness"]), abs(cur["rmse"] - prev["rmse"])
            if cur["d_fitness"] < relative_fitness and cur["d_rmse"] < relative_rmse:
                converged, stop = True, "converged"
                break
        if k == max_iter:
            break
        if cur["n"] < 3:
            stop = "few_correspondences"
            break
        T = kabsch(cur["p"], cur["q"]) @ T
        updates += 1
        passes.append(evaluate(T, src, tgt, tree, max_dist))
    last = passes[-1]
    return {"T": last["T"], "fitness": last["fitness"], "rmse": last["rmse"], "n": last["n"], "iterations": updates,
            "converged": converged, "stop": stop, "passes": passes}


def premises(res, criteria=1e-6):
    """The three conditions under which the fp32 kernels must take every decision the host took: -> (distances at the threshold,
    inliers with two nearest points at the same distance, stopping deltas within 10 % of the criteria), over all passes."""
    band = sum(p["band_bad"] for p in res["passes"])
    gap = sum(p["gap_bad"] for p in res["passes"])
    near = sum(1 for p in res["passes"] for k in ("d_fitness", "d_rmse") if k in p and abs(p[k] - criteria) <= 0.1 * criteria)
    return band, gap, near


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def rigid(axis, degrees, translation):
    """Rodrigues: the rotation by `degrees` about `axis`, then the translation -> [4,4] float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    out[:3, 3] = translation
    return out


MOTION = rigid((1.0, 2.0, 3.0), 3.0, (0.03, -0.02, 0.025))       # G: what the registration has to recover
FIXTURE_SEED = {"d10": 1, "d05": 1, "outliers": 1}
MAX_DIST = {"d10": 0.1, "d05": 0.05, "outliers": 0.1}
N_OUTLIERS = 300


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (source fp32 [N,3], target fp32 [2014,3]).  Target: the vertices of mesh_cc_ref.five_spheres() (no rotational symmetry).
    Source: a random half of them (1007 points: four workgroups of the reduction) with 2 mm Gaussian noise, moved by the inverse
    of MOTION; "outliers" appends 300 points near (3, 3, 3), far from every target point under every transformation met."""
    import mesh_eval_ref
    tgt = mesh_eval_ref.five_spheres()[0]
    rng = np.random.default_rng(FIXTURE_SEED[name])
    pick = rng.permutation(len(tgt))[:len(tgt) // 2]
    moved = tgt[pick].astype(np.float64) + rng.normal(0.0, 0.002, (len(pick), 3))
    src = (moved - MOTION[:3, 3]) @ MOTION[:3, :3]                # G^-1 x = R^T (x - t)
    if name == "outliers":
        src = np.concatenate((src, 3.0 + rng.normal(0.0, 0.05, (N_OUTLIERS, 3))))
    src = src.astype(np.float32)
    src.setflags(write=False)
    return src, tgt


@functools.lru_cache(maxsize=None)
def sparse_case(seed=0):
    """A sparse target (M = 65: a grid of a few cells per axis) against a dense source (N = 5000: twenty rows of the reduction),
    max_dist 0.6 = several cell widths: -> (source, target) fp32.  The target fills the unit cube; the source fills the cube
    [-0.5, 1.5]^3, slightly moved, so that part of it has no correspondence."""
    rng = np.random.default_rng(seed)
    tgt = rng.random((65, 3)).astype(np.float32)
    g = rigid((0.3, -1.0, 0.5), 2.0, (0.01, 0.02, -0.015))
    src = ((rng.random((5000, 3)) * 2.0 - 0.5 - g[:3, 3]) @ g[:3, :3]).astype(np.float32)
    return src, tgt


SPARSE_MAX_DIST = 0.6


@functools.lru_cache(maxsize=None)
def reference(name, max_iter=30, fixed=False):
    """icp() on a fixture, computed once and shared: the default criteria, or `fixed` (both criteria 0: exactly max_iter updates)."""
    src, tgt = fixture(name)
    rel = 0.0 if fixed else 1e-6
    return icp(src, tgt, MAX_DIST[name], None, max_iter, rel, rel)
