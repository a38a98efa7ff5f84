"""CPU: the host reference of the mesh evaluation (tests/mesh_eval_ref.py) against known answers, the premises of the GPU
tests' exclusion rules, and dns_slam_amd.evaluation's host-side readers (read_ply, load_poses)."""
import os

import numpy as np
import pytest

import mesh_eval_ref as R


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_metrics_on_two_planes(seed):
    """Planes z = 0 (16 x 16 quads) and z = 0.03 (12 x 12 quads), 20 000 samples each: every nearest neighbour is 3 cm away
    plus the in-plane distance to the nearest sample (3.026 / 3.027 cm measured with scipy for seeds 0 / 1)."""
    rng = np.random.default_rng(seed)
    (v0, f0), (v1, f1) = R.plane(16, 0.0), R.plane(12, 0.03)
    rec = R.sample_surface(v0, f0, rng.random((20000, 3)))[0].astype(np.float32)
    gt = R.sample_surface(v1, f1, rng.random((20000, 3)))[0].astype(np.float32)
    acc, comp, ratio = R.accuracy(gt, rec) * 100, R.completion(gt, rec) * 100, R.completion_ratio(gt, rec) * 100
    print(f"seed {seed}: accuracy {acc:.4f} cm, completion {comp:.4f} cm, ratio {ratio:.2f} %")
    assert 3.0 <= acc <= 3.1 and 3.0 <= comp <= 3.1
    assert ratio == 100.0
    assert (rec[:, 2] == 0).all() and rec[:, :2].min() >= 0 and rec[:, :2].max() <= 1


@pytest.mark.parametrize("name", sorted(R.SAMPLING_CASES))
def test_sampling_cases_exclude_nothing(name):
    """The GPU sampling test leaves out the samples whose pick lies within F 2^-52 total of a CDF entry: none for these seeds.
    The reference never picks a zero-area face and its points lie in their triangles."""
    v, f, u = R.sampling_case(name)
    pts, face, cdf, pick = R.sample_surface(v, f, u)
    assert not R.sample_ambiguous(cdf, pick).any()
    area = R.face_areas(v, f)
    assert (area[face] > 0).all()
    if name == "degenerate_faces":
        assert (area == 0).sum() == 4 and area[0] == 0 and area[-1] == 0
    assert R.barycentric_min(v, f, pts, face).min() >= -1e-9


def test_frustum_case_stays_under_the_exclusion_cap():
    """The GPU frustum test leaves out the vertices within a relative 1e-4 of a test boundary, at most 1 % of them; the poses
    see a real part of the sphere and miss a real part."""
    v, f = R.sphere(0.6, 32)
    w2c = R.world_to_camera(R.frustum_poses())
    seen, near = R.check_proj(v, w2c, **R.FRUSTUM_CAM)
    print(f"{len(v)} vertices, {seen.sum()} seen, {near.sum()} near a boundary")
    assert near.mean() <= 0.01
    assert 0.1 <= seen.mean() <= 0.9
    assert not R.check_proj(v, w2c[:0], **R.FRUSTUM_CAM)[0].any()


def test_lattice_cloud_premise():
    ref, q = R.cloud_lattice()
    assert len(ref) == 17000 and int(np.floor(np.cbrt(2 * len(ref)))) == 32
    d, _ = R.nearest(ref, q)
    assert (d[:17 ** 3] == 0).all() and d[17 ** 3:].min() > 0.4


# ---- PLY ---------------------------------------------------------------------------------------------------------------
def _mesh(seed=0, V=37, F=51):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(V, 3)).astype(np.float32), rng.integers(0, V, (F, 3)).astype(np.int32),
            rng.integers(0, 256, (V, 3)).astype(np.uint8), rng.integers(-1, 40, V).astype(np.int64))


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("with_labels", [False, True])
def test_read_ply_round_trip(tmp_path, with_colors, with_labels):
    from dns_slam_amd.evaluation import read_ply
    from dns_slam_amd.meshing import write_ply
    v, f, c, l = _mesh()
    p = os.path.join(tmp_path, "m.ply")
    write_ply(p, v, f, c if with_colors else None, l if with_labels else None)
    m = read_ply(p)
    assert m["verts"].dtype == np.float32 and m["faces"].dtype == np.int32
    assert np.array_equal(m["verts"], v) and np.array_equal(m["faces"], f)
    assert ("colors" in m) == with_colors and ("labels" in m) == with_labels
    if with_colors:
        assert m["colors"].dtype == np.uint8 and np.array_equal(m["colors"], c)
    if with_labels:
        assert m["labels"].dtype == np.int32 and np.array_equal(m["labels"], l)


def test_read_ply_empty_mesh(tmp_path):
    from dns_slam_amd.evaluation import read_ply
    from dns_slam_amd.meshing import write_ply
    p = os.path.join(tmp_path, "e.ply")
    write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8), np.zeros(0, np.int64))
    m = read_ply(p)
    assert m["verts"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["colors"].shape == (0, 3) and m["labels"].shape == (0,)


def test_read_ply_foreign_header(tmp_path):
    """Reordered and extra vertex properties of several types, a comment, uint indices under the other list name."""
    from dns_slam_amd.evaluation import read_ply
    v, f, c, l = _mesh(1)
    rec = np.dtype([("nx", "<f8"), ("z", "<f4"), ("blue", "u1"), ("x", "<f4"), ("quality", "<i2"), ("red", "u1"), ("y", "<f4"),
                    ("label", "<i4"), ("green", "u1"), ("flags", "<u2")])
    vd = np.zeros(len(v), rec)
    vd["x"], vd["y"], vd["z"] = v[:, 0], v[:, 1], v[:, 2]
    vd["red"], vd["green"], vd["blue"], vd["label"] = c[:, 0], c[:, 1], c[:, 2], l
    vd["nx"], vd["quality"], vd["flags"] = 0.5, -3, 65535
    fd = np.zeros(len(f), np.dtype([("n", "u1"), ("i", "<u4", (3,))]))
    fd["n"], fd["i"] = 3, f
    names = {"<f8": "double", "<f4": "float", "u1": "uchar", "|u1": "uchar", "<i2": "short", "<i4": "int", "<u2": "ushort"}
    header = ["ply", "format binary_little_endian 1.0", "comment made by hand", f"element vertex {len(v)}"]
    header += [f"property {names[rec[n].str]} {n}" for n in rec.names]
    header += [f"element face {len(f)}", "property list uint8 uint vertex_index", "end_header"]
    p = os.path.join(tmp_path, "h.ply")
    with open(p, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii") + vd.tobytes() + fd.tobytes())
    m = read_ply(p)
    assert np.array_equal(m["verts"], v) and np.array_equal(m["faces"], f)
    assert np.array_equal(m["colors"], c) and np.array_equal(m["labels"], l)


def test_read_ply_refusals(tmp_path):
    from dns_slam_amd.evaluation import read_ply
    body = "element vertex 1\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n" \
           "property list uchar int vertex_indices\nend_header\n"
    def write(name, text, tail=b""):
        p = os.path.join(tmp_path, name)
        with open(p, "wb") as fh:
            fh.write(text.encode("ascii") + tail)
        return p
    with pytest.raises(ValueError, match="(?i)ascii"):
        read_ply(write("a.ply", "ply\nformat ascii 1.0\n" + body, b"0 0 0\n"))
    with pytest.raises(ValueError, match="(?i)big.endian"):
        read_ply(write("b.ply", "ply\nformat binary_big_endian 1.0\n" + body, bytes(12)))
    quad = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n" \
           "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
    with pytest.raises(ValueError, match="(?i)triangle"):
        read_ply(write("q.ply", quad, bytes(48) + bytes([4]) + np.arange(4, dtype="<i4").tobytes()))
    with pytest.raises(ValueError, match="(?i)not a PLY"):
        read_ply(write("n.ply", "solid\n"))
    with pytest.raises(ValueError, match="(?i)truncated"):
        read_ply(write("t.ply", "ply\nformat binary_little_endian 1.0\n" + body, bytes(8)))


def test_load_poses(tmp_path):
    from dns_slam_amd.evaluation import load_poses, world_to_camera
    c2w = R.frustum_poses(3)
    p = os.path.join(tmp_path, "traj.txt")
    with open(p, "w") as fh:
        for m in c2w:
            fh.write(" ".join(repr(float(x)) for x in m.ravel()) + "\n")
    got = load_poses(p)
    assert got.shape == (3, 4, 4) and np.array_equal(got, c2w)
    assert np.array_equal(world_to_camera(got), R.world_to_camera(c2w))
    assert np.array_equal(got, c2w)                          # world_to_camera flips a copy
    with open(p, "a") as fh:
        fh.write("1 2 3\n")
    with pytest.raises(ValueError, match="line 4"):
        load_poses(p)
