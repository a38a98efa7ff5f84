"""A synthetic sequence for the driver's tests (tests/test_gpu_slam_run.py): ``synthetic.make_scene``'s box room seen from cameras
that move a little from frame to frame (``synthetic.SyntheticSequence``), as the dataset interface ``slam.DNS_SLAM`` takes (``__len__``, ``__getitem__``, ``n_class``,
``class2label_dict``), and the configuration of a small run."""
from dns_slam_amd import synthetic


class SynthSequence(synthetic.SyntheticSequence):
    """``synthetic.SyntheticSequence`` at the tests' size: eight frames of 48 x 64."""

    def __init__(self, n=8, H=48, W=64, fx=50.0, step=0.04, seed=0):
        super().__init__(n=n, H=H, W=W, fx=fx, step=step, seed=seed)


def run_cfg(seq, out_dir, **mapping):
    """The keys a run reads, sized for a test: a few iterations, tens of rays."""
    cfg = synthetic.default_cfg(n_pixels=96, n_samples_ray=16, n_surface_ray=9, n_frames=4, hash_size=12, voxel_size=0.16,
                                smooth_pts=8, track_pixels=48, track_iters=3)
    cam = seq.cam
    cfg["cam"] = {"H": cam["H"], "W": cam["W"], "fx": cam["fx"], "fy": cam["fy"], "cx": cam["cx"], "cy": cam["cy"], "crop_edge": 0}
    cfg["back_end"] = {"bound": synthetic.ROOM0_BOUND}
    cfg["bound_divisible"] = 0.32
    cfg["scale"] = 1
    cfg["scene"], cfg["out_dir"] = "synth", out_dir
    cfg["sync_method"], cfg["verbose"], cfg["const_speed_assumption"], cfg["use_gt_camera"] = "strict", True, True, False
    cfg["mapping"].update({"n_iters": 4, "n_iters_first": 6, "optimize_every_n_frames": 3, "choose_keyframe_every": 3, "vis_every": 3,
                           "mesh_every": 6, "checkpoint_every": 3, "start_optimize_idx": 2, "n_pts_batch": 1024})
    cfg["mapping"].update(mapping)
    cfg["meshing"] = {"resolution": 24, "level_set": 0.0, "points_batch_size": 1 << 16, "clean_mesh": False, "color": True}
    return cfg
