"""CPU: slam.schedule against event lists written out by hand from the conditions of the reference's Mapper.run
(slams/mapping.py:952-1146) and Tracker.run (slams/tracking.py:229-376) under sync_method 'strict'."""
import pytest

from dns_slam_amd.slam import schedule


def _cfg(every=3, kf=3, vis=3, mesh=6, ckpt=3, verbose=True, sync="strict", n_iters=100, n_first=300):
    return {"sync_method": sync, "verbose": verbose,
            "mapping": {"optimize_every_n_frames": every, "choose_keyframe_every": kf, "vis_every": vis, "mesh_every": mesh,
                        "checkpoint_every": ckpt, "n_iters": n_iters, "n_iters_first": n_first}}


FIRST = ("map", 1, 300, ("overlap",))
LATER = lambda i: ("map", i, 50, ("overlap", "global"))   # noqa: E731


def test_the_example():
    assert schedule(8, _cfg()) == [
        ("keyframe", 0),
        FIRST, ("vis", 1),
        ("track", 2), ("track", 3),
        LATER(3), ("vis", 3), ("keyframe", 3), ("checkpoint", "model_3.pt"),
        ("track", 4), ("track", 5), ("track", 6),
        LATER(6), ("vis", 6), ("keyframe", 6), ("mesh", 6), ("checkpoint", "model_6.pt"),
        ("track", 7),
        LATER(7), ("vis", 7), ("checkpoint", "model.pt"),
    ]


def test_every_frame_is_mapped_with_period_one():
    # idx % 1 == 0 always: every tracked frame is mapped; keyframes every 2 frames and at n_img - 2 = 3
    assert schedule(5, _cfg(every=1, kf=2, vis=0, mesh=0, ckpt=0)) == [
        ("keyframe", 0),
        FIRST,
        ("track", 2), LATER(2), ("keyframe", 2),
        ("track", 3), LATER(3), ("keyframe", 3),
        ("track", 4), LATER(4), ("keyframe", 4), ("vis", 4), ("checkpoint", "model.pt"),
    ]


def test_last_frame_a_multiple_of_the_period():
    # n_img - 1 = 6 = 2 * 3: mapped once; vis_every = 3 draws frame 6 twice, as the reference does (:1075 and :1136)
    assert schedule(7, _cfg(mesh=0, ckpt=0)) == [
        ("keyframe", 0),
        FIRST, ("vis", 1),
        ("track", 2), ("track", 3), LATER(3), ("vis", 3), ("keyframe", 3),
        ("track", 4), ("track", 5), ("track", 6), LATER(6), ("vis", 6), ("keyframe", 6), ("vis", 6), ("checkpoint", "model.pt"),
    ]


def test_last_frame_not_a_multiple_of_the_period():
    # n_img - 1 = 5: mapped because it is the last frame (:994); 5 is no keyframe (5 % 3 != 0, 5 != n_img - 2)
    assert schedule(6, _cfg(vis=0, mesh=0, ckpt=0)) == [
        ("keyframe", 0),
        FIRST,
        ("track", 2), ("track", 3), LATER(3), ("keyframe", 3),
        ("track", 4), ("track", 5), LATER(5), ("vis", 5), ("checkpoint", "model.pt"),
    ]


def test_the_second_to_last_frame_becomes_a_keyframe_when_it_is_mapped():
    # n_img = 6, period 2: frame 4 = n_img - 2 is mapped; choose_keyframe_every = 5 alone would not choose it
    assert schedule(6, _cfg(every=2, kf=5, vis=0, mesh=0, ckpt=0)) == [
        ("keyframe", 0),
        FIRST,
        ("track", 2), LATER(2),
        ("track", 3),
        ("track", 4), LATER(4), ("keyframe", 4),
        ("track", 5), LATER(5), ("keyframe", 5), ("vis", 5), ("checkpoint", "model.pt"),
    ]


def test_the_second_to_last_frame_cannot_be_a_keyframe_when_it_is_not_mapped():
    # n_img = 7, period 3: frame 5 = n_img - 2 is never mapped, so the idx == n_img - 2 rule adds nothing
    ev = schedule(7, _cfg(kf=4, vis=0, mesh=0, ckpt=0))
    assert ev == [
        ("keyframe", 0),
        FIRST,
        ("track", 2), ("track", 3), LATER(3),
        ("track", 4), ("track", 5), ("track", 6), LATER(6), ("vis", 6), ("checkpoint", "model.pt"),
    ]
    assert ("keyframe", 5) not in ev


@pytest.mark.parametrize("off,gone", [("vis", "vis"), ("mesh", "mesh"), ("ckpt", "checkpoint")])
def test_a_period_of_zero_switches_an_output_off(off, gone):
    full = schedule(8, _cfg())
    ev = schedule(8, _cfg(**{off: 0}))
    # the last frame's frame_vis and model.pt are unconditional (:1133-1145)
    keep = [e for e in full if e[0] != gone or e in (("vis", 7), ("checkpoint", "model.pt"))]
    assert ev == keep
    assert [e for e in ev if e[0] == gone] == ([("vis", 7)] if gone == "vis" else [("checkpoint", "model.pt")] if gone == "checkpoint" else [])


def test_not_verbose_draws_and_meshes_nothing_but_the_last_frame():
    assert schedule(8, _cfg(verbose=False)) == [
        ("keyframe", 0),
        FIRST,
        ("track", 2), ("track", 3), LATER(3), ("keyframe", 3), ("checkpoint", "model_3.pt"),
        ("track", 4), ("track", 5), ("track", 6), LATER(6), ("keyframe", 6), ("checkpoint", "model_6.pt"),
        ("track", 7), LATER(7), ("vis", 7), ("checkpoint", "model.pt"),
    ]


def test_two_frames_and_too_few():
    assert schedule(2, _cfg(vis=0, mesh=0, ckpt=0)) == [("keyframe", 0), FIRST, ("vis", 1), ("checkpoint", "model.pt")]
    with pytest.raises(ValueError):
        schedule(1, _cfg())


@pytest.mark.parametrize("sync", ["loose", "free"])
def test_other_sync_methods_are_refused(sync):
    with pytest.raises(NotImplementedError, match="strict"):
        schedule(8, _cfg(sync=sync))


def test_use_gt_camera_tracks_nothing():
    cfg = _cfg(vis=0, mesh=0, ckpt=0)
    cfg["use_gt_camera"] = True
    assert schedule(6, cfg) == [("keyframe", 0), FIRST, LATER(3), ("keyframe", 3), LATER(5), ("vis", 5), ("checkpoint", "model.pt")]
