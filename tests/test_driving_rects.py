"""host_models.driving_rects: the crop policy of a driving video, on constructed detector rows (H = 360, so a view pixel is a
source pixel)."""
import pytest
import torch

from tests.util import load_pkg

hm = load_pkg().host_models
H, W = 360, 640


def box(cx, cy, half=40, score=0.99):
    return [float(cx - half), float(cy - half), float(cx + half), float(cy + half), score]


def bbox_of(b):
    """process_img's rect for one frame whose detector returns `b`"""
    class FA:
        class face_detector:
            @staticmethod
            def detect_from_image(arr):
                return [tuple(b)]
    saved, hm._FA = hm._FA, FA()
    try:
        return hm.process_img(torch.zeros(H, W, 3), 64, 1.6)[1]
    finally:
        hm._FA = saved


def test_still_video_is_process_img(monkeypatch):
    monkeypatch.delenv("FLOAT_AMD_FACE_DETECTOR", raising=False)
    b = box(300, 170, 45)
    low = [10.0, 10.0, 90.0, 90.0, 0.9]  # below 0.95: not a face
    rects = hm.driving_rects([[low, b]] * 3, [0, 5, 9], 10, H, W)
    assert rects == [bbox_of(b)] * 10


def test_fixed_is_the_union_rule():
    rects = hm.driving_rects([[box(200, 150)], [box(320, 190)]], [0, 7], 8, H, W, margin=1.5)
    # union (160, 110) ... (360, 230): centre (260, 170), half sides 100 and 60 -> int(100 * 1.5)
    assert rects == [(260 - 150, 170 - 150, 300, 300)] * 8


def test_tracking_follows_the_nearer_centre():
    """two faces swap sides; index 2 picks the one that starts on the right, and the order of the rows flips on the way"""
    rows = [[box(100 + 50 * k, 170), box(500 - 50 * k, 200)][::1 if k < 5 else -1] for k in range(9)]
    got = hm.driving_rects(rows, list(range(9)), 9, H, W, index=2, crop="track", smooth=1, margin=1.0)
    assert [r[0] + 40 for r in got] == [500 - 50 * k for k in range(9)]


@pytest.mark.parametrize("rows,want", [
    ([[], [box(200, 150)], [], [box(400, 150)]], [200, 200, 200, 400]),  # later, own, earlier, own
    ([[], [], [], []], None)])
def test_frames_without_a_face(rows, want, caplog):
    import logging
    with caplog.at_level(logging.WARNING):
        got = hm.driving_rects(rows, [0, 1, 2, 3], 4, H, W, crop="track", smooth=1, margin=1.0, logger=logging.getLogger("t"))
    if want is None:
        assert got == [(140, 0, 360, 360)] * 4 == hm.driving_rects(None, None, 4, H, W, crop=None) and len(caplog.records) == 1
    else:
        assert [r[0] + 40 for r in got] == want and not caplog.records


def test_track_returns_linear_motion():
    T, smooth = 41, 9
    idx = hm.driving_detect_frames(T, 5)
    got = hm.driving_rects([[box(100 + 5 * t, 120 + 2 * t)] for t in idx], idx, T, H, W, crop="track", smooth=smooth, margin=1.5)
    assert all(r[2] == r[3] == 120 for r in got)
    for t in range(smooth // 2, T - smooth // 2):
        assert got[t][:2] == (100 + 5 * t - 60, 120 + 2 * t - 60), t


def test_detect_frames_include_the_last():
    assert hm.driving_detect_frames(12, 5) == [0, 5, 10, 11] and hm.driving_detect_frames(11, 5) == [0, 5, 10]
    assert hm.driving_detect_frames(1, 5) == [0]
