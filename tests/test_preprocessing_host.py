"""lmx.services.preprocessing (the mirror of services/video-preprocessing/app/main.py:39-149) and lmx_h_crop_box (csrc/host_crop.cpp),
without a GPU: the crop box on hand-derived cases, from Python and from C, which must agree; the confidence rule in front of it; the
`video.preprocessed` message key for key; and encoder_box, the documented departure for odd sides."""
import ctypes as C

import numpy as np
import pytest

from lmx import _lib
from lmx.services import preprocessing as P


def c_crop_box(boxes, width, height, pad=50):
    lib = _lib.load()
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    ptr = b.ctypes.data_as(C.POINTER(C.c_float)) if b.size else None
    assert lib.lmx_h_crop_box(ptr, b.shape[0], height, width, pad, out) == 0, lib.lmx_last_error().decode()
    return list(out)


# (name, boxes xyxy, width, height, the box derived by hand from main.py:85-110)
CASES = [
    ("no_detection", [], 640, 480, [0, 0, 640, 480]),
    # area 300.2 x 250.4 > 30720; int() of 100.7, 50.2, 400.9, 300.6 = 100, 50, 400, 300; -50 / +50
    ("one_box", [[100.7, 50.2, 400.9, 300.6]], 640, 480, [50, 0, 450, 350]),
    # an even count: the median averages the two middle values: 105.5, 110.5, 415.5, 430.5 -> 105, 110, 415, 430
    ("even_count_averages", [[100, 100, 400, 400], [111, 121, 431, 461]], 640, 480, [55, 60, 465, 480]),
    # 40 x 25 = 1000 = 100 * 100 * 0.1 exactly: "w * h > ..." is strict, the box does not count and the full frame is used
    ("exactly_ten_percent", [[10, 10, 50, 35]], 100, 100, [0, 0, 100, 100]),
    # half a pixel taller: 1020 > 1000; 10 - 50 and 10 - 50 clamp at 0, 50 + 50 reaches the width, 35 + 50 = 85
    ("just_above_ten_percent", [[10, 10, 50, 35.5]], 100, 100, [0, 0, 100, 85]),
    ("padding_clamped_left_top", [[20, 30, 400, 300]], 640, 480, [0, 0, 450, 350]),
    ("padding_clamped_right", [[200, 200, 630, 400]], 640, 480, [150, 150, 640, 450]),
    ("padding_clamped_bottom", [[200, 200, 500, 470]], 640, 480, [150, 150, 550, 480]),
    # int() truncates: 100.99 -> 100, not 101
    ("float_truncates", [[100.99, 150.99, 400.99, 300.99]], 640, 480, [50, 100, 450, 350]),
    # three kept boxes (the 10 x 10 one is far below 10 %): per column the middle value, whatever the order
    ("odd_count_takes_the_middle", [[0, 0, 10, 10], [300, 90, 600, 420], [100, 110, 500, 400], [200, 100, 550, 410]], 640, 480, [150, 50, 600, 460]),
    # every class and any order of frames: only the numbers count; two equal boxes and a third: the median is the repeated value
    ("repeated_boxes", [[100, 100, 400, 400]] * 2 + [[0, 0, 640, 480]], 640, 480, [50, 50, 450, 450]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crop_box_cases_from_python_and_from_c(case):
    _, boxes, width, height, want = case
    got = P.crop_box_of(np.asarray(boxes, np.float32).reshape(-1, 4), width, height)
    assert got == want and all(type(v) is int for v in got), got
    assert c_crop_box(boxes, width, height) == want


def test_python_and_c_agree_on_random_boxes():
    rng = np.random.default_rng(0)
    for trial in range(300):
        width, height = int(rng.integers(50, 2000)), int(rng.integers(50, 1200))
        k = int(rng.integers(0, 13))
        a = rng.random((k, 2), dtype=np.float32) * np.float32(0.6) * np.array([width, height], np.float32)
        size = rng.random((k, 2), dtype=np.float32) * np.array([width, height], np.float32)
        boxes = np.concatenate([a, np.minimum(a + size, np.array([width, height], np.float32))], axis=1).astype(np.float32)
        pad = int(rng.integers(0, 80))
        assert P.crop_box_of(boxes, width, height, pad) == c_crop_box(boxes, width, height, pad), (trial, boxes.tolist(), width, height, pad)


def test_the_float32_median_of_an_even_count():
    """np.median on float32 columns averages in float32: 2^24 + (2^24 + 2) = 2^25 + 2 is no float32 (the spacing there is 4) and rounds
    to even, 2^25, so the median is 2^24 — in double it would be 2^24 + 1.  Both boxes cover half of a 2^25 x 4 frame."""
    big = 2 ** 24
    boxes = [[0, 0, big, 4], [0, 0, big + 2, 4]]
    assert int(np.median(np.array([big, big + 2], np.float32))) == big and int(np.median(np.array([big, big + 2], np.float64))) == big + 1
    assert P.crop_box_of(boxes, 2 ** 25, 4, 0) == [0, 0, big, 4] == c_crop_box(boxes, 2 ** 25, 4, 0)


def test_crop_box_refusals():
    lib = _lib.load()
    boxes = (C.c_float * 4)(0, 0, 10, 10)
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    for args, text in (((boxes, -1, 480, 640, 50, out), "k = -1"), ((boxes, 1, 0, 640, 50, out), "0 x 640"), ((boxes, 1, 480, 640, -1, out), "pad = -1"),
                       ((None, 1, 480, 640, 50, out), "boxes_host"), ((boxes, 1, 480, 640, 50, None), "box_host")):
        assert lib.lmx_h_crop_box(*args) == -1
        msg = lib.lmx_last_error().decode()
        assert "lmx_h_crop_box" in msg and text in msg, msg
    assert list(out) == [-7] * 4


def test_confident_boxes_follow_the_reference_loop():
    """frame by frame, detection by detection, `conf > 0.5` strictly, only the first counts[i] rows of a frame, every class"""
    boxes = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    scores = np.array([[0.9, 0.5, 0.51], [0.7, 0.95, 0.99]], np.float32)
    got = P.confident_boxes(boxes, scores, np.array([3, 1]))
    assert got.dtype == np.float32 and got.tolist() == [boxes[0, 0].tolist(), boxes[0, 2].tolist(), boxes[1, 0].tolist()]
    assert P.confident_boxes(boxes, scores, np.array([0, 0])).shape == (0, 4)


class _FakeDetector:
    """YoloDetector.detect's tables from a list of per-frame [(box, score)]"""

    def __init__(self, per_frame):
        self.per_frame, self.calls = per_frame, []

    def detect(self, frames, conf=0.25):
        import torch

        n = frames.shape[0]
        self.calls.append((n, conf))
        boxes, scores = torch.zeros((n, 4, 4)), torch.zeros((n, 4))
        counts = torch.zeros((n,), dtype=torch.int32)
        for i in range(n):
            for j, (b, s) in enumerate(self.per_frame[i]):
                boxes[i, j], scores[i, j] = torch.tensor(b), s
            counts[i] = len(self.per_frame[i])
        return boxes, scores, torch.zeros((n, 4)), torch.zeros((n, 4)), counts


def test_video_preprocessor_crop_box_reads_ten_frames_at_the_models_confidence():
    import torch

    a, b, late = [100.0, 100.0, 400.0, 400.0], [111.0, 121.0, 431.0, 461.0], [0.0, 0.0, 640.0, 480.0]
    per_frame = [[(a, 0.9)], [(b, 0.8), (late, 0.4)]] + [[] for _ in range(8)] + [[(late, 0.99)]] * 2  # frames 10 and 11 are never read
    det = _FakeDetector(per_frame)
    vp = P.VideoPreprocessor(det)
    frames = torch.zeros((12, 480, 640, 3), dtype=torch.uint8)
    assert vp.crop_box(frames, 640, 480) == [55, 60, 465, 480]
    assert det.calls == [(10, 0.25)]
    assert vp.crop_box(frames[:0], 640, 480) == [0, 0, 640, 480] and len(det.calls) == 1
    assert P.VideoPreprocessor(_FakeDetector([[(late, 0.5)]])).crop_box(frames[:1], 640, 480) == [0, 0, 640, 480]  # conf > 0.5 is strict


def test_message_keys_and_values():
    msg = P.message("vid7", "/app/data/videos/vid7.mp4", "/app/data/processed/vid7_cropped.mp4", [55, 60, 465, 470], 25, 750)
    assert list(msg) == ["video_id", "original_path", "processed_path", "crop_box", "fps", "width", "height", "total_frames"]
    assert msg == {"video_id": "vid7", "original_path": "/app/data/videos/vid7.mp4", "processed_path": "/app/data/processed/vid7_cropped.mp4",
                   "crop_box": [55, 60, 465, 470], "fps": 25, "width": 410, "height": 410, "total_frames": 750}
    from pathlib import Path

    assert P.VideoPreprocessor.message("v", Path("/a/b.mp4"), Path("/c/d.mp4"), [0, 0, 4, 2], 30, 1)["original_path"] == "/a/b.mp4"


def test_encoder_box_shrinks_odd_sides_only():
    assert P.encoder_box([55, 60, 465, 470]) == [55, 60, 465, 470]  # 410 x 410
    assert P.encoder_box([55, 60, 466, 470]) == [55, 60, 465, 470]  # 411 wide
    assert P.encoder_box([55, 61, 465, 470]) == [55, 61, 465, 469]  # 409 high
    assert P.encoder_box([1, 1, 4, 4]) == [1, 1, 3, 3]
    assert P.VideoPreprocessor.encoder_box([0, 0, 640, 480]) == [0, 0, 640, 480]
