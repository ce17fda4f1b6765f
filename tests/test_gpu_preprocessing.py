"""lmx.services.preprocessing on the GPU: VideoPreprocessor.crop_box on synthetic frames equals the box lmx_h_crop_box computes from
the detector's own detections (at the reference's thresholds, and at thresholds placed inside the synthetic detector's scores so that
boxes pass), and cropped() equals the reference conversion (tests/yuvoutref.py) of the sliced frames, from BGR frames and from the
decoder's planes, for a box with odd sides."""
import ctypes as C

import numpy as np
import pytest
import torch

import yuvoutref
import yuvref
from lmx import _lib
from lmx.services import VideoPreprocessor
from lmx.services import preprocessing as P
from test_gpu_native_yolo import make_frames

pytestmark = pytest.mark.gpu
H, W, N = 180, 320, 12


@pytest.fixture(scope="module")
def detector(cuda):
    from lmx import yolo

    cfg = yolo.YoloConfig("n", nc=80, imgsz=320)
    return yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7, yolo.bn_stats_path("n")), cuda)


def c_crop_box(boxes, width, height, pad=50):
    lib = _lib.load()
    b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    out = (C.c_int32 * 4)()
    assert lib.lmx_h_crop_box(b.ctypes.data_as(C.POINTER(C.c_float)) if b.size else None, b.shape[0], height, width, pad, out) == 0
    return list(out)


def test_crop_box_equals_the_host_function_on_the_detectors_detections(cuda, detector):
    frames = torch.from_numpy(make_frames(H, W, N)).to(cuda)
    # the detector's own tables on the first 10 frames, as the reference's loop reads them
    boxes, scores, _, _, counts = (t.cpu().numpy() for t in detector.detect(frames[:10], conf=0.25))
    vp = VideoPreprocessor(detector)
    want = c_crop_box([boxes[i, j] for i in range(10) for j in range(int(counts[i])) if scores[i, j] > 0.5], W, H)
    assert vp.crop_box(frames, W, H) == want
    # synthetic weights score low: thresholds inside the scores, so that some boxes pass and some do not
    low = detector.detect(frames[:10], conf=0.001)
    b, s, n = (low[k].cpu().numpy() for k in (0, 1, 4))
    listed = np.sort(np.concatenate([s[i, : int(n[i])] for i in range(10)]))
    assert listed.size >= 2, "the synthetic detector found nothing at conf 0.001"
    cut = float(listed[listed.size // 2])
    passed = [b[i, j] for i in range(10) for j in range(int(n[i])) if s[i, j] > cut]
    assert 0 < len(passed) < listed.size
    got = VideoPreprocessor(detector, model_conf=0.001, box_conf=cut).crop_box(frames, W, H)
    assert got == c_crop_box(passed, W, H) == P.crop_box_of(np.asarray(passed, np.float32), W, H)
    print("crop boxes:", want, got, "of", len(passed), "confident boxes")


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_cropped_equals_the_reference_conversion_of_the_sliced_frames(cuda, layout):
    vp = VideoPreprocessor(None)
    box = [33, 21, 234, 152]  # 201 x 131: both sides odd, the encoder's box is 200 x 130
    x1, y1, x2, y2 = vp.encoder_box(box)
    assert (x2 - x1, y2 - y1) == (200, 130)
    frames = yuvoutref.random_bgr(H, W, 3, seed=31)
    want = yuvoutref.from_bgr(frames[:, y1:y2, x1:x2], "bt709")
    want = (want[0], yuvref.interleave(want[1], want[2])) if layout == "nv12" else want
    got = vp.cropped(torch.from_numpy(frames).to(cuda), box, layout=layout, matrix="bt709")
    assert len(got) == len(want) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    # from the decoder's planes: the window to BGR at the box's parity, then back
    y, u, v = yuvref.random_frame(H, W, 3, seed=32)
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
    bgr = yuvoutref.window(y, c, H, W, (x1, y1, x2 - x1, y2 - y1), layout, "bt709", v=vv)
    want = yuvoutref.from_bgr(bgr, "bt709")
    want = (want[0], yuvref.interleave(want[1], want[2])) if layout == "nv12" else want
    planes = tuple(torch.from_numpy(np.ascontiguousarray(p)).to(cuda) for p in ((y, c) if layout == "nv12" else (y, u, v)))
    got = vp.cropped(planes, box, layout=layout, matrix="bt709")
    assert len(got) == len(want) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
