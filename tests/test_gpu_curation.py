"""clip-curation behind the per-frame records on the GPU (lmx/services/curation.py): the frames of the canonical clip against
lmx.letterbox.letterbox_reference, and ClipCurator.curate on a short synthetic clip — its visual table against tests/qualityref.py, its
report against the host functions run on that table, and the selection following the sharp half of the clip."""
import numpy as np
import pytest
import torch

import qualityref as Q
from lmx import letterbox as LB
from lmx.services import ClipCurator
from lmx.services import curation as C

pytestmark = pytest.mark.gpu


def candidate(start, flip):
    return C.ClipCandidate(start, start + 125, 0.0, 5.0, C.QualityMetrics(0, 0, 0, 0, 0, 0), flip)


def resized_reference(frames, idx, flip):
    sh, sw = frames.shape[1:3]
    geo = LB.LetterboxGeo(sh, sw, 720, 1280, 0, 0, 720, 1280, min(720 / sh, 1280 / sw), 0.0, 0.0)
    want = np.stack([LB.letterbox_reference(frames[i], geo, swap_rb=False) for i in idx], 0)
    return want[:, :, ::-1].copy() if flip else want


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape,fps,start", [((2, 1080, 1920), 25.0, 0), ((5, 37, 53), 50.0, 1)], ids=["1080p", "37x53"])
def test_canonical_frames_equal_the_resize_reference(cuda, shape, fps, start, flip):
    """cv2.resize(frame, (1280, 720)) as lmx.letterbox restates it (PARITY UNPINNED against real cv2), shrinking 1080p and enlarging a
    small odd frame; at 50 fps every second frame is taken until the clip ends"""
    n, h, w = shape
    frames = Q.random_frames(n, h, w, seed=h)
    idx = C.canonical_frame_indices(start, n, fps)
    assert idx == ([0, 1] if n == 2 else [1, 3])
    got = C.canonical_frames(torch.from_numpy(frames).to(cuda), candidate(start, flip), fps)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(idx), 720, 1280, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(resized_reference(frames, idx, flip)))


def test_a_720p_source_passes_through(cuda):
    frames = Q.random_frames(3, 720, 1280, seed=2)
    dev = torch.from_numpy(frames).to(cuda)
    got = C.canonical_frames(dev, candidate(1, False), 25.0)
    assert torch.equal(got.cpu(), torch.from_numpy(frames[1:])) and got.data_ptr() != dev[1:].data_ptr()  # a copy, as cv2.resize returns one
    assert torch.equal(C.canonical_frames(dev, candidate(1, True), 25.0).cpu(), torch.from_numpy(frames[1:, :, ::-1].copy()))
    assert tuple(C.canonical_frames(dev, candidate(3, False), 25.0).shape) == (0, 720, 1280, 3)  # a window behind the clip's end


# ---- ClipCurator.curate.  The detector's synthetic weights find no cow walking through synthetic frames, so the tracker's records are
# injected: two equal walks (frames 0..49 and 51..100, no detection on frame 50) through a 48 x 64 frame, authored as in
# tests/test_curation_host.py.  Everything behind the records runs as shipped: K.frame_quality over the curator's batches, the one host
# copy, the host steps.
H, W, FPS, N = 48, 64, 10.0, 101


def records():
    out = []
    for f in range(N):
        if f == 50:
            out.append({"frame": f, "time": f / FPS, "detection": None})
            continue
        cx, cy = 16.0 + 0.6 * (f % 51), 24.0
        out.append({"frame": f, "time": f / FPS,
                    "detection": {"bbox": [cx - 10, cy - 12, cx + 10, cy + 12], "confidence": 0.8, "centroid": (cx, cy), "area": 480.0}})
    return out


def clip(sharp_first):
    """a ramp around mid-gray with noise of amplitude 64 (Laplacian variance far above 500: blur score 1) on the sharp half and of
    amplitude 4 (variance some tens: blur score below 0.2) on the blurred half; frame 50 belongs to the first half"""
    rng = np.random.default_rng(4)
    ramp = (96 + np.add.outer(np.arange(H), np.arange(W)) // 2).astype(np.int64)[None, :, :, None]
    amp = np.where((np.arange(N) <= 50) == sharp_first, 64, 4)[:, None, None, None]
    return (ramp + rng.integers(0, 65, (N, H, W, 3)) * amp // 64).astype(np.uint8)


@pytest.fixture(scope="module")
def curated(cuda):
    cur = ClipCurator(detector=None, conf=0.3, batch=32)  # 101 frames: three whole batches and a rest of 5
    cur.tracker.track = lambda frames, fps, first_frame=0: records()
    out = {}
    for sharp_first in (True, False):
        frames = clip(sharp_first)
        out[sharp_first] = (frames, cur.curate("clip", torch.from_numpy(frames).to(cuda), FPS))
    return out


@pytest.mark.parametrize("sharp_first", [True, False])
def test_curate_equals_the_host_steps_on_the_reference_table(curated, sharp_first):
    frames, got = curated[sharp_first]
    blur, bright = C.visual_scores(Q.sums(frames))
    visual = (blur + bright) / 2
    assert np.array_equal(got["visual"], visual)
    first, second = (blur[:51], blur[51:]) if sharp_first else (blur[51:], blur[:51])
    assert (first == 1.0).all() and (second < 0.2).all() and (second > 0.0).all()
    info = {"fps": FPS, "width": W, "height": H, "total_frames": N, "duration": N / FPS}
    passes = C.identify_walking_passes(records(), info)
    assert [(p.start_frame, p.end_frame) for p in passes] == [(0, 49), (51, 100)]
    selected, backup = C.select_windows(passes, info, visual)
    assert got["selected"] == selected and got["backup"] == backup
    assert got["report"] == C.generate_quality_report("clip", info, passes, selected, backup)
    assert got["report"]["status"] == "success" and got["report"]["source_video"]["total_frames"] == N


def test_blurring_the_other_half_moves_the_selection(curated):
    a, b = curated[True][1], curated[False][1]
    assert (a["selected"].start_frame, a["backup"].start_frame) == (0, 51)
    assert (b["selected"].start_frame, b["backup"].start_frame) == (51, 0)
    # the two windows differ in the visual score alone
    ma, mb = a["selected"].metrics, a["backup"].metrics
    assert (ma.framing_score, ma.steadiness_score, ma.straightness_score, ma.occlusion_score) == (mb.framing_score, mb.steadiness_score,
                                                                                                 mb.straightness_score, mb.occlusion_score)
    assert ma.visual_quality_score > mb.visual_quality_score
