"""lmx_k_tleap_series (csrc/tleap.hip) against its host twin lmx_h_tleap_series on hand-made detection tensors: every output (rows, the
records of each clip's rows, series, mask) must be equal bit for bit (np.array_equal; the inputs hold no NaN).  The shapes cross every
chunk seam of the 256-frame scan, the crop / pad boundaries of the 125-step window, both modes and the mask's threshold."""
import numpy as np
import pytest
import torch

from lmx import kernels as K

pytestmark = pytest.mark.gpu
COWS = (3, 19)
HW = (720, 1280)


def detections(frame_counts, max_det, K_=None, ndim=3, seed=0):
    """Random detector outputs for frames with the given counts; every slot is filled (slots beyond a count must not be read as rows)."""
    rng = np.random.default_rng(seed)
    F = len(frame_counts)
    boxes = rng.uniform(0, 1200, (F, max_det, 4)).astype(np.float32)
    boxes[..., 2:] = boxes[..., :2] + rng.uniform(0.2, 500, (F, max_det, 2)).astype(np.float32)
    t = {"boxes": boxes, "scores": rng.uniform(0.3, 1, (F, max_det)).astype(np.float32),
         "cls": rng.choice(np.array([0, 3, 7, 19], np.int32), (F, max_det)).astype(np.int32), "counts": np.asarray(frame_counts, np.int32), "kpts": None}
    if K_ is not None:
        t["kpts"] = rng.uniform(0, 1300, (F, max_det, K_, ndim)).astype(np.float32)
        if ndim == 3:
            t["kpts"][..., 2] = rng.uniform(0, 1, (F, max_det, K_)).astype(np.float32)
            t["kpts"][:, :, 2, 2] = rng.choice(np.array([0.3, np.nextafter(np.float32(0.3), np.float32(0)), 0.0, 0.31, 0.9], np.float32), (F, max_det))
    return t


def run(t, first, dev=None, target=125):
    ops = [torch.from_numpy(t[k]) if t[k] is not None else None for k in ("boxes", "scores", "cls", "counts", "kpts")]
    if dev is not None:
        ops = [o.to(dev) if o is not None else None for o in ops]
    rows, rec, series, mask = K.tleap_series(*ops, HW, first, target, COWS, host=dev is None)
    rows, rec = rows.cpu().numpy(), rec.cpu().numpy()
    md = t["boxes"].shape[1]
    return rows, [rec[first[c] * md:first[c] * md + rows[c]] for c in range(len(rows))], series.cpu().numpy(), mask.cpu().numpy()


def check(t, first, dev, target=125):
    """device == host on every output; returns the host's"""
    host, got = run(t, first, None, target), run(t, first, dev, target)
    assert np.array_equal(got[0], host[0]), (got[0], host[0])
    for c, (g, h) in enumerate(zip(got[1], host[1])):
        assert np.array_equal(g, h), f"records of clip {c}"
    assert np.array_equal(got[2], host[2]) and np.array_equal(got[3], host[3])
    assert not np.isnan(host[2]).any()
    return host


def clip_slice(t, a, b):
    return {k: (v[a:b] if v is not None else None) for k, v in t.items()}


def bounds(lengths):
    return [int(v) for v in np.cumsum([0] + list(lengths))]


@pytest.mark.parametrize("mode", ["trained", "heuristic"])
def test_window_boundaries(cuda, mode):
    """T0 = 1, 124 (pads 0 in front, 1 behind), 125, 126, 127 (the first crop with start 1: the first step's velocity differences a row
    outside the window), 128 and 300, one row per frame"""
    T0s = [1, 124, 125, 126, 127, 128, 300]
    t = detections([1] * sum(T0s), 2, 20 if mode == "trained" else None, seed=1)
    if mode == "heuristic":
        t["cls"][:, 0] = 19
    rows, _, series, mask = check(t, bounds(T0s), cuda)
    assert rows.tolist() == T0s
    assert mask[0].sum() >= 124 and not series[0, :62].any() and series[0, 62].any()
    assert series[4, 0, 43] != 0.0  # T0 = 127: the velocity of the first kept step is against row 0, outside the crop


@pytest.mark.parametrize("mode", ["trained", "heuristic"])
def test_scan_seams(cuda, mode):
    """1, 255, 256, 257 and 600 frames with counts cycling 0, 1, 2, 3 and one frame at max_det: every seam of the 256-frame chunks"""
    lengths, md = [1, 255, 256, 257, 600], 5
    counts = [i % 4 for i in range(sum(lengths))]
    counts[0] = 1
    counts[300], counts[1000] = md, md
    t = detections(counts, md, 20 if mode == "trained" else None, seed=2)
    rows, rec, _, _ = check(t, bounds(lengths), cuda)
    if mode == "trained":
        first = bounds(lengths)
        assert rows.tolist() == [sum(counts[first[c]:first[c + 1]]) for c in range(5)]
        c4 = np.repeat(np.arange(600), counts[first[4]:first[5]])
        assert np.array_equal(rec[4].view(K.tleap_record_dtype()).reshape(-1)["frame"], c4)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("K_", [17, 20, 23])
def test_trained_keypoint_shapes(cuda, K_, ndim):
    t = detections([i % 4 for i in range(70)], 3, K_, ndim, seed=3 + K_ + ndim)
    _, rec, _, _ = check(t, bounds([30, 40]), cuda)
    r = rec[1].view(K.tleap_record_dtype()).reshape(-1)
    assert (r["n_kp"] == min(K_, 20)).all() and (r["keypoints"][:, min(K_, 20):] == 0).all()
    if ndim == 3:
        assert (r["keypoints"][:, 2, 2] == 0.8).any() and (r["keypoints"][:, 2, 2] == float(np.float32(0.3))).any()  # fallback and model both occur


def test_clips_without_a_detection(cuda):
    """a trained clip with T0 = 0 (zero series, full mask) beside one with rows; a heuristic clip where every frame takes the assumed box"""
    t = detections([0] * 7 + [2] * 3, 2, 17, seed=5)
    rows, _, series, mask = check(t, bounds([7, 3]), cuda)
    assert rows.tolist() == [0, 6] and not series[0].any() and mask[0].all()
    t = detections([0, 2, 1, 0, 2], 2, None, seed=6)
    t["cls"][:] = 7
    rows, rec, _, mask = check(t, bounds([5]), cuda)
    r = rec[0].view(K.tleap_record_dtype()).reshape(-1)
    assert rows.tolist() == [5] and (r["det"] == -1).all() and (r["confidence"] == 0.5).all() and np.array_equal(r["bbox"][0], [1280 * 0.1, 720 * 0.1, 1280 * (1 - 0.1), 720 * (1 - 0.1)])
    assert not mask[0, 60:65].any()  # 0.705 x 0.5 is above the threshold


def test_mask_threshold_and_thin_boxes(cuda):
    """heuristic rows with detection confidences 0.4255 and 0.4256: 0.705 x them is 0.29998 and 0.30005, either side of 0.3; boxes 0.5 and
    exactly 1.0 wide and high (the divisors max(bbox_w, 1) / max(bbox_h, 1))"""
    t = detections([1, 1, 1, 1], 1, None, seed=7)
    t["cls"][:] = 19
    t["scores"][:, 0] = [0.4255, 0.4256, 0.9, 0.9]
    t["boxes"][2, 0] = [100.25, 50.5, 100.75, 51.0]
    t["boxes"][3, 0] = [200.0, 80.0, 201.0, 81.0]
    _, _, series, mask = check(t, bounds([4]), cuda)
    assert mask[0, 60:64].tolist() == [1, 0, 0, 0] and mask[0].sum() == 122
    assert series[0, 62, 42] == np.float32(0.5 * 0.5 / (1280 * 720)) and series[0, 63, 42] == np.float32(1.0 / (1280 * 720))


@pytest.mark.parametrize("mode", ["trained", "heuristic"])
def test_batch_position_invariance(cuda, mode):
    """five clips of differing length in one launch, each equal to the same clip launched alone"""
    lengths = [3, 140, 1, 61, 260]
    t = detections([(3 * i) % 4 for i in range(sum(lengths))], 3, 23 if mode == "trained" else None, seed=8)
    first = bounds(lengths)
    rows, rec, series, mask = check(t, first, cuda)
    for c in range(5):
        r1, rec1, s1, m1 = run(clip_slice(t, first[c], first[c + 1]), [0, lengths[c]], cuda)
        assert r1[0] == rows[c] and np.array_equal(rec1[0], rec[c]) and np.array_equal(s1[0], series[c]) and np.array_equal(m1[0], mask[c])


@pytest.mark.parametrize("max_det", [1, 300])
def test_max_det(cuda, max_det):
    counts = [min(max_det, c) for c in [0, 1, 300, 2, 299, 1, 0, 300, 7]]
    check(detections(counts, max_det, 20, seed=9), bounds([4, 5]), cuda)
    t = detections(counts, max_det, None, seed=10)
    t["counts"][1], t["counts"][2] = -3, max_det + 5  # clamped to 0 .. max_det
    check(t, bounds([9]), cuda, target=16)
