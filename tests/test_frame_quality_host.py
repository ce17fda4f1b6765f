"""lmx_h_frame_quality (csrc/host_quality.cpp), the plain C++ restatement of the per-frame blur / brightness sums, without a GPU: EQUAL
to tests/qualityref.py, the numpy form written from the text in include/lmx.h; the reference is guarded by five defect models and by
closed forms; lmx.services.curation.visual_scores turns the sums into the two scores of clip-curation main.py:276-289; every refused
input is LMX_EINVAL with a message and writes nothing.  cv2 is not installed: parity with real OpenCV is UNPINNED."""
import numpy as np
import pytest

import qualityref as Q
from lmx import _lib
from lmx.services import curation

N = 3


def host_sums(frames, fill=0xA5):
    lib = _lib.load()
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    out = np.full((n, 4), fill, np.uint8).repeat(8, axis=1).view(np.int64)
    rc = lib.lmx_h_frame_quality(frames.ctypes.data, n, h, w, out.ctypes.data)
    assert rc == 0, lib.lmx_last_error().decode()
    return out


@pytest.fixture(scope="module")
def cases():
    """size -> (frames, reference sums), computed once"""
    out = {}
    for h, w in Q.SIZES:
        f = Q.random_frames(N, h, w, seed=1000 * h + w)
        out[(h, w)] = (f, Q.sums(f))
    return out


@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_function_equals_the_reference(cases, size):
    frames, want = cases[size]
    got = host_sums(frames)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(host_sums(frames, fill=0x00), want)  # whatever out held


@pytest.mark.parametrize("defect", Q.DEFECTS)
def test_each_defect_model_differs_on_those_inputs(cases, defect):
    """guards the reference and the fixtures: swapped coefficient order, the 14-bit coefficients, a truncating descale, an
    edge-replicating border and an edge-repeating reflection are each told from the right form — by the set of inputs as a whole and by
    each of the two larger sizes alone (a 2 x 2 frame has too few pixels for the two coefficient sets to have to disagree)"""
    differs = {size: not np.array_equal(Q.sums(frames, defect), want) for size, (frames, want) in cases.items()}
    assert any(differs.values()), defect
    assert differs[(17, 33)] and differs[(33, 1027)], (defect, differs)
    if defect in ("replicate", "symmetric"):  # a border model shows at every size
        assert all(differs.values()), (defect, differs)


def test_constant_frames():
    for h, w in ((2, 2), (5, 7), (33, 70)):
        n = h * w
        assert np.array_equal(host_sums(np.zeros((1, h, w, 3), np.uint8)), [[0, 0, 0, n]])
        assert np.array_equal(host_sums(np.full((1, h, w, 3), 255, np.uint8)), [[255 * n, 0, 0, n]])  # the coefficients add up to 2^15
        assert np.array_equal(Q.sums(np.full((1, h, w, 3), 255, np.uint8)), [[255 * n, 0, 0, n]])


@pytest.mark.parametrize("first", [0, 255])
def test_checkerboard_closed_form(first):
    for h, w in ((2, 2), (3, 3), (5, 7), (34, 70)):
        board = Q.checkerboard(h, w, first)
        want = Q.checkerboard_sums(h, w, first)
        n_first = (h * w + 1) // 2
        n_black = n_first if first == 0 else h * w - n_first
        assert want[2] == 1040400 * h * w and want[1] == 1020 * (n_black - (h * w - n_black))
        assert np.array_equal(host_sums(board)[0], want), (h, w)
        assert np.array_equal(Q.sums(board)[0], want), (h, w)


def test_visual_scores_against_numpy(cases):
    """brightness bit-equal to 1 - |np.mean(gray) - 128| / 128 on the u8 gray image; blur equal to min(1, np.var(lap as float64) / 500)
    to 1e-12 relative: numpy's pairwise sum over at most 2^21 terms carries an error bound near 21 * 2^-53 = 2.3e-15 per sum, and the
    margin covers its two-pass mean.  Random frames saturate the blur score, so the variance itself is compared as well, and smooth
    frames keep the score below 1."""
    ramp = np.add.outer(np.arange(40), np.arange(64) * 2).astype(np.uint8)
    smooth = np.repeat(ramp[None, :, :, None], 3, axis=3)
    smooth[0, 10:20, 10:30, 1] += 9
    for frames in [c[0] for c in cases.values()] + [smooth, Q.checkerboard(6, 9)]:
        stats = Q.sums(frames)
        blur, bright = curation.visual_scores(stats)
        assert blur.dtype == bright.dtype == np.float64
        for i in range(frames.shape[0]):
            g8 = Q.gray(frames[i:i + 1])[0].astype(np.uint8)
            lap = Q.laplacian(Q.gray(frames[i:i + 1]))[0].astype(np.float64)
            assert bright[i] == max(0.0, 1.0 - abs(np.mean(g8) - 128) / 128)
            want = min(1.0, lap.var() / 500.0)
            assert abs(blur[i] - want) <= 1e-12 * want
            s0, s1, s2, n = (int(v) for v in stats[i])
            assert abs((n * s2 - s1 * s1) / (n * n) - lap.var()) <= 1e-12 * lap.var()
    assert 0.0 < curation.visual_scores(Q.sums(smooth))[0][0] < 1.0


def test_visual_scores_beyond_int64_products():
    """N * S2 passes 2^63 for a 4096 x 4096 checkerboard's sums: Python integers carry it, the variance is 1040400 - (1020 / N)^2-ish"""
    n = 4096 * 4096
    stats = np.array([[255 * n // 2, 0, 1040400 * n, n]], np.int64)
    assert n * 1040400 * n > 2 ** 63
    blur, bright = curation.visual_scores(stats)
    assert blur[0] == 1.0 and bright[0] == 1.0 - abs(127.5 - 128) / 128


REFUSALS = [
    ("h_below_2", dict(h=1), "2 or more"),
    ("w_below_2", dict(w=1), "2 or more"),
    ("h_zero", dict(h=0), "2 or more"),
    ("h_above_32768", dict(h=32769), "above 32768"),
    ("w_above_32768", dict(w=32769), "above 32768"),
    ("n_negative", dict(n=-1), "n = -1"),
    ("null_bgr", dict(bgr=None), "null pointer (bgr)"),
    ("null_out", dict(out=None), "null pointer (out)"),
]


@pytest.mark.parametrize("entry", ["lmx_h_frame_quality", "lmx_k_frame_quality"])
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refused_inputs(case, entry):
    """LMX_EINVAL with a message; the checks run before anything is read, written or launched, so the kernel's entry point refuses on a
    host without a GPU too (its pointers are never followed)"""
    _, kw, text = case
    lib = _lib.load()
    frames = Q.random_frames(2, 5, 7)
    out = np.full((2, 4), 0xA5, np.uint8).repeat(8, axis=1).view(np.int64)
    guard = out.copy()
    args = (kw.get("bgr", frames.ctypes.data), kw.get("n", 2), kw.get("h", 5), kw.get("w", 7), kw["out"] if "out" in kw else out.ctypes.data)
    args += (None, None) if entry.startswith("lmx_k_") else ()
    assert getattr(lib, entry)(*args) == -1, case[0]
    msg = lib.lmx_last_error().decode()
    assert msg and entry in msg and text in msg, msg
    assert np.array_equal(out, guard), "a refused call wrote"


def test_zero_frames_touch_nothing():
    lib = _lib.load()
    out = np.full((1, 4), 0xA5, np.uint8).repeat(8, axis=1).view(np.int64)
    guard = out.copy()
    assert lib.lmx_h_frame_quality(None, 0, 5, 7, out.ctypes.data) == 0
    assert lib.lmx_k_frame_quality(None, 0, 5, 7, out.ctypes.data, None, None) == 0  # n = 0 launches nothing: no GPU needed
    assert lib.lmx_frame_quality_workspace_bytes(0, 5, 7) >= 0 and lib.lmx_frame_quality_workspace_bytes(150, 1080, 1920) >= 0
    assert np.array_equal(out, guard)
