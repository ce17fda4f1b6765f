"""lmx_h_bgr_to_yuv420 and lmx_h_yuv420_to_bgr_roi (csrc/host_yuv.cpp), the plain C++ restatements of the two kernels behind
lmx_k_yuv420_to_bgr, without a GPU: EQUAL (np.array_equal) to tests/yuvoutref.py, the numpy int64 form written from the texts in
include/lmx.h, over tests/yuvegress.py's matrix of sizes, pitches, bases and windows with the guard bytes around every output
untouched; the reference itself is guarded by five defect models, by known answers and by its coefficients; every refused input is
LMX_EINVAL with a message that names the argument.  Neither cv2 nor swscale is installed: the arithmetic is pinned by the text,
parity with them is UNPINNED."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import yuvegress as E
import yuvoutref
import yuvref
from lmx import _lib

ARENA = E.HostArena()


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bgr_to_yuv420_equals_the_reference(size, layout, matrix):
    """n = 2 with frame strides above a frame; source and output pitches of row + 0 / 1 / 13; bases at + 0 and + 1"""
    h, w = size
    frames = yuvoutref.random_bgr(h, w, 2, seed=100 * h + w)
    fn = _lib.load().lmx_h_bgr_to_yuv420
    for extra in E.PITCH_EXTRA:
        for offset in E.OFFSETS:
            E.bgr_to_yuv420(fn, ARENA, frames, layout, matrix, src_extra=extra, src_offset=offset, out_extra=extra, out_offset=offset, extra_stride=37)
    E.bgr_to_yuv420(fn, ARENA, frames, layout, matrix, src_extra=13, src_offset=0, out_extra=0, out_offset=1, extra_stride=5)


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_windows_equal_the_reference(layout, matrix):
    """every window of the matrix on an 18 x 70 frame, n = 2, under source pitches of row + 0 / 1 / 13 and bases at + 0 / + 1"""
    h, w = E.FRAME
    y, u, v = yuvref.random_frame(h, w, 2, seed=3)
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
    fn = _lib.load().lmx_h_yuv420_to_bgr_roi
    for extra in E.PITCH_EXTRA:
        for offset in E.OFFSETS:
            f, keep = E.source_planes(ARENA, y, u, v, layout, matrix, extra, offset, extra_stride=37)
            for roi in E.WINDOWS:
                E.window(fn, ARENA, f, 2, h, w, roi, yuvoutref.window(y, c, h, w, roi, layout, matrix, v=vv), out_offset=offset)
            del keep


@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_the_full_frame_window_is_the_whole_frame_conversion(layout):
    h, w = E.FRAME
    y, u, v = yuvref.random_frame(h, w, 2, seed=4)
    lib = _lib.load()
    f, keep = E.source_planes(ARENA, y, u, v, layout, "bt709", 1, 1, extra_stride=3)
    whole = np.full((2, h, w, 3), 1, np.uint8)
    assert lib.lmx_h_yuv420_to_bgr(C.byref(f), 2, h, w, whole.ctypes.data) == 0, lib.lmx_last_error().decode()
    E.window(lib.lmx_h_yuv420_to_bgr_roi, ARENA, f, 2, h, w, (0, 0, w, h), whole)


def test_window_cases_are_what_the_matrix_says():
    h, w = E.FRAME
    assert {(x & 1, y & 1) for x, y, _, _ in E.WINDOWS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {1, 15, 16, 17} <= {rw for _, _, rw, _ in E.WINDOWS}
    assert {rw & 1 for _, _, rw, _ in E.WINDOWS} == {rh & 1 for _, _, _, rh in E.WINDOWS} == {0, 1}
    assert any(x + rw == w and (x, rw) != (0, w) for x, _, rw, _ in E.WINDOWS) and any(y + rh == h and (y, rh) != (0, h) for _, y, _, rh in E.WINDOWS)
    assert (0, 0, w, h) in E.WINDOWS and all(x >= 0 and y >= 0 and x + rw <= w and y + rh <= h for x, y, rw, rh in E.WINDOWS)


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
def fixture_frames():
    """a random 6 x 34 frame and a 2 x 4 frame whose 2 x 2 blocks are far from flat (the top-left pixel is no mean of its block)"""
    sharp = np.array([[[[255, 0, 0], [0, 0, 0], [10, 200, 30], [250, 3, 77]], [[0, 0, 0], [0, 0, 1], [90, 91, 92], [1, 254, 128]]]], np.uint8)
    return [yuvoutref.random_bgr(6, 34, 1, seed=8), sharp]


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("defect", yuvoutref.DEFECTS)
def test_each_defect_model_changes_a_fixture_byte(defect, matrix):
    """chroma from the top-left pixel only, converting a rounded mean instead of the sum, a truncating shift (no 2^21), R and B swapped,
    full-range coefficients: each is told apart from the definition by at least one byte of the fixtures"""
    differ = 0
    for frames in fixture_frames():
        right, wrong = yuvoutref.from_bgr(frames, matrix), yuvoutref.from_bgr(frames, matrix, defect=defect)
        differ += sum(int((a != b).sum()) for a, b in zip(right, wrong))
    assert differ >= 1, defect


def host_planes(frames, layout, matrix):
    """lmx_h_bgr_to_yuv420 on tight frames -> (y, u, v)"""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    y = np.zeros((n, h, w), np.uint8)
    c = np.zeros((n, h // 2, w if layout == "nv12" else w // 2), np.uint8)
    v = np.zeros_like(c) if layout == "i420" else None
    o = _lib.YuvOut(y.ctypes.data, c.ctypes.data, v.ctypes.data if v is not None else None, w, c.shape[2], h * w, c[0].size, E.LAYOUTS[layout], E.MATRICES[matrix])
    assert lib.lmx_h_bgr_to_yuv420(frames.ctypes.data, 3 * w, 3 * w * h, n, h, w, C.byref(o)) == 0, lib.lmx_last_error().decode()
    return (y, c[..., 0::2], c[..., 1::2]) if layout == "nv12" else (y, c, v)


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_known_answers(layout, matrix):
    """grey gives U = V = 128; black Y = 16 and white Y = 235; pure blue, green and red reach the chroma extremes 16 and 240"""
    def solid(b, g, r):
        return np.broadcast_to(np.array([b, g, r], np.uint8), (1, 2, 2, 3))

    for make in (lambda f: yuvoutref.from_bgr(f, matrix), lambda f: host_planes(f, layout, matrix)):
        for grey in (0, 1, 77, 128, 254, 255):
            y, u, v = make(solid(grey, grey, grey))
            assert (u == 128).all() and (v == 128).all(), grey
        assert (make(solid(0, 0, 0))[0] == 16).all() and (make(solid(255, 255, 255))[0] == 235).all()
        blue, green, red = (make(solid(*p)) for p in ((255, 0, 0), (0, 255, 0), (0, 0, 255)))
        assert (blue[1] == 240).all() and (red[2] == 240).all()  # U of pure blue, V of pure red: the upper extreme
        assert max(int(p[k].max()) for p in (blue, green, red) for k in (1, 2)) == 240 and (green[1] < 128).all() and (green[2] < 128).all()
        # the lower extreme is reached by their complements: yellow's U and cyan's V
        assert (make(solid(0, 255, 255))[1] == 16).all() and (make(solid(255, 255, 0))[2] == 16).all()


def test_reference_coefficients():
    table = {"bt601": ((102760, 528482, 269484), (460325, -305136, -155189), (-74449, -385876, 460325)),
             "bt709": ((65012, 643826, 191889), (460325, -354419, -105906), (-41943, -418382, 460325))}
    assert yuvoutref.COEF == table
    for m, (ky, ku, kv) in table.items():
        assert sum(ku) == 0 and sum(kv) == 0, m  # a grey block has no chroma
        assert ((255 * sum(ky) + (1 << 19)) >> 20) + 16 == 235, m
        assert 255 * sum(ky) + (1 << 19) < 2 ** 31
        for k in (ku, kv):  # the largest sum of products of either sign, on 2 x 2 sums of 0 .. 1020
            assert 1020 * sum(c for c in k if c > 0) + (1 << 21) < 2 ** 31 and -1020 * sum(c for c in k if c < 0) < 2 ** 31
        assert all(abs(c) < 2 ** 23 for k in (ky, ku, kv) for c in k)  # the 24-bit multiply serves


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
OUT_REFUSALS = [
    ("odd_h", dict(h=5), "even sizes"),
    ("odd_w", dict(w=33), "even sizes"),
    ("w_below_2", dict(w=0), "even sizes"),
    ("pitch_bgr_below_row", dict(pitch_bgr=101), "pitch_bgr"),
    ("pitch_y_below_row", dict(pitch_y=33), "pitch_y"),
    ("pitch_c_below_row_nv12", dict(pitch_c=33), "pitch_c"),
    ("pitch_c_below_row_i420", dict(layout="i420", pitch_c=16), "pitch_c"),
    ("layout_outside", dict(layout=2), "layout 2"),
    ("matrix_outside", dict(matrix=2), "matrix 2"),
    ("nv12_with_v", dict(with_v=True), "v must be NULL"),
    ("i420_without_v", dict(layout="i420", with_v=False), "needs the v plane"),
    ("null_descriptor", dict(no_out=True), "out_host"),
]


@pytest.mark.parametrize("entry", ["lmx_h_bgr_to_yuv420", "lmx_k_bgr_to_yuv420"])
@pytest.mark.parametrize("case", OUT_REFUSALS, ids=[c[0] for c in OUT_REFUSALS])
def test_bgr_to_yuv420_refusals(case, entry):
    """LMX_EINVAL with a message; the checks run before anything is read, written or launched, so the kernel's entry point refuses on a
    host without a GPU too (its pointers are never followed)"""
    _, kw, text = case
    lib = _lib.load()
    layout = kw.get("layout", "nv12")
    h, w = kw.get("h", 6), kw.get("w", 34)
    frames = yuvoutref.random_bgr(6, 34)
    y, c, v = (np.full((1, 6, 34), E.FILL, np.uint8) for _ in range(3))
    with_v = kw.get("with_v", layout == "i420")
    o = _lib.YuvOut(y.ctypes.data, c.ctypes.data, v.ctypes.data if with_v else None, kw.get("pitch_y", 34), kw.get("pitch_c", 34), 6 * 34, 6 * 34,
                    E.LAYOUTS.get(layout, layout), kw.get("matrix", 0))
    args = (frames.ctypes.data, kw.get("pitch_bgr", 102), 6 * 102, 1, h, w, None if kw.get("no_out") else C.byref(o))
    assert getattr(lib, entry)(*args + ((None,) if entry.startswith("lmx_k_") else ())) == -1, case[0]
    msg = lib.lmx_last_error().decode()
    assert msg and entry in msg and text in msg, msg
    assert all((p == E.FILL).all() for p in (y, c, v)), "a refused call wrote"


ROI_REFUSALS = [
    ("empty_w", dict(roi=(0, 0, 0, 4)), "roi is empty"),
    ("empty_h", dict(roi=(0, 0, 4, 0)), "roi is empty"),
    ("negative_w", dict(roi=(4, 4, -2, 4)), "roi is empty"),
    ("x_negative", dict(roi=(-1, 0, 4, 4)), "roi (x = -1"),
    ("y_negative", dict(roi=(0, -1, 4, 4)), "roi (x = 0, y = -1"),
    ("right_of_the_frame", dict(roi=(67, 0, 4, 4)), "is outside the 18 x 70 frame"),
    ("below_the_frame", dict(roi=(0, 15, 4, 4)), "is outside the 18 x 70 frame"),
    ("overflowing_sum", dict(roi=(2 ** 31 - 1, 0, 2 ** 31 - 1, 4)), "is outside"),
    ("null_window", dict(roi=None), "roi_host"),
    ("odd_frame_h", dict(h=17), "even sizes"),
    ("pitch_y_below_row", dict(pitch_y=69), "pitch_y"),
    ("layout_outside", dict(layout=2), "layout 2"),
    ("nv12_with_v", dict(with_v=True), "v must be NULL"),
]


@pytest.mark.parametrize("entry", ["lmx_h_yuv420_to_bgr_roi", "lmx_k_yuv420_to_bgr_roi"])
@pytest.mark.parametrize("case", ROI_REFUSALS, ids=[c[0] for c in ROI_REFUSALS])
def test_window_refusals(case, entry):
    """everything lmx_yuv_check refuses, a window outside the frame and an empty window"""
    _, kw, text = case
    lib = _lib.load()
    y, u, v = yuvref.random_frame()
    c = yuvref.interleave(u, v)
    f = _lib.YuvFrames(y.ctypes.data, c.ctypes.data, v.ctypes.data if kw.get("with_v") else None, kw.get("pitch_y", 70), 70, 18 * 70, 9 * 70,
                       kw.get("layout", 0), 0)
    roi = kw.get("roi", (0, 0, 4, 4))
    rect = _lib.Rect(*roi) if roi is not None else None
    out = np.full((1, 18, 70, 3), E.FILL, np.uint8)
    args = (C.byref(f), 1, kw.get("h", 18), 70, C.byref(rect) if rect is not None else None, out.ctypes.data)
    assert getattr(lib, entry)(*args + ((None,) if entry.startswith("lmx_k_") else ())) == -1, case[0]
    msg = lib.lmx_last_error().decode()
    assert msg and entry in msg and text in msg, msg
    assert (out == E.FILL).all(), "a refused call wrote"


def test_zero_frames_touch_nothing():
    lib = _lib.load()
    y, u, v = yuvref.random_frame()
    c = yuvref.interleave(u, v)
    f = _lib.YuvFrames(y.ctypes.data, c.ctypes.data, None, 70, 70, 18 * 70, 9 * 70, 0, 0)
    rect = _lib.Rect(1, 1, 5, 5)
    out = np.full((1, 18, 70, 3), E.FILL, np.uint8)
    assert lib.lmx_h_yuv420_to_bgr_roi(C.byref(f), 0, 18, 70, C.byref(rect), out.ctypes.data) == 0
    assert lib.lmx_k_yuv420_to_bgr_roi(C.byref(f), 0, 18, 70, C.byref(rect), out.ctypes.data, None) == 0  # n = 0 launches nothing: no GPU needed
    o = _lib.YuvOut(out.ctypes.data, out.ctypes.data, None, 70, 70, 18 * 70, 9 * 70, 0, 0)
    src = yuvoutref.random_bgr(18, 70)
    assert lib.lmx_h_bgr_to_yuv420(src.ctypes.data, 210, 18 * 210, 0, 18, 70, C.byref(o)) == 0
    assert lib.lmx_k_bgr_to_yuv420(src.ctypes.data, 210, 18 * 210, 0, 18, 70, C.byref(o), None) == 0
    assert (out == E.FILL).all()


def test_host_functions_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/yuv_egress_check_main.cpp + csrc/host_yuv.cpp built with -fsanitize=address,undefined as a program of its own and run
    directly: every buffer is a heap block that ends with its last row's last byte and starts `offset` bytes into its allocation,
    pitches of row + 0 / 1 / 13, frame strides above a frame; the outputs equal the reference and the sanitizers stay silent"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "yuv_egress_check_main"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(root, "tests", "yuv_egress_check_main.cpp"), os.path.join(root, "vision-sam3-yolo-lameless_amd", "csrc", "host_yuv.cpp"),
                    "-o", str(exe)], check=True, timeout=300)

    def tight(planes, pitch, stride):
        """the bytes of an allocation that ends with the last row's last byte"""
        n, rows, row = planes.shape
        a = np.full((n - 1) * stride + (rows - 1) * pitch + row, 0x5A, np.uint8)
        np.lib.stride_tricks.as_strided(a, (n, rows, row), (stride, pitch, 1))[...] = planes
        return a.tobytes()

    def untangle(blob, n, rows, row, pitch, stride):
        a = np.frombuffer(blob, np.uint8)
        assert a.size == (n - 1) * stride + (rows - 1) * pitch + row
        return np.array(np.lib.stride_tricks.as_strided(a, (n, rows, row), (stride, pitch, 1)))

    n = 2
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    for (h, w), extra, offset in (((2, 2), 0, 0), ((2, 18), 1, 1), ((6, 34), 13, 1), ((4, 50), 13, 0), ((6, 34), 0, 3)):
        for layout in E.LAYOUTS:
            # mode 0: BGR -> YUV
            frames = yuvoutref.random_bgr(h, w, n, seed=h + w + extra)
            sp = 3 * w + extra
            cw = w if layout == "nv12" else w // 2
            py, pc = w + extra, cw + extra
            sy, sc = h * py + 5, (h // 2) * pc + 3
            hd = np.array([0, n, h, w, E.LAYOUTS[layout], 1, offset, sp, h * sp + 7, py, pc, sy, sc, 0, 0, 0, 0], np.int64)
            src.write_bytes(hd.tobytes() + tight(frames.reshape(n, h, 3 * w), sp, h * sp + 7))
            run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=60)
            assert run.returncode == 0 and run.stderr == "", (h, w, extra, offset, layout, run.returncode, run.stderr[-2000:])
            blob = dst.read_bytes()
            wy, wu, wv = yuvoutref.from_bgr(frames, "bt709")
            ny = (n - 1) * sy + (h - 1) * py + w
            nc = (n - 1) * sc + (h // 2 - 1) * pc + cw
            assert np.array_equal(untangle(blob[:ny], n, h, w, py, sy), wy)
            if layout == "nv12":
                assert np.array_equal(untangle(blob[ny:], n, h // 2, cw, pc, sc), yuvref.interleave(wu, wv))
            else:
                assert np.array_equal(untangle(blob[ny:ny + nc], n, h // 2, cw, pc, sc), wu) and np.array_equal(untangle(blob[ny + nc:], n, h // 2, cw, pc, sc), wv)
    h, w = E.FRAME
    for extra, offset in ((0, 0), (1, 1), (13, 3)):
        for layout in E.LAYOUTS:
            # mode 1: the window
            y, u, v = yuvref.random_frame(h, w, n, seed=extra)
            c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
            cw = w if layout == "nv12" else w // 2
            py, pc = w + extra, cw + extra
            sy, sc = h * py + 5, (h // 2) * pc + 3
            for roi in E.WINDOWS:
                hd = np.array([1, n, h, w, E.LAYOUTS[layout], 0, offset, 0, 0, py, pc, sy, sc, *roi], np.int64)
                blob = hd.tobytes() + tight(y, py, sy) + tight(c, pc, sc) + (tight(vv, pc, sc) if vv is not None else b"")
                src.write_bytes(blob)
                run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=60)
                assert run.returncode == 0 and run.stderr == "", (roi, extra, offset, layout, run.returncode, run.stderr[-2000:])
                got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(n, roi[3], roi[2], 3)
                assert np.array_equal(got, yuvoutref.window(y, c, h, w, roi, layout, "bt601", v=vv)), (roi, extra, offset, layout)
