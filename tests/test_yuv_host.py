"""lmx_h_yuv420_to_bgr (csrc/host_yuv.cpp), the plain C++ restatement of the YUV 4:2:0 -> BGR kernel, without a GPU: EQUAL
(np.array_equal) to tests/yuvref.py, the numpy int64 form written from the text in include/lmx.h, for both layouts and both matrices;
the reference itself is guarded by five defect models and by its coefficients; every refused input is LMX_EINVAL with a message.
cv2 is not installed: the arithmetic is pinned by the text, parity with real OpenCV is UNPINNED."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import yuvref
from lmx import _lib

LAYOUTS = {"nv12": 0, "i420": 1}
MATRICES = {"bt601": 0, "bt709": 1}


def frames_desc(y, u, v, layout, matrix, pitch_y=None, pitch_c=None):
    """lmx_yuv_frames_t over C-contiguous numpy planes [n, rows, pitch]; the arrays must outlive the call"""
    return _lib.YuvFrames(y.ctypes.data, u.ctypes.data, v.ctypes.data if v is not None else None, pitch_y or y.strides[1], pitch_c or u.strides[1],
                          y.strides[0], u.strides[0], LAYOUTS.get(layout, layout), MATRICES.get(matrix, matrix))


def host_bgr(y, u, v, h, w, layout, matrix):
    """lmx_h_yuv420_to_bgr on planes y [n,h,w], u / v [n,h/2,w/2] (interleaved here for nv12)"""
    lib = _lib.load()
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (np.ascontiguousarray(u), np.ascontiguousarray(v))
    y = np.ascontiguousarray(y)
    out = np.full((y.shape[0], h, w, 3), 0xA5, np.uint8)
    f = frames_desc(y, c, vv, layout, matrix)
    rc = lib.lmx_h_yuv420_to_bgr(C.byref(f), y.shape[0], h, w, out.ctypes.data)
    assert rc == 0, lib.lmx_last_error().decode()
    return out


def ref_bgr(y, u, v, h, w, layout, matrix, defect=None):
    if layout == "nv12":
        return yuvref.to_bgr(y, yuvref.interleave(u, v), h, w, "nv12", matrix, defect=defect)
    return yuvref.to_bgr(y, u, h, w, "i420", matrix, v=v, defect=defect)


@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("frame", ["random_18x70", "sweep_162x512"])
def test_host_function_equals_the_reference(frame, layout, matrix):
    y, u, v = yuvref.random_frame() if frame == "random_18x70" else yuvref.sweep_frame()
    h, w = y.shape[1:]
    want = ref_bgr(y, u, v, h, w, layout, matrix)
    got = host_bgr(y, u, v, h, w, layout, matrix)
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    if frame == "sweep_162x512":  # saturation at both ends, in every channel
        assert all(want[..., ch].min() == 0 and want[..., ch].max() == 255 for ch in range(3))


def test_sweep_frame_is_what_it_says():
    y, u, v = yuvref.sweep_frame()
    assert y.shape == (1, 162, 512) and u.shape == v.shape == (1, 81, 256)
    vals = {0, 1, 16, 127, 128, 129, 240, 254, 255}
    assert {(int(a), int(b)) for a, b in zip(u[0, :, 0], v[0, :, 0])} == {(a, b) for a in vals for b in vals}
    assert (u == u[:, :, :1]).all() and (v == v[:, :, :1]).all()
    assert set(y[0, 0].tolist()) == set(y[0, 1].tolist()) == set(range(256))  # every Y in both rows of every chroma block-row
    assert np.array_equal(y[0, 0], np.arange(512) >> 1) and np.array_equal(y[0, 1], 255 - (np.arange(512) >> 1))


@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("defect", yuvref.DEFECTS)
def test_each_defect_model_changes_the_random_frame(defect, layout, matrix):
    """guards the reference: a formula without the rounding term, without the clamp of Y - 16, with U and V swapped, or with the
    chroma row / column not halved is told apart from the right one by at least one byte"""
    y, u, v = yuvref.random_frame()
    right = ref_bgr(y, u, v, 18, 70, layout, matrix)
    wrong = ref_bgr(y, u, v, 18, 70, layout, matrix, defect=defect)
    assert int((right != wrong).sum()) >= 1, defect


def test_the_two_matrices_differ_on_the_random_frame():
    y, u, v = yuvref.random_frame()
    assert int((ref_bgr(y, u, v, 18, 70, "i420", "bt601") != ref_bgr(y, u, v, 18, 70, "i420", "bt709")).sum()) >= 1


def test_reference_coefficients():
    table = {"bt601": (1220542, 2116026, -409993, -852492, 1673527), "bt709": (1220542, 2214593, -223347, -558891, 1880097)}
    consts = {"bt601": (1.164, 2.018, -0.391, -0.813, 1.596), "bt709": (1.164, 2.112, -0.213, -0.533, 1.793)}
    for m in table:
        assert yuvref.COEF[m] == table[m] == tuple(int(round(c * 2 ** 20)) for c in consts[m]), m
    # nothing overflows 32 bits: the largest intermediate over every byte triple
    for cy, cub, cug, cvg, cvr in table.values():
        top = (255 - 16) * cy + (1 << 19)
        assert top + 128 * max(abs(cub), abs(cvr), abs(cug) + abs(cvg)) < 2 ** 31


REFUSALS = [
    ("odd_h", dict(h=17), "even sizes"),
    ("odd_w", dict(w=69), "even sizes"),
    ("h_below_2", dict(h=0), "even sizes"),
    ("w_below_2", dict(w=0), "even sizes"),
    ("pitch_y_below_row", dict(pitch_y=69), "pitch_y"),
    ("pitch_c_below_row_nv12", dict(pitch_c=69), "pitch_c"),
    ("pitch_c_below_row_i420", dict(layout="i420", pitch_c=34), "pitch_c"),
    ("layout_outside", dict(layout=2), "layout 2"),
    ("layout_negative", dict(layout=-1), "layout -1"),
    ("matrix_outside", dict(matrix=2), "matrix 2"),
    ("nv12_with_v", dict(with_v=True), "v must be NULL"),
    ("i420_without_v", dict(layout="i420", with_v=False), "needs the v plane"),
]


@pytest.mark.parametrize("entry", ["lmx_h_yuv420_to_bgr", "lmx_k_yuv420_to_bgr"])
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refused_inputs(case, entry):
    """LMX_EINVAL with a message; the checks run before anything is read or launched, so the kernel's entry point refuses on a host
    without a GPU too (its pointers are never followed)"""
    _, kw, text = case
    lib = _lib.load()
    layout = kw.get("layout", "nv12")
    h, w = kw.get("h", 18), kw.get("w", 70)
    y, u, v = yuvref.random_frame()
    c = yuvref.interleave(u, v) if layout != "i420" else u
    with_v = kw.get("with_v", layout == "i420")
    f = frames_desc(y, c, v if with_v else None, layout, kw.get("matrix", "bt601"), kw.get("pitch_y"), kw.get("pitch_c"))
    out = np.full((1, 18, 70, 3), 0xA5, np.uint8)
    args = (C.byref(f), 1, h, w, out.ctypes.data) + ((None,) if entry.startswith("lmx_k_") else ())
    assert getattr(lib, entry)(*args) == -1, case[0]
    msg = lib.lmx_last_error().decode()
    assert msg and entry in msg and text in msg, msg
    assert (out == 0xA5).all(), "a refused call wrote"


def test_zero_frames_touch_nothing():
    lib = _lib.load()
    y, u, v = yuvref.random_frame()
    f = frames_desc(y, yuvref.interleave(u, v), None, "nv12", "bt601")
    out = np.full((1, 18, 70, 3), 0xA5, np.uint8)
    assert lib.lmx_h_yuv420_to_bgr(C.byref(f), 0, 18, 70, out.ctypes.data) == 0
    assert lib.lmx_k_yuv420_to_bgr(C.byref(f), 0, 18, 70, out.ctypes.data, None) == 0  # n = 0 launches nothing: no GPU needed
    assert (out == 0xA5).all()


def test_pitched_and_strided_planes_on_the_host():
    """pitches above the row and frame strides above a frame: the host function reads through the descriptor, not through a shape"""
    n, h, w = 3, 18, 70
    y, u, v = yuvref.random_frame(h, w, n, seed=1)
    for layout in LAYOUTS:
        cw = w if layout == "nv12" else w // 2
        yb = np.full((n, h + 3, w + 14), 7, np.uint8)
        cb = np.full((n, h // 2 + 2, cw + 5), 9, np.uint8)
        vb = np.full_like(cb, 11)
        yb[:, :h, :w] = y
        if layout == "nv12":
            cb[:, : h // 2, :cw] = yuvref.interleave(u, v)
        else:
            cb[:, : h // 2, :cw], vb[:, : h // 2, :cw] = u, v
        f = frames_desc(yb, cb, vb if layout == "i420" else None, layout, "bt709")
        out = np.zeros((n, h, w, 3), np.uint8)
        lib = _lib.load()
        assert lib.lmx_h_yuv420_to_bgr(C.byref(f), n, h, w, out.ctypes.data) == 0, lib.lmx_last_error().decode()
        assert np.array_equal(out, ref_bgr(y, u, v, h, w, layout, "bt709")), layout


def test_host_function_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/yuv_check_main.cpp + csrc/host_yuv.cpp built with -fsanitize=address,undefined as a program of its own and run directly: planes
    at offsets 0, 1, 2, 3 and 8 of heap blocks that end with the last row's last byte, pitches w, w + 1, w + 14 and the next multiple of
    256, frame strides above a frame; the output equals the reference and the sanitizers stay silent"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "yuv_check_main"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(root, "tests", "yuv_check_main.cpp"),
                    os.path.join(root, "vision-sam3-yolo-lameless_amd", "csrc", "host_yuv.cpp"), "-o", str(exe)], check=True, timeout=300)
    n, h = 3, 18
    for w, offset, extra in ((70, 0, 0), (70, 1, 1), (64, 2, 14), (70, 3, None), (64, 8, 1)):
        for layout in LAYOUTS:
            y, u, v = yuvref.random_frame(h, w, n, seed=w + offset)
            cw = w if layout == "nv12" else w // 2
            py, pc = (-(-w // 256) * 256, -(-cw // 256) * 256) if extra is None else (w + extra, cw + extra)
            sy, sc = py * h + 5, pc * (h // 2) + 3

            def alloc(planes, rows, row, pitch, stride):
                a = np.full(((n - 1) * stride + (rows - 1) * pitch + row,), 0x5A, np.uint8)
                for i in range(n):
                    for r in range(rows):
                        a[i * stride + r * pitch: i * stride + r * pitch + row] = planes[i, r]
                return a.tobytes()

            blob = np.array([n, h, w, LAYOUTS[layout], MATRICES["bt601"], offset, py, pc, sy, sc], np.int64).tobytes() + alloc(y, h, w, py, sy)
            if layout == "nv12":
                blob += alloc(yuvref.interleave(u, v), h // 2, cw, pc, sc)
            else:
                blob += alloc(u, h // 2, cw, pc, sc) + alloc(v, h // 2, cw, pc, sc)
            src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
            src.write_bytes(blob)
            run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=60)
            assert run.returncode == 0 and run.stderr == "", (w, offset, extra, layout, run.returncode, run.stderr[-2000:])
            got = np.frombuffer(dst.read_bytes(), np.uint8).reshape(n, h, w, 3)
            assert np.array_equal(got, ref_bgr(y, u, v, h, w, layout, "bt601")), (w, offset, extra, layout)
