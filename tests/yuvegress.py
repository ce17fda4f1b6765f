"""The case matrix and the runners that tests/test_yuv_egress_host.py (lmx_h_*, numpy memory) and tests/test_gpu_yuv_egress.py (lmx_k_*,
device memory) share, so that the GPU runs exactly what the host runs.  A runner lays its inputs and outputs into byte buffers of an
`arena` at a chosen pitch, frame stride and base offset, calls the entry point through ctypes, and compares the WHOLE output buffers
with buffers built from the numpy reference (tests/yuvoutref.py): the bytes of the planes and the untouched guard bytes around and
between them in one comparison."""
import ctypes as C

import numpy as np

import yuvoutref
import yuvref
from lmx import _lib

LAYOUTS = {"nv12": 0, "i420": 1}
MATRICES = {"bt601": 0, "bt709": 1}
SIZES = [(2, 2), (2, 18), (6, 34), (4, 50)]  # h x w of lmx_*_bgr_to_yuv420: below a block, a block and a tail of 2, two blocks + 2, three + 2
PITCH_EXTRA = (0, 1, 13)  # pitch = row + extra
OFFSETS = (0, 1)  # base = a 16-byte boundary + offset
FRAME = (18, 70)  # h x w of the source frame of the windows
# (x, y, w, h) on FRAME: all four parities of (x, y); odd and even w and h; w of 1, 15, 16, 17; windows on the right and bottom edges; the frame
WINDOWS = [(0, 0, 70, 18), (1, 0, 16, 4), (0, 1, 15, 3), (1, 1, 17, 5), (2, 2, 1, 1), (3, 5, 1, 2), (16, 0, 16, 2), (15, 3, 17, 15), (53, 7, 17, 11),
           (69, 17, 1, 1), (5, 4, 60, 9), (32, 6, 38, 12)]
GUARD = 64
FILL = 0xA5


class HostArena:
    """byte buffers in host memory, 16-byte aligned"""
    stream = ()  # lmx_h_ entry points take no stream

    def put(self, data):
        raw = np.empty(data.size + 16, np.uint8)
        start = (-raw.ctypes.data) % 16
        buf = raw[start:start + data.size]
        buf[:] = data
        return buf

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return np.array(buf)


class DeviceArena:
    """byte buffers in device memory (torch allocations are 256-byte aligned)"""
    stream = (None,)  # the null stream; get() synchronises

    def __init__(self, dev):
        import torch

        self.torch, self.dev = torch, dev

    def put(self, data):
        return self.torch.from_numpy(np.ascontiguousarray(data)).to(self.dev)

    def ptr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        self.torch.cuda.synchronize(self.dev)
        return buf.cpu().numpy()


def lay(planes, pitch, stride, offset, fill):
    """planes uint8 [n, rows, row] -> (bytes of a buffer, start): the planes at row pitch `pitch` and frame stride `stride` from byte
    GUARD + offset on, `fill` everywhere else (GUARD is a multiple of 16: the base's alignment is offset % 16)"""
    n, rows, row = planes.shape
    assert pitch >= row and (n <= 1 or stride >= rows * pitch)
    start = GUARD + offset
    buf = np.full(start + max(n - 1, 0) * stride + rows * pitch + GUARD, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[start:], (n, rows, row), (stride, pitch, 1))
    view[...] = planes
    return buf, start


def bgr_to_yuv420(fn, arena, frames, layout, matrix, src_extra=0, src_offset=0, out_extra=0, out_offset=0, extra_stride=0):
    """run lmx_h_ / lmx_k_bgr_to_yuv420 (`fn`) on frames uint8 [n,h,w,3] laid out as asked; asserts the output buffers byte for byte"""
    n, h, w, _ = frames.shape
    want = yuvoutref.from_bgr(frames, matrix)
    want = [want[0], yuvref.interleave(want[1], want[2])] if layout == "nv12" else list(want)
    sp = 3 * w + src_extra
    src, s0 = lay(frames.reshape(n, h, 3 * w), sp, h * sp + extra_stride, src_offset, 0x5A)
    dsrc = arena.put(src)
    outs, bufs, ptrs, geo = [], [], [], []
    for p in want:
        pitch = p.shape[2] + out_extra
        stride = p.shape[1] * pitch + extra_stride
        exp, start = lay(p, pitch, stride, out_offset, FILL)
        outs.append(exp)
        b = arena.put(np.full(exp.size, FILL, np.uint8))
        bufs.append(b)
        ptrs.append(arena.ptr(b) + start)
        geo.append((pitch, stride))
    assert all(g == geo[1] for g in geo[1:])
    o = _lib.YuvOut(ptrs[0], ptrs[1], ptrs[2] if layout == "i420" else None, geo[0][0], geo[1][0], geo[0][1], geo[1][1], LAYOUTS[layout], MATRICES[matrix])
    lib = _lib.load()
    rc = fn(arena.ptr(dsrc) + s0, sp, h * sp + extra_stride, n, h, w, C.byref(o), *arena.stream)
    assert rc == 0, lib.lmx_last_error().decode()
    for name, b, exp in zip("yuv", bufs, outs):
        got = arena.get(b)
        assert np.array_equal(got, exp), (name, layout, matrix, (h, w), src_extra, src_offset, out_extra, out_offset, int((got != exp).sum()))
    assert np.array_equal(arena.get(dsrc), src), "the source was written"


def source_planes(arena, y, u, v, layout, matrix, extra=0, offset=0, extra_stride=0):
    """(lmx_yuv_frames_t, the buffers that keep it alive) of planes y [n,h,w], u / v [n,h/2,w/2] laid out as asked"""
    planes = [y, yuvref.interleave(u, v)] if layout == "nv12" else [y, u, v]
    bufs, ptrs, geo = [], [], []
    for p in planes:
        pitch = p.shape[2] + extra
        stride = p.shape[1] * pitch + extra_stride
        b, start = lay(p, pitch, stride, offset, 0x5A)
        d = arena.put(b)
        bufs.append(d)
        ptrs.append(arena.ptr(d) + start)
        geo.append((pitch, stride))
    f = _lib.YuvFrames(ptrs[0], ptrs[1], ptrs[2] if layout == "i420" else None, geo[0][0], geo[1][0], geo[0][1], geo[1][1], LAYOUTS[layout], MATRICES[matrix])
    return f, bufs


def window(fn, arena, f, n, h, w, roi, want, out_offset=0):
    """run lmx_h_ / lmx_k_yuv420_to_bgr_roi (`fn`) on the descriptor f; `want` uint8 [n, roi h, roi w, 3]; asserts the whole output buffer"""
    rx, ry, rw, rh = roi
    exp, start = lay(want.reshape(1, 1, -1), want.size, want.size, out_offset, FILL)
    b = arena.put(np.full(exp.size, FILL, np.uint8))
    rect = _lib.Rect(rx, ry, rw, rh)
    rc = fn(C.byref(f), n, h, w, C.byref(rect), arena.ptr(b) + start, *arena.stream)
    assert rc == 0, _lib.load().lmx_last_error().decode()
    got = arena.get(b)
    assert np.array_equal(got, exp), (roi, out_offset, int((got != exp).sum()))
