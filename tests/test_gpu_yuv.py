"""lmx_k_yuv420_to_bgr (csrc/yuv.hip) on the GPU: EQUAL (torch.equal) to tests/yuvref.py, the numpy int64 form of the text in
include/lmx.h, and to lmx_h_yuv420_to_bgr, for both layouts and both matrices — on both sides of every vector width and of the seam
between a thread's whole 16-column block and the row's tail, at every plane and output alignment, under pitches and frame strides
above the row and the frame, and at the 1080p NV12 surface pitched to 2048 bytes the wide path was written for.  Every output sits
inside a guard buffer filled with 0xA5 first: the bytes outside [n][h][w][3] stay untouched and the result does not depend on the fill."""
import ctypes as C

import numpy as np
import pytest
import torch

import yuvref
from lmx import _lib
from lmx import kernels as K

pytestmark = pytest.mark.gpu
LAYOUTS = ("nv12", "i420")
MATRICES = ("bt601", "bt709")
GUARD = 64  # bytes in front of and behind the output


def placed(dev, planes, pitch, stride, offset):
    """planes uint8 numpy [n, rows, row] -> a device view [n, rows, row] with row pitch `pitch` and frame stride `stride` (bytes) that
    starts `offset` bytes into an allocation of its own; the bytes between rows and frames hold 0x5A"""
    n, rows, row = planes.shape
    assert pitch >= row and stride >= rows * pitch
    buf = torch.full((offset + n * stride,), 0x5A, dtype=torch.uint8, device=dev)
    view = torch.as_strided(buf, (n, rows, row), (stride, pitch, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(planes)))
    return view


def device_planes(dev, y, u, v, layout, pitch=None, extra_stride=0, offset=0):
    """(y, c, v) device views for K.yuv420_to_bgr; pitch: a function of the row length (None: tight)"""
    pitch = pitch or (lambda row: row)
    h = y.shape[1]
    c = yuvref.interleave(u, v) if layout == "nv12" else u
    py, pc = pitch(y.shape[2]), pitch(c.shape[2])
    dy = placed(dev, y, py, h * py + extra_stride, offset)
    dc = placed(dev, c, pc, (h // 2) * pc + extra_stride, offset)
    dv = placed(dev, v, pc, (h // 2) * pc + extra_stride, offset) if layout == "i420" else None
    return dy, dc, dv


def convert(dev, dy, dc, dv, n, h, w, layout, matrix, out_offset=0, fill=0xA5):
    """the converted frames, taken out of a guard buffer whose other bytes must still hold the fill"""
    nbytes = n * h * w * 3
    guard = torch.full((GUARD + out_offset + nbytes + GUARD,), fill, dtype=torch.uint8, device=dev)
    out = guard[GUARD + out_offset: GUARD + out_offset + nbytes].view(n, h, w, 3)
    assert out.data_ptr() % 16 == out_offset % 16
    got = K.yuv420_to_bgr(dy, dc, h, w, layout=layout, matrix=matrix, v=dv, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize(dev)
    assert bool((guard[: GUARD + out_offset] == fill).all()) and bool((guard[GUARD + out_offset + nbytes:] == fill).all()), "bytes outside the frames were written"
    return out.cpu()


def reference(y, u, v, h, w, layout, matrix):
    if layout == "nv12":
        return yuvref.to_bgr(y, yuvref.interleave(u, v), h, w, "nv12", matrix)
    return yuvref.to_bgr(y, u, h, w, "i420", matrix, v=v)


def host(y, u, v, h, w, layout, matrix):
    """lmx_h_yuv420_to_bgr on tight planes"""
    lib = _lib.load()
    y = np.ascontiguousarray(y)
    c = yuvref.interleave(u, v) if layout == "nv12" else np.ascontiguousarray(u)
    vv = np.ascontiguousarray(v) if layout == "i420" else None
    f = _lib.YuvFrames(y.ctypes.data, c.ctypes.data, vv.ctypes.data if vv is not None else None, y.strides[1], c.strides[1], y.strides[0], c.strides[0],
                       K.YUV_LAYOUTS[layout], K.YUV_MATRICES[matrix])
    out = np.empty((y.shape[0], h, w, 3), np.uint8)
    assert lib.lmx_h_yuv420_to_bgr(C.byref(f), y.shape[0], h, w, out.ctypes.data) == 0, lib.lmx_last_error().decode()
    return out


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_sizes_equal_the_reference_and_the_host_function(cuda, layout, matrix):
    """h in {2, 4, 18} x w in {2, 6, 14, 16, 18, 30, 32, 34, 66, 258}: a row shorter than a thread's 16-column block, exactly one block,
    whole blocks with a tail of 2 or 14 columns, and both sides of 16, 32 and 64 columns"""
    for h in (2, 4, 18):
        for w in (2, 6, 14, 16, 18, 30, 32, 34, 66, 258):
            y, u, v = yuvref.random_frame(h, w, 1, seed=1000 * h + w)
            want = reference(y, u, v, h, w, layout, matrix)
            assert np.array_equal(host(y, u, v, h, w, layout, matrix), want), (h, w)
            got = convert(cuda, *device_planes(cuda, y, u, v, layout), 1, h, w, layout, matrix)
            assert torch.equal(got, torch.from_numpy(want)), (h, w, int((got.numpy() != want).sum()))


PITCHES = {"w": lambda row: row, "w+1": lambda row: row + 1, "w+14": lambda row: row + 14, "next256": lambda row: -(-row // 256) * 256}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("w", [70, 64])
def test_alignments_pitches_and_strides(cuda, w, layout):
    """18 x 70 and 18 x 64, n = 3 with frame strides above a frame: plane base pointers offset by 0, 1, 2, 3 and 8 bytes, pitches w,
    w + 1, w + 14 and the next multiple of 256, the output at a 16-byte-aligned and at an odd address, both matrices"""
    n, h = 3, 18
    y, u, v = yuvref.random_frame(h, w, n, seed=w)
    want = {m: torch.from_numpy(reference(y, u, v, h, w, layout, m)) for m in MATRICES}
    for m in MATRICES:
        assert np.array_equal(host(y, u, v, h, w, layout, m), want[m].numpy()), m
    for offset in (0, 1, 2, 3, 8):
        for name, pitch in PITCHES.items():
            dy, dc, dv = device_planes(cuda, y, u, v, layout, pitch, extra_stride=37, offset=offset)
            assert dy.data_ptr() % 16 == offset and dy.stride(1) == pitch(w) and dy.stride(0) > h * dy.stride(1)
            for out_offset in (0, 5):
                for m in MATRICES:
                    got = convert(cuda, dy, dc, dv, n, h, w, layout, m, out_offset)
                    assert torch.equal(got, want[m]), (offset, name, out_offset, m, int((got != want[m]).sum()))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_result_does_not_depend_on_the_fill(cuda, layout):
    n, h, w = 2, 18, 70
    y, u, v = yuvref.random_frame(h, w, n, seed=5)
    planes = device_planes(cuda, y, u, v, layout, PITCHES["w+1"], offset=1)
    a = convert(cuda, *planes, n, h, w, layout, "bt601", 3, fill=0xA5)
    b = convert(cuda, *planes, n, h, w, layout, "bt601", 3, fill=0x00)
    assert torch.equal(a, b) and torch.equal(a, torch.from_numpy(reference(y, u, v, h, w, layout, "bt601")))


def test_1080p_nv12_surface_pitched_to_2048(cuda):
    """the shape the wide path was written for: every block whole, every address 16-byte aligned, some 500 workgroups; n = 2 so that the
    frame stride counts too"""
    n, h, w = 2, 1080, 1920
    y, u, v = yuvref.random_frame(h, w, n, seed=9)
    want = torch.from_numpy(reference(y, u, v, h, w, "nv12", "bt709"))
    dy, dc, dv = device_planes(cuda, y, u, v, "nv12", lambda row: 2048)
    assert dy.stride(1) == dc.stride(1) == 2048 and dy.data_ptr() % 16 == 0 and dc.data_ptr() % 16 == 0
    got = convert(cuda, dy, dc, dv, n, h, w, "nv12", "bt709")
    assert torch.equal(got, want), int((got != want).sum())


def test_more_blocks_than_the_grid_has_threads(cuda):
    """the launch is capped at 2048 workgroups of 256 threads and strides over the rest: 2 x 2 frames are one block each, so 2048 * 256
    + 1000 of them send some threads round the loop twice (and take the 64-bit frame offsets past a few megabytes)"""
    n, h, w = 2048 * 256 + 1000, 2, 2
    y, u, v = yuvref.random_frame(h, w, n, seed=11)
    for layout in LAYOUTS:
        want = torch.from_numpy(reference(y, u, v, h, w, layout, "bt601"))
        got = convert(cuda, *device_planes(cuda, y, u, v, layout), n, h, w, layout, "bt601")
        assert torch.equal(got, want), (layout, int((got != want).sum()))


def test_sweep_frame_on_the_device(cuda):
    """every listed (U, V) pair against every Y, saturation at both ends, both layouts and matrices"""
    y, u, v = yuvref.sweep_frame()
    h, w = y.shape[1:]
    for layout in LAYOUTS:
        planes = device_planes(cuda, y, u, v, layout)
        for m in MATRICES:
            got = convert(cuda, *planes, 1, h, w, layout, m)
            assert torch.equal(got, torch.from_numpy(reference(y, u, v, h, w, layout, m))), (layout, m)


def test_zero_frames_and_refusals(cuda):
    y, u, v = yuvref.random_frame()
    dy, dc, dv = device_planes(cuda, y, u, v, "i420")
    assert tuple(K.yuv420_to_bgr(dy[:0], dc[:0], 18, 70, layout="i420", v=dv[:0]).shape) == (0, 18, 70, 3)
    with pytest.raises(K.LmxError, match="even sizes"):
        K.yuv420_to_bgr(dy, dc, 17, 70, layout="i420", v=dv)
    with pytest.raises(K.LmxError, match="i420 takes the V plane"):
        K.yuv420_to_bgr(dy, dc, 18, 70, layout="i420")
    with pytest.raises(K.LmxError, match="CPU tensor"):
        K.yuv420_to_bgr(dy.cpu(), dc.cpu(), 18, 70, layout="i420", v=dv.cpu())
    torch.cuda.synchronize(cuda)
