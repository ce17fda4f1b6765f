"""lmx_k_bgr_to_yuv420 and lmx_k_yuv420_to_bgr_roi (csrc/yuv.hip) on the GPU: EQUAL to tests/yuvoutref.py, the numpy int64 form of
the texts in include/lmx.h, over the same matrix of sizes, pitches, bases and windows as tests/test_yuv_egress_host.py (the runners of
tests/yuvegress.py on device memory) — whole output buffers compared, so the guard bytes around and between the planes are checked
untouched — and on the cases that pin a path: everything aligned (every piece wide), an aligned surface under a window at x = 3
(wide loads, byte stores), a sliced view against its contiguous copy, and n = 3 under a grid-stride loop that crosses frames."""
import numpy as np
import pytest
import torch

import yuvegress as E
import yuvoutref
import yuvref
from lmx import _lib
from lmx import kernels as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_bgr_to_yuv420_equals_the_reference(cuda, layout, matrix):
    """the host test's matrix: 2x2, 2x18, 6x34, 4x50; n = 2 with frame strides above a frame; pitches of row + 0 / 1 / 13; bases + 0 / + 1"""
    arena, fn = E.DeviceArena(cuda), _lib.load().lmx_k_bgr_to_yuv420
    for h, w in E.SIZES:
        frames = yuvoutref.random_bgr(h, w, 2, seed=100 * h + w)
        for extra in E.PITCH_EXTRA:
            for offset in E.OFFSETS:
                E.bgr_to_yuv420(fn, arena, frames, layout, matrix, src_extra=extra, src_offset=offset, out_extra=extra, out_offset=offset, extra_stride=37)
        E.bgr_to_yuv420(fn, arena, frames, layout, matrix, src_extra=13, src_offset=0, out_extra=0, out_offset=1, extra_stride=5)


@pytest.mark.parametrize("matrix", list(E.MATRICES))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_windows_equal_the_reference(cuda, layout, matrix):
    """the host test's windows on an 18 x 70 frame, n = 2, source pitches of row + 0 / 1 / 13, bases at + 0 / + 1"""
    arena, fn = E.DeviceArena(cuda), _lib.load().lmx_k_yuv420_to_bgr_roi
    h, w = E.FRAME
    y, u, v = yuvref.random_frame(h, w, 2, seed=3)
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
    want = {roi: yuvoutref.window(y, c, h, w, roi, layout, matrix, v=vv) for roi in E.WINDOWS}
    for extra in E.PITCH_EXTRA:
        for offset in E.OFFSETS:
            f, keep = E.source_planes(arena, y, u, v, layout, matrix, extra, offset, extra_stride=37)
            for roi in E.WINDOWS:
                E.window(fn, arena, f, 2, h, w, roi, want[roi], out_offset=offset)
            del keep


@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_everything_aligned_takes_the_wide_path(cuda, layout):
    """w = 64, pitches that are multiples of 16, bases on 16-byte boundaries, in both directions: no piece is moved byte by byte; n = 3"""
    arena, lib = E.DeviceArena(cuda), _lib.load()
    h, w, n = 6, 64, 3
    frames = yuvoutref.random_bgr(h, w, n, seed=21)
    E.bgr_to_yuv420(lib.lmx_k_bgr_to_yuv420, arena, frames, layout, "bt709", src_extra=16, out_extra=16, extra_stride=32)
    y, u, v = yuvref.random_frame(h, w, n, seed=22)
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
    f, keep = E.source_planes(arena, y, u, v, layout, "bt709", 16, 0, extra_stride=32)
    for roi in ((0, 0, 64, 6), (16, 2, 48, 4)):  # x, w multiples of 16: output rows of 192 / 144 bytes, 16-byte aligned
        E.window(lib.lmx_k_yuv420_to_bgr_roi, arena, f, n, h, w, roi, yuvoutref.window(y, c, h, w, roi, layout, "bt709", v=vv))


@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_aligned_surface_under_a_window_at_x_3(cuda, layout):
    """w = 64, an aligned surface and a window at x = 3: the blocks lie on the source's grid, so the loads stay wide, and every store is
    byte-wise (the first and last blocks are partial, the others land at odd output addresses)"""
    arena, lib = E.DeviceArena(cuda), _lib.load()
    h, w, n = 6, 64, 3
    y, u, v = yuvref.random_frame(h, w, n, seed=23)
    c, vv = (yuvref.interleave(u, v), None) if layout == "nv12" else (u, v)
    f, keep = E.source_planes(arena, y, u, v, layout, "bt601", 0, 0)
    for roi in ((3, 1, 58, 4), (3, 0, 61, 6)):
        E.window(lib.lmx_k_yuv420_to_bgr_roi, arena, f, n, h, w, roi, yuvoutref.window(y, c, h, w, roi, layout, "bt601", v=vv))


@pytest.mark.parametrize("layout", list(E.LAYOUTS))
def test_sliced_view_equals_its_contiguous_copy(cuda, layout):
    """K.bgr_to_yuv420 on frames[:, y0:y1, x0:x1] (pitch and stride from the tensor's strides, an odd x0: byte-wise loads) against the
    same call on a contiguous copy and against the reference"""
    frames = yuvoutref.random_bgr(20, 72, 3, seed=24)
    d = torch.from_numpy(frames).to(cuda)
    for x0, y0, x1, y1 in ((3, 1, 53, 15), (16, 2, 64, 20)):
        view = d[:, y0:y1, x0:x1]
        assert not view.is_contiguous()
        a = K.bgr_to_yuv420(view, layout=layout, matrix="bt709")
        b = K.bgr_to_yuv420(view.contiguous(), layout=layout, matrix="bt709")
        want = yuvoutref.from_bgr(frames[:, y0:y1, x0:x1], "bt709")
        want = (want[0], yuvref.interleave(want[1], want[2])) if layout == "nv12" else want
        assert len(a) == len(b) == len(want)
        for pa, pb, pw in zip(a, b, want):
            assert torch.equal(pa, pb) and np.array_equal(pa.cpu().numpy(), pw)


def test_grid_stride_loop_crosses_frames(cuda):
    """2 x 2 frames are one block each: 2048 * 256 + 1000 of them send some threads round the loop twice, in both kernels"""
    n = 2048 * 256 + 1000
    frames = yuvoutref.random_bgr(2, 2, n, seed=25)
    got = K.bgr_to_yuv420(torch.from_numpy(frames).to(cuda), layout="i420", matrix="bt601")
    for g, wnt in zip(got, yuvoutref.from_bgr(frames, "bt601")):
        assert np.array_equal(g.cpu().numpy(), wnt)
    y, u, v = yuvref.random_frame(2, 2, n, seed=26)
    dy, du, dv = (torch.from_numpy(t).to(cuda) for t in (y, u, v))
    got = K.yuv420_to_bgr_roi(dy, du, 2, 2, (1, 0, 1, 2), layout="i420", v=dv)
    assert np.array_equal(got.cpu().numpy(), yuvoutref.window(y, u, 2, 2, (1, 0, 1, 2), "i420", "bt601", v=v))


def test_python_wrappers_refuse_and_pass_zero_frames(cuda):
    y, u, v = (torch.from_numpy(t).to(cuda) for t in yuvref.random_frame())
    assert tuple(K.yuv420_to_bgr_roi(y[:0], u[:0], 18, 70, (1, 1, 5, 3), layout="i420", v=v[:0]).shape) == (0, 3, 5, 3)
    with pytest.raises(K.LmxError, match="is outside the 18 x 70 frame"):
        K.yuv420_to_bgr_roi(y, u, 18, 70, (60, 0, 11, 4), layout="i420", v=v)
    with pytest.raises(K.LmxError, match="roi is empty"):
        K.yuv420_to_bgr_roi(y, u, 18, 70, (0, 0, 0, 4), layout="i420", v=v)
    frames = torch.zeros((1, 6, 34, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(K.LmxError, match="even sizes"):
        K.bgr_to_yuv420(frames[:, :5])
    with pytest.raises(K.LmxError, match="packed pixels"):
        K.bgr_to_yuv420(frames[:, :, ::2])
    with pytest.raises(K.LmxError, match="CPU tensor"):
        K.bgr_to_yuv420(frames.cpu())
    assert [tuple(t.shape) for t in K.bgr_to_yuv420(frames[:0])] == [(0, 6, 34), (0, 3, 34)]
    torch.cuda.synchronize(cuda)
