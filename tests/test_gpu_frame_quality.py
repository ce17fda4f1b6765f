"""lmx_k_frame_quality (csrc/quality.hip) on the GPU: EQUAL to tests/qualityref.py, the numpy int64 form of the text in include/lmx.h,
and to lmx_h_frame_quality — on both sides of a thread's 16-column run, of a wave's 1024-column strip and of its 32-row band, for frames
at aligned and at odd byte addresses, at the sizes whose narrow accumulators carry the most (checkerboards: |lap| = 1020 everywhere),
alone and inside a batch, whatever `out` held before, with the words around `out` untouched."""
import numpy as np
import pytest
import torch

import qualityref as Q
from lmx import _lib
from lmx import kernels as K

pytestmark = pytest.mark.gpu
RUN, STRIP, BAND = 16, 1024, 32  # csrc/quality.hip: BW, SW, RB
GUARD = 8  # int64 words in front of and behind out


def host_sums(frames):
    lib = _lib.load()
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    out = np.empty((n, 4), np.int64)
    assert lib.lmx_h_frame_quality(frames.ctypes.data, n, h, w, out.ctypes.data) == 0, lib.lmx_last_error().decode()
    return out


def device_sums(dev, frames, offset=0, fill=0xA5):
    """K.frame_quality on a device view of `frames` (numpy u8 [n,h,w,3]) that starts `offset` bytes into its allocation, into an `out`
    that sits between guard words and holds `fill` bytes first; the guards must still hold the fill afterwards"""
    n, h, w, _ = frames.shape
    buf = torch.full((offset + frames.size,), 0x5A, dtype=torch.uint8, device=dev)
    view = buf[offset:].view(n, h, w, 3)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
    assert view.data_ptr() % 16 == offset % 16
    word = int(np.full(8, fill, np.uint8).view(np.int64)[0])
    guard = torch.full((GUARD + 4 * n + GUARD,), word, dtype=torch.int64, device=dev)
    out = guard[GUARD: GUARD + 4 * n].view(n, 4)
    got = K.frame_quality(view, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize(dev)
    assert bool((guard[:GUARD] == word).all()) and bool((guard[GUARD + 4 * n:] == word).all()), "words outside out were written"
    return out.cpu().numpy()


@pytest.mark.parametrize("size", Q.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_listed_sizes_equal_the_reference_and_the_host_function(cuda, size):
    h, w = size
    frames = Q.random_frames(3, h, w, seed=1000 * h + w)
    want = Q.sums(frames)
    assert np.array_equal(host_sums(frames), want)
    got = device_sums(cuda, frames)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("w", [RUN - 1, RUN, RUN + 1, STRIP - 1, STRIP, STRIP + 1])
def test_widths_and_heights_around_the_kernels_seams(cuda, w):
    """heights on both sides of one band and of two; n = 2 so that the frame stride counts.  w = 16 and w = 1024 with an aligned base
    take the 16-byte loads, everything else the byte loads"""
    for h in (BAND - 1, BAND, BAND + 1, 2 * BAND - 1, 2 * BAND, 2 * BAND + 1):
        frames = Q.random_frames(2, h, w, seed=7 * h + w)
        want = Q.sums(frames)
        got = device_sums(cuda, frames)
        assert np.array_equal(got, want), (h, w, got, want)
    assert np.array_equal(host_sums(frames), want)


@pytest.mark.parametrize("size", [(5, 7), (33, 48), (BAND + 1, STRIP + RUN)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_at_odd_and_aligned_byte_offsets(cuda, size):
    """the input starts 1, 3 and 16 bytes into its allocation: a thread's run is 16-byte aligned at offsets 0 and 16 only (w % 16 == 0)"""
    h, w = size
    frames = Q.random_frames(3, h, w, seed=h + w)
    want = Q.sums(frames)
    for offset in (0, 1, 3, 16):
        got = device_sums(cuda, frames, offset=offset)
        assert np.array_equal(got, want), (offset, got, want)


def test_checkerboards_hit_the_closed_form(cuda):
    """the overflow cases: |lap| = 1020 on every pixel.  8192 x 34 walks 256 bands of one narrow strip, 1080 x 1920 is the shape the wide
    path was written for (every run whole and aligned, 68 waves add into one frame's words)"""
    for h, w, first in ((8192, 34, 0), (1080, 1920, 255)):
        got = device_sums(cuda, Q.checkerboard(h, w, first))
        assert np.array_equal(got[0], Q.checkerboard_sums(h, w, first)), (h, w, got)
        assert got[0, 2] == 1040400 * h * w


def test_a_frame_alone_equals_the_frame_in_a_batch(cuda):
    h, w = 70, 1050
    frames = Q.random_frames(5, h, w, seed=3)
    batch = device_sums(cuda, frames)
    assert np.array_equal(batch, Q.sums(frames))
    for i in (0, 2, 4):
        assert np.array_equal(device_sums(cuda, frames[i:i + 1])[0], batch[i]), i


def test_result_does_not_depend_on_what_out_held(cuda):
    frames = Q.random_frames(2, 37, 1100, seed=5)
    want = Q.sums(frames)
    for fill in (0xA5, 0x00, 0xFF):
        assert np.array_equal(device_sums(cuda, frames, offset=1, fill=fill), want), fill
    assert np.array_equal(K.frame_quality(torch.from_numpy(frames).to(cuda)).cpu().numpy(), want)  # out allocated by the binding


def test_zero_frames_and_refusals(cuda):
    frames = torch.from_numpy(Q.random_frames(2, 5, 7)).to(cuda)
    assert tuple(K.frame_quality(frames[:0]).shape) == (0, 4)
    with pytest.raises(K.LmxError, match="2 or more"):
        K.frame_quality(frames[:, :1].contiguous())
    with pytest.raises(K.LmxError, match="2 or more"):
        K.frame_quality(frames[:, :, :1].contiguous())
    with pytest.raises(K.LmxError, match="contiguous uint8"):
        K.frame_quality(frames[:, :, ::2])
    with pytest.raises(K.LmxError, match="contiguous uint8"):
        K.frame_quality(frames.to(torch.int32))
    with pytest.raises(K.LmxError, match="contiguous uint8"):
        K.frame_quality(frames[..., :2].contiguous())
    with pytest.raises(K.LmxError, match="int64"):
        K.frame_quality(frames, out=torch.empty((2, 4), dtype=torch.int32, device=cuda))
    with pytest.raises(K.LmxError, match="CPU tensor"):
        K.frame_quality(frames.cpu())
    torch.cuda.synchronize(cuda)
