"""lmx_k_contour_features labels row RUNS (csrc/contour.hip: 64-bit bit rows, run boundaries, unions between runs of
adjacent rows).  These cases put the run boundaries where that indexing can go wrong — on 64-bit word edges, on both frame
edges, at widths that are no multiple of 4 or 64, behind an unaligned mask pointer, at the worst-case run count — and compare
with the sequential border following of csrc/host_mask.cpp BIT FOR BIT, like tests/test_gpu_contour.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KEYS = ["mask_area", "area_ratio", "circularity", "aspect_ratio", "centroid_x", "centroid_y", "perimeter"]
WIDTHS = [2, 3, 63, 64, 65, 127, 128, 130, 1918, 1919, 1920]


def _host(mask):
    from lmx import _lib

    m = np.ascontiguousarray(mask.astype(np.uint8))
    out = (C.c_double * 7)()
    assert _lib.load().lmx_h_mask_features(m.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], C.cast(out, C.c_void_p)) == 0
    return dict(zip(KEYS, list(out)))


def _contour(masks, cuda, offset=0):
    """masks bool/u8 [n,h,w] -> int64 [n,8] on the host; the device copy starts `offset` bytes into its allocation."""
    from lmx import kernels as K

    m = np.ascontiguousarray(np.asarray(masks).astype(np.uint8))
    buf = torch.empty(m.size + 16, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + m.size].view(m.shape)
    view.copy_(torch.from_numpy(m).to(cuda))
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return K.contour_features(view).cpu().numpy()


def _check(masks, cuda, label, offset=0):
    from lmx.services.sam3_pipeline import features_from_device

    masks = np.asarray(masks)
    n, h, w = masks.shape
    cont = _contour(masks, cuda, offset)
    for i in range(n):
        ys, xs = np.nonzero(masks[i])
        dev = features_from_device([len(xs), int(xs.sum()), int(ys.sum())], cont[i], h, w)
        ref = _host(masks[i])
        for k in KEYS:
            assert dev[k] == ref[k], f"{label}[{i}] {k}: device {dev[k]!r} host {ref[k]!r} (contour row {cont[i].tolist()})"
    return cont


def _width_cases(w, rng):
    """[n, h, w] masks whose runs start and end on the word edges (x = 63, 64, 127, 128, ...) and on x = 0 and x = w - 1."""
    h = 24
    out = []
    m = np.zeros((h, w), bool); m[3:20, :] = True; out.append(m)                                   # rows that are one run, frame to frame
    m = np.zeros((h, w), bool); m[2:9, 0:max(1, w // 2)] = True; m[12:22, w // 2:] = True; out.append(m)  # touching x = 0, touching x = w - 1
    m = np.zeros((h, w), bool)                                                                       # runs that end at 63 / start at 64, ...
    for e in range(64, w + 64, 64):
        m[2:6, max(0, e - 5):min(w, e)] = True        # ends on the last bit of a word
        m[8:12, min(w - 1, e):min(w, e + 5)] = True   # starts on the first bit of the next
        m[14:18, max(0, e - 3):min(w, e + 3)] = True  # crosses the edge
    out.append(m)
    m = np.zeros((h, w), bool)                                                                       # a diagonal staircase across the word edges
    for y in range(h):
        x = (y * max(1, w - 1)) // (h - 1)
        m[y, min(w - 1, x)] = True
    out.append(m)
    m = np.ones((h, w), bool); m[5:15, w // 3:max(w // 3 + 1, 2 * w // 3)] = False; out.append(m)    # a hole: inner background is not outside
    for k in range(3):                                                                              # blobs with salt and pepper
        cell = 4
        g = rng.random(((h + cell - 1) // cell, (w + cell - 1) // cell))
        m = np.kron(g, np.ones((cell, cell)))[:h, :w] > rng.uniform(0.4, 0.7)
        m ^= rng.random(m.shape) > 0.96
        out.append(m)
    return np.stack(out, 0)


@pytest.mark.parametrize("w", WIDTHS)
def test_widths_at_word_and_frame_edges(cuda, w):
    _check(_width_cases(w, np.random.default_rng(w)), cuda, f"w={w}")


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("w", [64, 130, 1920])
def test_mask_pointer_offset(cuda, offset, w):
    masks = _width_cases(w, np.random.default_rng(100 + w))
    cont = _check(masks, cuda, f"w={w} offset={offset}", offset)
    assert np.array_equal(cont, _contour(masks, cuda, 0))  # the byte-wise reader writes the bits the word-wise one writes


def test_full_empty_and_checkerboard(cuda):
    """The one-pixel checkerboard has one run per pixel: the worst case lmx_contour_workspace_bytes must cover."""
    h, w = 64, 130
    yy, xx = np.mgrid[0:h, 0:w]
    cb = (xx + yy) % 2 == 0
    masks = np.stack([np.ones((h, w), bool), np.zeros((h, w), bool), cb, ~cb], 0)
    cont = _check(masks, cuda, "full/empty/checkerboard")
    assert cont[0].tolist() == [2 * (w - 1) * (h - 1), 2 * (w - 1) + 2 * (h - 1), 0, 0, 0, w - 1, h - 1, 1]
    assert cont[1].tolist() == [0] * 8
    assert cont[2][7] == 1 and cont[3][7] == 1  # 8-connected: one component each
    for ww in (2, 3, 63, 65, 1919):  # worst-case run count at widths that are odd or smaller than a word
        hh = 2 if ww == 1919 else 7
        yy, xx = np.mgrid[0:hh, 0:ww]
        _check(np.stack([(xx + yy) % 2 == 0, (xx + yy) % 2 == 1, xx % 2 == 0, xx % 2 == 1], 0), cuda, f"checkerboard w={ww}")


def test_workspace_covers_any_mask_within_todays_size():
    from lmx import _lib

    lib = _lib.load()
    for h in list(range(2, 40)) + [64, 1080]:
        for w in list(range(2, 140)) + WIDTHS:
            for n in (1, 30):
                b = lib.lmx_contour_workspace_bytes(n, h, w)
                assert 0 < b <= n * (36 * h * w + 4), (n, h, w, b)


def test_root_is_first_pixel_in_raster_order_not_leftmost(cuda):
    """The root of a component is its first pixel in raster order; here that pixel is far right of the leftmost column, in
    another 64-bit word, and the external test (west neighbour of the root) and the tie-break key both hang on it."""
    h, w = 40, 200
    m = np.zeros((h, w), bool)
    m[5, 150:160] = True       # first row of the component: x = 150
    m[6:20, 155] = True        # stem down
    m[20, 10:156] = True       # foot reaching left to x = 10
    m[21:30, 10] = True
    cont = _check(m[None], cuda, "root")
    assert cont[0][3:7].tolist() == [10, 5, 159, 29] and cont[0][7] == 1
    # the same shape inside a ring: the ring is the one external contour, and ITS root is (2, 2)
    r = np.zeros((h, w), bool)
    r[2, 2:198] = True; r[37, 2:198] = True; r[2:38, 2] = True; r[2:38, 197] = True
    cont = _check((m | r)[None], cuda, "root in ring")
    assert cont[0][3:7].tolist() == [2, 2, 197, 37] and cont[0][7] == 1


def test_equal_area_components_first_in_raster_order_wins(cuda):
    h, w = 40, 200
    m = np.zeros((h, w), bool)
    m[20:30, 5:15] = True      # lower left ...
    m[4:14, 120:130] = True    # ... and upper right, same area: the upper one is first in raster order
    cont = _check(m[None], cuda, "tie")
    assert cont[0].tolist() == [2 * 9 * 9, 4 * 9, 0, 120, 4, 129, 13, 2]
    m2 = np.zeros((h, w), bool)
    m2[10:20, 60:70] = True    # same first row: the left one is first
    m2[10:20, 64 + 60:64 + 70] = True
    cont = _check(m2[None], cuda, "tie in a row")
    assert cont[0].tolist() == [2 * 9 * 9, 4 * 9, 0, 60, 10, 69, 19, 2]


def test_frame_alone_and_inside_a_batch_of_30(cuda):
    rng = np.random.default_rng(5)
    h, w = 270, 480
    masks = []
    for j in range(30):
        g = rng.random((9, 16))
        m = np.kron(g, np.ones((30, 30))) > 0.45 + 0.01 * j
        if j % 3 == 0:
            m ^= rng.random(m.shape) > 0.995
        masks.append(m)
    masks = np.stack(masks, 0)
    from lmx import kernels as K

    d = torch.from_numpy(masks.astype(np.uint8)).to(cuda)
    whole = K.contour_features(d)
    for j in (0, 7, 29):
        assert torch.equal(K.contour_features(d[j:j + 1].contiguous()), whole[j:j + 1])
    _check(masks[[0, 7, 29]], cuda, "batch")
