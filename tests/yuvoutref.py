"""numpy int64 references of the two texts in include/lmx.h behind lmx_k_yuv420_to_bgr (INTEGRATION.md "Frames to an encoder, and the
crop in between"), written from those texts and not from the C++.  Neither cv2 nor swscale is installed: parity with them is UNPINNED;
this file is the pin.

The window: output pixel (i, j) of roi = (x, y, w, h) is pixel (x + i, y + j) of tests/yuvref.py's to_bgr — the whole frame converted
by that file, then sliced.

BGR -> YUV 4:2:0, limited range, 20-bit fixed point, chroma from the 2 x 2 box:

    Y(x, y) = sat8(((YB B + YG G + YR R + 2^19) >> 20) + 16)
    SB, SG, SR = sums of B, G, R over pixels (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1)
    U(i, j) = sat8(((UB SB + UG SG + UR SR + 2^21) >> 22) + 128);  V(i, j) = sat8(((VB SB + VG SG + VR SR + 2^21) >> 22) + 128)

`defect` switches one of five wrong models on, for the tests that show the right formula is told apart from each."""
import numpy as np

import yuvref

SHIFT = 20
# three-decimal constants: (YB, YG, YR), (UB, UG, UR), (VB, VG, VR)
CONSTANTS = {"bt601": ((0.098, 0.504, 0.257), (0.439, -0.291, -0.148), (-0.071, -0.368, 0.439)),
             "bt709": ((0.062, 0.614, 0.183), (0.439, -0.338, -0.101), (-0.040, -0.399, 0.439))}
COEF = {m: tuple(tuple(int(round(c * 2 ** SHIFT)) for c in row) for row in rows) for m, rows in CONSTANTS.items()}
# full-range (JFIF) BT.601 rows, for the defect model only
FULL_RANGE = tuple(tuple(int(round(c * 2 ** SHIFT)) for c in row) for row in ((0.114, 0.587, 0.299), (0.5, -0.331, -0.169), (-0.081, -0.419, 0.5)))
DEFECTS = ("chroma_top_left", "chroma_rounded_mean", "no_rounding", "swap_rb", "full_range")


def window(y, c, h, w, roi, layout="nv12", matrix="bt601", v=None):
    """the window roi = (x, y, w, h) of the frames -> uint8 [n, roi h, roi w, 3]: yuvref.to_bgr of the whole frame, sliced"""
    rx, ry, rw, rh = roi
    assert rw >= 1 and rh >= 1 and rx >= 0 and ry >= 0 and rx + rw <= w and ry + rh <= h
    return np.ascontiguousarray(yuvref.to_bgr(y, c, h, w, layout, matrix, v=v)[:, ry:ry + rh, rx:rx + rw])


def from_bgr(frames, matrix="bt601", defect=None):
    """uint8 [n, h, w, 3] BGR (any strides) -> (y [n,h,w], u [n,h/2,w/2], v [n,h/2,w/2]) uint8"""
    assert defect is None or defect in DEFECTS
    f = np.asarray(frames).astype(np.int64)
    n, h, w, _ = f.shape
    assert h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0
    ky, ku, kv = FULL_RANGE if defect == "full_range" else COEF[matrix]
    b, g, r = (f[..., 2], f[..., 1], f[..., 0]) if defect == "swap_rb" else (f[..., 0], f[..., 1], f[..., 2])
    ty = ky[0] * b + ky[1] * g + ky[2] * r + (1 << (SHIFT - 1))
    assert int(np.abs(ty).max(initial=0)) < 2 ** 31, "the text promises 32-bit intermediates"
    y = np.clip((ty >> SHIFT) + (0 if defect == "full_range" else 16), 0, 255).astype(np.uint8)

    def box(p):  # the 2 x 2 sums, 0 .. 1020
        return p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]

    if defect == "chroma_top_left":
        sb, sg, sr = (4 * p[:, 0::2, 0::2] for p in (b, g, r))
    elif defect == "chroma_rounded_mean":
        sb, sg, sr = (4 * ((box(p) + 2) >> 2) for p in (b, g, r))
    else:
        sb, sg, sr = box(b), box(g), box(r)
    half = 0 if defect == "no_rounding" else 1 << (SHIFT + 1)
    out = [y]
    for k in (ku, kv):
        t = k[0] * sb + k[1] * sg + k[2] * sr + half
        assert int(np.abs(t).max(initial=0)) < 2 ** 31, "the text promises 32-bit intermediates"
        out.append(np.clip((t >> (SHIFT + 2)) + 128, 0, 255).astype(np.uint8))  # >> on int64: arithmetic = floor
    return tuple(out)


def random_bgr(h, w, n=1, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
