"""numpy int64 reference of the YUV 4:2:0 -> BGR conversion (include/lmx.h at lmx_k_yuv420_to_bgr; INTEGRATION.md "Frames from a
decoder"), written from that text and not from the C++: limited range, 20-bit fixed point, nearest chroma — the public integer form
of cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420).  cv2 is not installed: parity with real OpenCV is UNPINNED; this file is the pin.

    Y = y[y, x];  nv12: U, V = c[y >> 1, 2 (x >> 1)], the byte after it;  i420: U = u[y >> 1, x >> 1], V = v[the same]
    yy = max(0, Y - 16) CY;  B = sat8((yy + CUB (U - 128) + 2^19) >> 20);  G = sat8((yy + CUG (U - 128) + CVG (V - 128) + 2^19) >> 20)
    R = sat8((yy + CVR (V - 128) + 2^19) >> 20);  out[y, x] = (B, G, R)

`defect` switches one of five wrong models on, for the tests that show the right formula is told apart from each."""
import numpy as np

SHIFT = 20
# three-decimal constants: Y gain | U -> B, U -> G, V -> G, V -> R
CONSTANTS = {"bt601": (1.164, 2.018, -0.391, -0.813, 1.596), "bt709": (1.164, 2.112, -0.213, -0.533, 1.793)}
COEF = {m: tuple(int(round(c * 2 ** SHIFT)) for c in cs) for m, cs in CONSTANTS.items()}
DEFECTS = ("no_rounding", "no_clamp", "swap_uv", "chroma_row", "chroma_col")


def chroma_planes(c, h, w, layout, v=None):
    """(U, V) as [n, h/2, w/2] arrays from the interleaved plane c [n, h/2, w] (nv12) or from the planes c, v (i420)"""
    if layout == "nv12":
        assert v is None
        return c[:, : h // 2, 0:w:2], c[:, : h // 2, 1:w:2]
    assert layout == "i420" and v is not None
    return c[:, : h // 2, : w // 2], v[:, : h // 2, : w // 2]


def to_bgr(y, c, h, w, layout="nv12", matrix="bt601", v=None, defect=None):
    """y uint8 [n, >= h, >= w], c / v as chroma_planes takes them -> uint8 [n, h, w, 3]"""
    assert defect is None or defect in DEFECTS
    assert h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0
    cy, cub, cug, cvg, cvr = COEF[matrix]
    U, V = chroma_planes(np.asarray(c), h, w, layout, None if v is None else np.asarray(v))
    if defect == "swap_uv":
        U, V = V, U
    ys, xs = np.arange(h), np.arange(w)
    rows = np.minimum(ys, h // 2 - 1) if defect == "chroma_row" else ys >> 1
    cols = np.minimum(xs, w // 2 - 1) if defect == "chroma_col" else xs >> 1
    U = U.astype(np.int64)[:, rows][:, :, cols] - 128
    V = V.astype(np.int64)[:, rows][:, :, cols] - 128
    Y = np.asarray(y)[:, :h, :w].astype(np.int64) - 16
    yy = (Y if defect == "no_clamp" else np.maximum(Y, 0)) * cy
    half = 0 if defect == "no_rounding" else 1 << (SHIFT - 1)
    chan = (yy + cub * U + half, yy + cug * U + cvg * V + half, yy + cvr * V + half)
    assert all(int(np.abs(t).max(initial=0)) < 2 ** 31 for t in chan), "the text promises 32-bit intermediates"
    return np.stack([np.clip(t >> SHIFT, 0, 255) for t in chan], axis=-1).astype(np.uint8)  # >> on int64: arithmetic = floor


def random_frame(h=18, w=70, n=1, seed=0):
    """(y [n,h,w], u [n,h/2,w/2], v [n,h/2,w/2]) uniform bytes from default_rng(seed)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8))


def sweep_frame():
    """162 x 512: chroma block-row j holds the j-th of the 81 (U, V) pairs over {0, 1, 16, 127, 128, 129, 240, 254, 255}^2; Y = x >> 1 on
    even rows and 255 - (x >> 1) on odd rows: every Y meets every listed pair, and saturation is reached at both ends"""
    vals = (0, 1, 16, 127, 128, 129, 240, 254, 255)
    h, w = 2 * len(vals) ** 2, 512
    pairs = np.array([(a, b) for a in vals for b in vals], np.uint8)
    u = np.repeat(pairs[:, 0:1], w // 2, axis=1)[None]
    v = np.repeat(pairs[:, 1:2], w // 2, axis=1)[None]
    ramp = (np.arange(w) >> 1).astype(np.uint8)
    y = np.empty((1, h, w), np.uint8)
    y[0, 0::2] = ramp
    y[0, 1::2] = 255 - ramp
    return y, u, v


def interleave(u, v):
    """the NV12 chroma plane [n, h/2, w] of two planes [n, h/2, w/2]"""
    c = np.empty(u.shape[:2] + (2 * u.shape[2],), np.uint8)
    c[..., 0::2], c[..., 1::2] = u, v
    return c


def bgr_to_yuv(frames):
    """a fixed, deterministic BGR -> (y, u, v) map for tests that need decoder-shaped inputs made from BGR frames (BT.601 studio swing
    in integers, chroma taken from the top-left pixel of each 2 x 2 block); it is no inverse of to_bgr and need not be"""
    f = np.asarray(frames).astype(np.int64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = np.clip(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, 0, 255).astype(np.uint8)
    u = np.clip(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, 0, 255).astype(np.uint8)[:, 0::2, 0::2]
    v = np.clip(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128, 0, 255).astype(np.uint8)[:, 0::2, 0::2]
    return y, np.ascontiguousarray(u), np.ascontiguousarray(v)
