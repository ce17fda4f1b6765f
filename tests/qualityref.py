"""numpy restatement of the text at lmx_k_frame_quality in include/lmx.h, independent of csrc/host_quality.cpp: integer gray, np.pad for
the reflected border, int64 sums.  Five named defect models produce the results of plausible wrong implementations, so that a fixture
which cannot tell them from the right one is known to be too weak.  cv2 is not installed: the text is the definition (PARITY UNPINNED)."""
import numpy as np

DEFECTS = ("rgb_order", "coef14", "truncate", "replicate", "symmetric")
SIZES = ((2, 2), (2, 3), (3, 2), (5, 7), (17, 33), (33, 1027))


def gray(frames, defect=None):
    """u8 BGR [n,h,w,3] -> int64 [n,h,w]"""
    f = np.asarray(frames).astype(np.int64)
    b, g, r = (f[..., 2], f[..., 1], f[..., 0]) if defect == "rgb_order" else (f[..., 0], f[..., 1], f[..., 2])
    if defect == "coef14":  # the 14-bit coefficients of older OpenCV
        return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14
    return (3735 * b + 19235 * g + 9798 * r + (0 if defect == "truncate" else 16384)) >> 15


def laplacian(g, defect=None):
    """int64 [n,h,w] -> int64 [n,h,w]: ksize 1 under BORDER_REFLECT_101 (np.pad's "reflect")"""
    mode = {"replicate": "edge", "symmetric": "symmetric"}.get(defect, "reflect")
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode=mode)
    return p[:, 1:-1, :-2] + p[:, 1:-1, 2:] + p[:, :-2, 1:-1] + p[:, 2:, 1:-1] - 4 * g


def sums(frames, defect=None):
    """u8 BGR [n,h,w,3] -> int64 [n,4]: (sum g, sum lap, sum lap^2, h * w) per frame"""
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    out = np.empty((n, 4), np.int64)
    for i in range(n):  # one frame at a time: the int64 intermediates of a 1080p batch are large
        g = gray(frames[i:i + 1], defect)
        lap = laplacian(g, defect)
        out[i] = (g.sum(), lap.sum(), (lap * lap).sum(), h * w)
    return out


def random_frames(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def checkerboard(h, w, first=0):
    """u8 [1,h,w,3]: 0 / 255 squares of one pixel, pixel (0, 0) = first"""
    yy, xx = np.mgrid[0:h, 0:w]
    v = np.where((yy + xx) % 2 == 0, first, 255 - first).astype(np.uint8)
    return np.repeat(v[None, :, :, None], 3, axis=3)


def checkerboard_sums(h, w, first=0):
    """the closed form: every neighbour of a pixel, reflected ones included, has the other colour, so lap = +1020 on black, -1020 on white"""
    n_first = (h * w + 1) // 2
    n_black, n_white = (n_first, h * w - n_first) if first == 0 else (h * w - n_first, n_first)
    return np.array([255 * n_white, 1020 * (n_black - n_white), 1040400 * h * w, h * w], np.int64)
