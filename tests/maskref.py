"""float64 reference of SAM's mask output chain, written from the text of include/lmx.h and not from the kernels:
lmx_k_hyper_mask / _multi (hyper_mask), lmx_k_mask_post / lmx_k_mask_logits / lmx_k_mask_score (postprocess, stats), with the
geometries, the smooth fixture and the bounds that tests/test_gpu_mask_output.py holds the kernels to.
tests/test_mask_ref_host.py establishes every constant below on the CPU, without the code under test."""
import numpy as np
import torch
import torch.nn.functional as F

import samprompt as SP


# ---------------------------------------------------------------------------------------------------------------- hyper_mask
def hyper_mask(up, hyper):
    """logits[b, 4y + 2dy1 + dy2, 4x + 2dx1 + dx2] = sum_c up[b, y, x, dy1, dx1, dy2, dx2, c] * hyper[b, c] in float64.
    up [n, G, G, 2, 2, 2, 2, C], hyper [n, C] (or [n, M, C]) -> (logits [n, 4G, 4G] (or [n, M, 4G, 4G]), mag = the same sum over
    |up_c * hyper_c|, which scales the error bound of an f32 fma chain)."""
    hy = hyper.double()
    single = hy.dim() == 2
    if single:
        hy = hy[:, None]
    n, G = up.shape[0], up.shape[1]
    M = hy.shape[1]
    out = torch.zeros(n, M, 4 * G, 4 * G, dtype=torch.float64)
    mag = torch.zeros_like(out)
    for dy1 in range(2):
        for dx1 in range(2):
            for dy2 in range(2):
                for dx2 in range(2):
                    u = up[:, :, :, dy1, dx1, dy2, dx2, :].double()  # [n, G(y), G(x), C]
                    out[:, :, 2 * dy1 + dy2::4, 2 * dx1 + dx2::4] = torch.einsum("byxc,bmc->bmyx", u, hy)
                    mag[:, :, 2 * dy1 + dy2::4, 2 * dx1 + dx2::4] = torch.einsum("byxc,bmc->bmyx", u.abs(), hy.abs())
    return (out[:, 0], mag[:, 0]) if single else (out, mag)


def hyper_mask_bound(mag, C):
    """|f32 fma chain of C terms - exact| <= (C + 1) * 2^-24 * sum_c |up_c * hyper_c| (the products are exact in the fma, each
    of the C additions rounds once, (1 + u)^C - 1 <= (C + 1) u for C <= 64)."""
    return (C + 1) * 2.0 ** -24 * mag


# ---------------------------------------------------------------------------------------------------------------- resize
def resized(h, w, T):
    """segment_anything ResizeLongestSide.get_preprocess_shape"""
    s = T * 1.0 / max(h, w)
    return int(h * s + 0.5), int(w * s + 0.5)


def postprocess(low, T, resized_hw, hw):
    """Sam.postprocess_masks without the threshold in low's dtype: [n, L, L] -> bilinear (align_corners=False) to T x T, crop
    [:nh, :nw], bilinear to h x w.  On a .double() tensor this is the float64 reference."""
    return SP.postprocess_logits(low[:, None], resized_hw, hw, target=T)[:, 0]


def stats(mask):
    """area, sum_x, sum_y, min_x, min_y, max_x, max_y of one [h, w] mask, int64 (None for the box of an empty mask)."""
    m = np.asarray(mask) != 0
    ys, xs = np.nonzero(m)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    if len(ys) == 0:
        return [0, 0, 0, None, None, None, None]
    return [int(len(ys)), int(xs.sum()), int(ys.sum()), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


# (h, w, L, T): what each reaches is in the table of tests/test_gpu_mask_output.py
GEOMETRIES = [
    (97, 130, 256, 1024), (333, 517, 256, 1024), (541, 962, 256, 1024), (1030, 1031, 256, 1024), (1079, 1919, 256, 1024),
    (1, 1024, 256, 1024), (1024, 1, 256, 1024), (2, 3, 256, 1024), (64, 64, 64, 256), (150, 100, 128, 512), (1080, 1920, 256, 1024),
]
N_MASKS = 3


def geo_id(g):
    return f"{g[0]}x{g[1]}-L{g[2]}-T{g[3]}"


def fixture(geo):
    """The smooth fixture: N_MASKS 12 x 12 normal seeds x 10, interpolated to L x L (f32, as the kernels read it)."""
    g = torch.Generator().manual_seed(SEEDS[geo])
    seeds = torch.randn(N_MASKS, 1, 12, 12, generator=g) * 10
    return F.interpolate(seeds, size=(geo[2], geo[2]), mode="bilinear", align_corners=False)[:, 0].contiguous()


def e_ref(geo, low=None):
    """max |postprocess in f32 on the CPU - postprocess in float64| / max|low|: what rounding the source coordinate
    scale * (dst + 0.5) - 0.5 and the blends to f32 costs, without the device.  -> (e_ref, ref64, top)"""
    h, w, L, T = geo
    low = fixture(geo) if low is None else low
    rhw = resized(h, w, T)
    ref64 = postprocess(low.double(), T, rhw, (h, w))
    ref32 = postprocess(low, T, rhw, (h, w))
    top = float(low.abs().max())
    return float((ref32.double() - ref64).abs().max()) / top, ref64, top


def ambiguous(ref64, bound):
    """pixels whose sign the bound does not decide"""
    return ref64.abs() <= bound


# The device against torch's f32 result: 2^-20 max|low| everywhere (neither side is exact, and both round the same coordinate).
LOG2_BOUND32 = -20
# The device against float64: 2^-18 max|low| where e_ref <= 2^-19 (half of it); elsewhere 4 x e_ref rounded up to a power of two.
# Measured e_ref per geometry (test_mask_ref_host.py prints them) beside each.
# No geometry exceeds 2^-19, so none is raised; the largest, 2^-19.70, is the 1080 x 1920 anchor the 2^-18 came from.
LOG2_BOUND64 = {
    (97, 130, 256, 1024): -18,     # e_ref 2^-19.98
    (333, 517, 256, 1024): -18,    # e_ref 2^-20.30
    (541, 962, 256, 1024): -18,    # e_ref 2^-20.44
    (1030, 1031, 256, 1024): -18,  # e_ref 2^-19.93
    (1079, 1919, 256, 1024): -18,  # e_ref 2^-19.97
    (1, 1024, 256, 1024): -18,     # e_ref 2^-24.07
    (1024, 1, 256, 1024): -18,     # e_ref 2^-24.56
    (2, 3, 256, 1024): -18,        # e_ref 2^-22.12
    (64, 64, 64, 256): -18,        # e_ref 2^-23.04
    (150, 100, 128, 512): -18,     # e_ref 2^-20.19
    (1080, 1920, 256, 1024): -18,  # e_ref 2^-19.70
}
LOG2_KEPT = -18  # a geometry at this exponent kept the existing bound (e_ref <= half of it); any other was raised to >= 4 x e_ref
# One seed serves every geometry: all 33 masks cover between 33 % and 62 % of their frame, and the worst ambiguous share is
# 0.51 per 10 000 (mask 2 of 1079 x 1919: 106 pixels); the frames below 10 000 pixels have no ambiguous pixel at all.
SEEDS = {g: 11 for g in GEOMETRIES}
AMBIGUOUS_CAP = 1e-4  # at most 1 ambiguous pixel per 10 000, per mask


def bound64(geo, top):
    return 2.0 ** LOG2_BOUND64[geo] * top


def bound32(top):
    return 2.0 ** LOG2_BOUND32 * top


# ---------------------------------------------------------------------------------------------------------------- made masks
def made_low(kind, L=256):
    """empty: -10 everywhere; full: +10; border: -10 with a 3-pixel frame of +5.  The crop [:nh, :nw] removes the frame's bar
    along the shorter side's far edge, but the two bars across it run the whole length of the frame, so the box still touches
    all four edges of the output."""
    low = torch.full((1, L, L), 10.0 if kind == "full" else -10.0)
    if kind == "border":
        low[:, :3, :] = low[:, -3:, :] = 5.0
        low[:, :, :3] = low[:, :, -3:] = 5.0
    return low


def full_stats(h, w):
    return [h * w, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, 0, w - 1, h - 1]
