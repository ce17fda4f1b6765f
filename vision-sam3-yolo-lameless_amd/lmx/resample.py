"""Host-side tables for the preprocessing kernels.

``coeff_tables`` restates Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` (Pillow src/libImaging/Resample.c,
not in this tree; checked bit-for-bit against the installed Pillow in tests/test_resample.py) so the device kernels
(lmx_k_pil_resize_h/_v) reproduce ``PIL.Image.resize`` on uint8 exactly.  Used for
  * DINO: shortest-edge-256 BICUBIC (AutoImageProcessor, services/dinov3-pipeline/app/main.py:107)
  * SAM : ResizeLongestSide(1024) BILINEAR via torchvision ``resize(to_pil_image(..))`` (services/sam3-pipeline/app/main.py:80)

``aa_tables`` is the float counterpart for DINOv3ViTImageProcessor (a dinov3_vit directory's preprocessor_config.json): the
float32 weights of torch's antialiased ``F.interpolate`` in ATen's own arithmetic, same ``bounds`` layout, for
lmx_k_float_resize_patchify (checked against torch in tests/test_dino_float_resample.py).
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
BILINEAR, BICUBIC = "bilinear", "bicubic"


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def coeff_tables(in_size, out_size, filt):
    """-> (bounds int32 [out*2] = (xmin, count), kk int32 [out*ksize], ksize) for one axis (box = full input)."""
    fn, fsupport = _FILTERS[filt]
    in0, in1 = 0.0, float(in_size)
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        ww = 0.0
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        for x in range(xmax):
            w = fn((x + xmin - center + 0.5) * ss)
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            kk[xx, :xmax] /= ww
        bounds[xx] = (xmin, xmax)
    # normalize_coeffs_8bpc: (int)(+-0.5 + k * 2^22), C truncation toward zero
    scaled = kk * float(1 << PRECISION_BITS)
    ikk = np.where(kk < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)
    return bounds.reshape(-1), ikk.reshape(-1), ksize


def resize_u8_reference(img, dw, dh, filt):
    """numpy restatement of the two device passes (used by the CPU tests to pin the tables against PIL)."""
    h, w, _ = img.shape
    cur = img
    if dw != w:
        b, k, ks = coeff_tables(w, dw, filt)
        b = b.reshape(-1, 2)
        k = k.reshape(-1, ks)
        out = np.empty((h, dw, 3), np.uint8)
        for xo in range(dw):
            xmin, cnt = b[xo]
            acc = (cur[:, xmin:xmin + cnt, :].astype(np.int64) * k[xo, :cnt, None]).sum(1) + (1 << (PRECISION_BITS - 1))
            out[:, xo, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
        cur = out
    if dh != h:
        b, k, ks = coeff_tables(h, dh, filt)
        b = b.reshape(-1, 2)
        k = k.reshape(-1, ks)
        out = np.empty((dh, cur.shape[1], 3), np.uint8)
        for yo in range(dh):
            ymin, cnt = b[yo]
            acc = (cur[ymin:ymin + cnt].astype(np.int64) * k[yo, :cnt, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))
            out[yo] = np.clip(acc >> PRECISION_BITS, 0, 255)
        cur = out
    return cur


def _aa_filter_f32(filt):
    """ATen's antialias filters (aten/src/ATen/native/cpu/UpSampleKernel.cpp, not in this tree: HelperInterpLinear /
    HelperInterpCubic ::aa_filter with upsample_get_cubic_coefficients' two polynomials, A = -0.5), evaluated in float32 like
    ATen does for a float32 tensor.  Vectorised over the taps of one output index."""
    f = np.float32
    if filt == BILINEAR:
        def fn(x):
            x = np.abs(x)
            return np.where(x < f(1.0), f(1.0) - x, f(0.0)).astype(np.float32)
        return fn, 2
    a = -0.5

    def fma(p, q, r):
        # float32 fused multiply-add: the product of two float32 is exact in float64.  torch's CPU kernels are built with FMA
        # contraction, and only this form reproduces its bicubic weights bit for bit (the bilinear filter has no product to fuse)
        return (p.astype(np.float64) * q + r).astype(np.float32)

    def fn(x):
        x = np.abs(x).astype(np.float32)
        c1 = fma((fma(x, a + 2.0, -(a + 3.0)) * x).astype(np.float32), x, 1.0)
        c2 = fma(fma(fma(x, a, -5.0 * a), x, 8.0 * a), x, -4.0 * a)
        return np.where(x < f(1.0), c1, np.where(x < f(2.0), c2, f(0.0))).astype(np.float32)
    return fn, 4


def aa_tables(in_size, out_size, filt):
    """-> (bounds int32 [out*2] = (xmin, count), kk float32 [out*ksize], ksize) for one axis of torch's
    ``F.interpolate(x, size, mode=filt, antialias=True, align_corners=False)`` on a float32 CPU tensor (what torchvision's
    ``resize`` of a float tensor calls — the resize of DINOv3ViTImageProcessor).  Same layout as ``coeff_tables``; the weights are
    float32 and EVERY step is float32 in ATen's order (HelperInterpBase::_compute_indices_min_size_weights_aa): scale = in / out,
    support = (interp_size / 2) * max(scale, 1), center = scale * (i + 0.5), the int() truncations of center -+ support + 0.5,
    filter((j + xmin - center + 0.5) * invscale), weights divided by their float32 running sum.  Weights computed in float64 and
    rounded put the resized image 4e-6 .. 1.3e-5 off torch's; these are torch's own bits (tests/test_dino_float_resample.py)."""
    f = np.float32
    fn, interp_size = _aa_filter_f32(filt)
    scale = f(in_size) / f(out_size)
    support = f(interp_size * 0.5) * scale if scale >= f(1.0) else f(interp_size * 0.5)
    ksize = int(math.ceil(float(support))) * 2 + 1
    invscale = f(1.0) / scale if scale >= f(1.0) else f(1.0)
    kk = np.zeros((out_size, ksize), dtype=np.float32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        # the C++ literals 0.5 are doubles: `x + 0.5` promotes the float32 difference / sum, and the result is narrowed again
        center = f(float(scale) * (i + 0.5))
        xmin = max(int(float(f(center - support)) + 0.5), 0)
        xsize = min(max(min(int(float(f(center + support)) + 0.5), in_size) - xmin, 0), ksize)
        d = ((np.arange(xsize, dtype=np.int64) + xmin).astype(np.float32) - center).astype(np.float64)
        w = fn(((d + 0.5) * float(invscale)).astype(np.float32))
        total = f(0.0)
        for v in w:  # ATen's running float32 sum, tap by tap
            total = f(total + v)
        if total != f(0.0):
            w = (w / total).astype(np.float32)
        kk[i, :xsize] = w
        bounds[i] = (xmin, xsize)
    return bounds.reshape(-1), kk.reshape(-1), ksize


def segment_cols(bounds, tile=256):
    """The most source columns any run of `tile` consecutive outputs (starting at a multiple of `tile`) reads: the LDS segment
    lmx_k_float_resize_patchify stages per source row."""
    b = np.asarray(bounds).reshape(-1, 2)
    return max(int((b[i:i + tile, 0] + b[i:i + tile, 1]).max() - b[i:i + tile, 0].min()) for i in range(0, len(b), tile))


def resize_f32_reference(img, dw, dh, filt):
    """numpy restatement of the float device path on f32 [h, w, c]: width first, then height, f32 intermediate, taps
    accumulated in order with a fused multiply-add per tap (ATen's basic_loop_aa_horizontal / _vertical as an FMA build of
    torch compiles them; the device kernel uses fmaf).  The FMA is emulated through float64 (exact product, one extra
    rounding of the sum).  A size that does not change is not resampled."""
    h, w, _ = img.shape
    cur = np.ascontiguousarray(img, dtype=np.float32)
    for axis, (n_in, n_out) in ((1, (w, dw)), (0, (h, dh))):
        if n_in == n_out:
            continue
        b, k, ks = aa_tables(n_in, n_out, filt)
        b, k = b.reshape(-1, 2), k.reshape(-1, ks)
        src = np.moveaxis(cur, axis, 0)
        out = np.empty((n_out,) + src.shape[1:], np.float32)
        for o in range(n_out):
            lo, cnt = b[o]
            acc = src[lo] * k[o, 0]
            for j in range(1, cnt):
                acc = (src[lo + j].astype(np.float64) * np.float64(k[o, j]) + acc).astype(np.float32)
            out[o] = acc
        cur = np.ascontiguousarray(np.moveaxis(out, 0, axis))
    return cur


def shortest_edge_size(h, w, edge):
    """transformers get_resize_output_image_size(default_to_square=False): (new_h, new_w), int() truncation."""
    short, long = (w, h) if w <= h else (h, w)
    if short == edge:
        return h, w
    new_short, new_long = edge, int(edge * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def norm_lut(mean, std, rescale=1.0 / 255.0):
    """lut[c][u]: the image processor's rescale + normalize applied to byte u (same numpy expressions as
    transformers.image_transforms.rescale/normalize: f64 multiply -> f32, then (x - mean)/std in f32)."""
    u = np.arange(256, dtype=np.uint8)
    x = (u.astype(np.float64) * rescale).astype(np.float32)
    m = np.array(mean, dtype=np.float32)
    s = np.array(std, dtype=np.float32)
    return ((x[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
