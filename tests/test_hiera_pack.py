"""Host-side packing of the fused Hiera kernels' operands (lmx/sam.py pack_hiera_attn / pack_hiera_attn4 / pack_hiera_attn_pool /
pack_ln_mlp; csrc/hiera.hip): the images the kernels read, addressed exactly as the kernels address them, give back the
torch-layout weights.  CPU only (the kernels themselves: tests/test_gpu_kernels.py::test_hiera_attn*)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vision-sam3-yolo-lameless_amd"))


def _kslot_feature(pos):
    """MFMA k-slot order (csrc/hiera.hip): position 32 s + 8 g + 4 h + i holds feature 16 (2 s + h) + 4 g + i."""
    s, r = divmod(pos, 32)
    g, r = divmod(r, 8)
    h, i = divmod(r, 4)
    return 16 * (2 * s + h) + 4 * g + i


def _frag256(img, row, ks, fg):
    """The 8 halfs a lane (row, fg) reads for k-step ks from an image with 256-byte rows: chunk (4 ks + fg) ^ (row & 15)."""
    c = ((4 * ks + fg) ^ (row & 15))
    return img[row * 128 + c * 8: row * 128 + c * 8 + 8]


def _frag128(img, row, s, fg):
    """... from an image with 128-byte rows: chunk (4 s + fg) ^ ((row >> 1) & 7)."""
    c = ((4 * s + fg) ^ ((row >> 1) & 7))
    return img[row * 64 + c * 8: row * 64 + c * 8 + 8]


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_kslot_order_is_a_permutation():
    assert sorted(_kslot_feature(p) for p in range(128)) == list(range(128))
    assert [_kslot_feature(p) for p in (0, 1, 4, 8, 32)] == [0, 1, 16, 4, 32]


def test_pack_hiera_attn_stage1():
    from lmx import sam

    D, heads, hd = 112, 2, 56
    wqkv, bqkv, wo, bo = _rand((3 * D, D), 1), _rand((3 * D,), 2), _rand((D, D), 3), _rand((D,), 4)
    for ln_inside in (False, True):
        wq, bq, wop, bop = sam.pack_hiera_attn(wqkv, bqkv, wo, bo, heads, ln_inside=ln_inside)
        assert wq.shape == (384, 128) and wq.dtype == np.float16 and wop.shape == (D, 128) and bq.shape == (384,)
        for sec in range(3):
            for hh in range(heads):
                r0 = sec * 128 + hh * 64
                src = wqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd].astype(np.float16)
                cols = [_kslot_feature(p) for p in range(128)] if ln_inside else list(range(128))
                for p, f in enumerate(cols):  # column p of the packed rows holds input feature f (zeros past D)
                    want = src[:, f] if f < D else np.zeros(hd, np.float16)
                    assert np.array_equal(wq[r0:r0 + hd, p], want)
                assert not wq[r0 + hd:r0 + 64].any()  # padding rows (v's row 63 included: the bias carries the 1)
                assert np.array_equal(bq[r0:r0 + hd], bqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd])
                assert bq[r0 + 63] == (1.0 if sec == 2 else 0.0) and not bq[r0 + hd:r0 + 63].any()
        for hh in range(heads):
            for p in range(64):
                d = _kslot_feature(p)
                want = wo[:, hh * hd + d].astype(np.float16) if d < hd else np.zeros(D, np.float16)
                assert np.array_equal(wop[:, 64 * hh + p], want)
        assert np.array_equal(bop, bo)


def test_pack_hiera_attn4_images():
    from lmx import sam

    D, heads, hd = 224, 4, 56
    wqkv, bqkv, wo, bo = _rand((3 * D, D), 5), _rand((3 * D,), 6), _rand((D, D), 7), _rand((D,), 8)
    img, bias = sam.pack_hiera_attn4(wqkv, bqkv, wo, bo, heads)
    assert img.shape == (16, 16384) and img.dtype == np.float16 and bias.shape == (heads * 192 + D,)
    for hh in range(heads):
        for sec in range(3):
            src = wqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd].astype(np.float16)
            # rows of 512 bytes: chunk c of row r at c ^ (r & 15); the kernel reads chunk 4 ks + fg of k-step ks < 7
            for row in (0, 1, 17, 55, 56, 63):
                for ks in range(7):
                    for fg in range(4):
                        c = (4 * ks + fg) ^ (row & 15)
                        got = img[4 * hh + sec][row * 256 + c * 8: row * 256 + c * 8 + 8]
                        want = src[row, 32 * ks + 8 * fg: 32 * ks + 8 * fg + 8] if row < hd else np.zeros(8, np.float16)
                        assert np.array_equal(got, want)
            assert np.array_equal(bias[hh * 192 + sec * 64: hh * 192 + sec * 64 + hd], bqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd])
        assert bias[hh * 192 + 128 + 63] == 1.0
        for row in (0, 3, 100, 223, 224, 255):
            for s in range(2):
                for fg in range(4):
                    got = _frag128(img[4 * hh + 3], row, s, fg)
                    want = np.array([wo[row, hh * hd + _kslot_feature(32 * s + 8 * fg + j)] if row < D and _kslot_feature(32 * s + 8 * fg + j) < hd else 0.0
                                     for j in range(8)], np.float32).astype(np.float16)
                    assert np.array_equal(got, want)
    assert np.array_equal(bias[heads * 192:], bo)


def test_pack_hiera_attn_pool_images():
    from lmx import sam

    Din, D, heads, hd = 112, 224, 4, 56
    wsc, bsc = _rand((D, Din), 9), _rand((D,), 10)
    wqkv, bqkv, wo, bo = _rand((3 * D, Din), 11), _rand((3 * D,), 12), _rand((D, D), 13), _rand((D,), 14)
    img, bias = sam.pack_hiera_attn_pool(wsc, bsc, wqkv, bqkv, wo, bo, heads)
    assert img.shape == (14, 16384) and bias.shape == (2 * D + heads * 192,)
    assert np.array_equal(bias[:D], bsc + bo)  # the shortcut's and the output projection's biases enter the same accumulators

    def check256(image, row, src_row):
        for ks in range(4):
            for fg in range(4):
                lo = 32 * ks + 8 * fg
                want = np.zeros(8, np.float16)
                if src_row is not None and lo < Din:
                    want = src_row[lo:lo + 8].astype(np.float16)
                assert np.array_equal(_frag256(image, row, ks, fg), want)

    for r in (0, 5, 127):
        check256(img[0], r, wsc[r])
    for r in (0, 95):
        check256(img[1], r, wsc[128 + r])
    check256(img[1], 96, None)  # rows 224.. of the shortcut image do not exist
    for hh in range(heads):
        for sec in range(2):
            for r in (0, 31, 55):
                check256(img[2 + 3 * hh], sec * 64 + r, wqkv[sec * D + hh * hd + r])
            check256(img[2 + 3 * hh], sec * 64 + 60, None)
        for r in (0, 55):
            check256(img[3 + 3 * hh], r, wqkv[2 * D + hh * hd + r])
        check256(img[3 + 3 * hh], 63, None)
        assert bias[D + hh * 192 + 128 + 63] == 1.0
        for sec in range(3):
            assert np.array_equal(bias[D + hh * 192 + sec * 64: D + hh * 192 + sec * 64 + hd], bqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd])
        for row in (0, 111, 223, 230):
            for s in range(2):
                for fg in range(4):
                    want = np.array([wo[row, hh * hd + _kslot_feature(32 * s + 8 * fg + j)] if row < D and _kslot_feature(32 * s + 8 * fg + j) < hd else 0.0
                                     for j in range(8)], np.float32).astype(np.float16)
                    assert np.array_equal(_frag128(img[4 + 3 * hh], row, s, fg), want)


def _frag512(img, row, ks, fg):
    """... from an image with 512-byte rows: chunk (4 ks + fg) ^ (row & 15)."""
    c = ((4 * ks + fg) ^ (row & 15))
    return img[row * 256 + c * 8: row * 256 + c * 8 + 8]


def _kslot_frag(w_row, lo, width):
    """The 8 halfs at k-slot positions lo .. lo + 7 of a row whose features are w_row (zeros past `width`)."""
    return np.array([w_row[_kslot_feature(lo + j)] if _kslot_feature(lo + j) < width else 0.0 for j in range(8)], np.float32).astype(np.float16)


def test_pack_hiera_attn_pool_images_stage3():
    """224 -> 448, 8 heads: 47 images — the shortcut in 7 of 64 rows, then per head q, k, v and the projection's columns in two
    images (output rows 0..223, 224..447); rows of 512 bytes swizzled by r & 15."""
    from lmx import sam

    Din, D, heads, hd = 224, 448, 8, 56
    wsc, bsc = _rand((D, Din), 21), _rand((D,), 22)
    wqkv, bqkv, wo, bo = _rand((3 * D, Din), 23), _rand((3 * D,), 24), _rand((D, D), 25), _rand((D,), 26)
    img, bias = sam.pack_hiera_attn_pool(wsc, bsc, wqkv, bqkv, wo, bo, heads)
    assert img.shape == (47, 16384) and img.dtype == np.float16 and bias.shape == (D + heads * 192,) and bias.dtype == np.float32
    assert np.array_equal(bias[:D], bsc + bo)

    def check512(image, row, src_row):
        for ks in range(8):  # (the kernel reads k-steps 0 .. 6; the eighth is the row's zero padding)
            for fg in range(4):
                lo = 32 * ks + 8 * fg
                want = src_row[lo:lo + 8].astype(np.float16) if src_row is not None and lo < Din else np.zeros(8, np.float16)
                assert np.array_equal(_frag512(image, row, ks, fg), want)

    for j in range(7):
        for r in (0, 1, 17, 63):
            check512(img[j], r, wsc[64 * j + r])
    for hh in range(heads):
        for sec in range(3):
            for r in (0, 15, 16, 55):
                check512(img[7 + 5 * hh + sec], r, wqkv[sec * D + hh * hd + r])
            for r in (56, 63):
                check512(img[7 + 5 * hh + sec], r, None)
            lo = D + hh * 192 + sec * 64
            assert np.array_equal(bias[lo:lo + hd], bqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd])
            assert not bias[lo + hd:lo + 63].any() and bias[lo + 63] == (1.0 if sec == 2 else 0.0)
        for half in range(2):
            for row in (0, 3, 100, 223, 224, 255):
                for s in range(2):
                    for fg in range(4):
                        want = _kslot_frag(wo[224 * half + row, hh * hd:(hh + 1) * hd], 32 * s + 8 * fg, hd) if row < 224 else np.zeros(8, np.float16)
                        assert np.array_equal(_frag128(img[7 + 5 * hh + 3 + half], row, s, fg), want)


def _mlp_inputs(D, seed):
    return [_rand((4 * D, D), seed), _rand((4 * D,), seed + 1), _rand((D, 4 * D), seed + 2)] + [_rand((D,), seed + 3 + i) for i in range(5)]


def _check_mlp_bias(bias, D, b1, b2, g2, e2, gn, en):
    assert bias.shape == (9 * D,) and bias.dtype == np.float32
    for lo, want in ((0, b1), (4 * D, b2), (5 * D, g2), (6 * D, e2), (7 * D, gn), (8 * D, en)):  # [b1 | b2 | g2 | e2 | gn | en]
        assert np.array_equal(bias[lo:lo + len(want)], want)


def test_pack_ln_mlp_images_d112():
    """D = 112: 7 images, one per 64 hidden units — w1's 64 rows (256 bytes, inputs in k-slot order) and, from half 8192 on, w2's 112
    rows x 64 columns (128 bytes, columns in k-slot order)."""
    from lmx import sam

    D = 112
    w1, b1, w2, b2, g2, e2, gn, en = args = _mlp_inputs(D, 31)
    img, bias = sam.pack_ln_mlp(*args)
    assert img.shape == (7, 16384) and img.dtype == np.float16
    _check_mlp_bias(bias, D, b1, b2, g2, e2, gn, en)
    for ch in range(7):
        for row in (0, 1, 17, 63):
            for ks in range(4):
                for fg in range(4):
                    assert np.array_equal(_frag256(img[ch], row, ks, fg), _kslot_frag(w1[64 * ch + row], 32 * ks + 8 * fg, D))
        for row in (0, 3, 55, 111):
            for s in range(2):
                for fg in range(4):
                    assert np.array_equal(_frag128(img[ch][8192:], row, s, fg), _kslot_frag(w2[row, 64 * ch: 64 * ch + 64], 32 * s + 8 * fg, 64))
        assert not img[ch][8192 + D * 64:].any()
    img0, bias0 = sam.pack_ln_mlp(*args[:6])  # no next block: the same images, zeros for its LayerNorm vectors
    assert np.array_equal(img0, img)
    _check_mlp_bias(bias0, D, b1, b2, g2, e2, np.zeros(D, np.float32), np.zeros(D, np.float32))


def test_pack_ln_mlp_images_d224():
    """D = 224: 28 images, alternating — w1's 64 rows of 512 bytes, then w2's 224 rows x 64 columns of 128 bytes."""
    from lmx import sam

    D = 224
    w1, b1, w2, b2, g2, e2, gn, en = args = _mlp_inputs(D, 41)
    img, bias = sam.pack_ln_mlp(*args)
    assert img.shape == (28, 16384) and img.dtype == np.float16
    _check_mlp_bias(bias, D, b1, b2, g2, e2, gn, en)
    for ch in (0, 1, 6, 13):
        for row in (0, 1, 17, 63):
            for ks in range(8):
                for fg in range(4):
                    assert np.array_equal(_frag512(img[2 * ch], row, ks, fg), _kslot_frag(w1[64 * ch + row], 32 * ks + 8 * fg, D))
        for row in (0, 3, 100, 223):
            for s in range(2):
                for fg in range(4):
                    assert np.array_equal(_frag128(img[2 * ch + 1], row, s, fg), _kslot_frag(w2[row, 64 * ch: 64 * ch + 64], 32 * s + 8 * fg, 64))
        assert not img[2 * ch + 1][D * 64:].any()
    img0, bias0 = sam.pack_ln_mlp(*args[:6])
    assert np.array_equal(img0, img)
    _check_mlp_bias(bias0, D, b1, b2, g2, e2, np.zeros(D, np.float32), np.zeros(D, np.float32))


def test_packers_keep_every_byte():
    """SHA-256 (first 16 hex digits) over the returned arrays in order, each as str(dtype) + str(shape) + bytes: the digests of the
    packers as they were before they were rebuilt on shared pieces."""
    from lmx import sam

    def attn_in(Din, D, s):
        return _rand((3 * D, Din), s), _rand((3 * D,), s + 1), _rand((D, D), s + 2), _rand((D,), s + 3)

    def digest(arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update((str(a.dtype) + str(a.shape)).encode() + a.tobytes())
        return h.hexdigest()[:16]

    assert digest(sam.pack_hiera_attn(*attn_in(112, 112, 100), 2, ln_inside=False)) == "ec64e3283c18e807"
    assert digest(sam.pack_hiera_attn(*attn_in(112, 112, 100), 2, ln_inside=True)) == "c499eb892d00083d"
    assert digest(sam.pack_hiera_attn4(*attn_in(224, 224, 200), 4)) == "ee5edbe0902fefb0"
    assert digest(sam.pack_hiera_attn_pool(_rand((224, 112), 300), _rand((224,), 301), *attn_in(112, 224, 302), 4)) == "c241773efdf718d9"
    assert digest(sam.pack_hiera_attn_pool(_rand((448, 224), 400), _rand((448,), 401), *attn_in(224, 448, 402), 8)) == "9dfd2a7bd0669578"
    for D, s, with_next, without in ((112, 500, "707adae84420d3f0", "451c458082155ab3"), (224, 600, "21380b05096fc584", "54efae5bbe26724e")):
        args = _mlp_inputs(D, s)
        assert digest(sam.pack_ln_mlp(*args)) == with_next and digest(sam.pack_ln_mlp(*args[:6])) == without
