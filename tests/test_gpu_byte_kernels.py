"""The kernels that move bytes and integers around the three networks, on the smallest shapes at which each of their branches can
go wrong: the two Pillow resize passes (csrc/pre.hip), the patch matrix (csrc/sam.hip), the NMS candidate filter (csrc/nms.hip),
Detect's decode and the stem (csrc/yolo.hip).  Integer and copy kernels are compared bit for bit with a reference that is not the
code under test; the two float kernels are held to the float64 references of tests/rowref.py at their existing bounds."""
import numpy as np
import pytest
import torch
from PIL import Image

import rowref as RR
from lmx import resample as R
from oracle import nms as ONMS

pytestmark = pytest.mark.gpu

PIL_FILT = {R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC}
SENT = -1234.0


def _up(tab, dev):
    b, k, ks = tab
    return torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), ks


def _frames(n, h, w, seed):
    """Random bytes with runs of 0 and 255 (the clip at both ends of bicubic's overshoot)."""
    g = np.random.default_rng(seed)
    f = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if w >= 16:
        f[:, :, w // 3:w // 3 + 3] = 255
        f[:, :, w // 2:w // 2 + 3] = 0
    else:
        f[:, ::3, :, 0], f[:, 1::3, :, 1] = 255, 0
    return f


def _offset_view(frames, off, dev):
    """The frames as a contiguous device tensor whose first byte lies `off` bytes past a 256-byte aligned address."""
    flat = torch.zeros((frames.size + 16,), dtype=torch.uint8, device=dev)
    v = flat[off:off + frames.size].view(frames.shape)
    v.copy_(torch.from_numpy(frames))
    assert v.data_ptr() % 16 == off % 16 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------- resize, horizontal
H_CASES = [
    # n, sh, sw, dw: what the case is there for
    (1, 5, 53, 29),      # rows of 159 bytes (odd, no multiple of 16); a staging group of 5 rows = one task of 4 + a remainder of 1;
                         # output rows of 87 bytes: no multiple of 4, so most rows start off a dword
    (2, 9, 64, 40),      # two frames, 18 rows: groups of 8, 8 and 2 across the frame boundary
    (2, 9, 64, 100),     # upscale: 1-2 taps (bilinear)
    (1, 1, 64, 30),      # one source row
    (1, 3, 37, 7),       # the last thread task of a row holds 3 pixels
    (1, 6, 1400, 747),   # rows of 4200 bytes: 4 rows a group (as at 1080p), then a group of 2
    (1, 3, 4000, 101),   # rows of 12000 bytes: 2 rows a group, then 1
    (1, 2, 5461, 64),    # the widest row that is staged: 1 row a group
]


@pytest.mark.parametrize("filt", [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize("n,sh,sw,dw", H_CASES)
def test_resize_h(cuda, n, sh, sw, dw, filt):
    """Against lmx.resample.resize_u8_reference and Pillow's Image.resize, both swap_rb values, the source at 0, 1 and 3 bytes past
    an aligned address."""
    from lmx import kernels as K

    frames = _frames(n, sh, sw, sh * 1000 + sw)
    ref = np.stack([R.resize_u8_reference(f, dw, sh, filt) for f in frames], 0)
    pil = np.stack([np.asarray(Image.fromarray(f).resize((dw, sh), PIL_FILT[filt])) for f in frames], 0)
    assert np.array_equal(ref, pil), "the numpy reference and Pillow disagree"
    tab = _up(R.coeff_tables(sw, dw, filt), cuda)
    for off in (0, 1, 3):
        src = _offset_view(frames, off, cuda)
        for swap in (False, True):
            got = K.pil_resize(src, dw, sh, tab, None, swap_rb=swap).cpu().numpy()
            want = ref[..., ::-1] if swap else ref
            assert got.shape == want.shape and np.array_equal(got, want), f"h {(n, sh, sw, dw)} {filt} offset {off} swap_rb {swap}"


def test_resize_h_rejects_rows_wider_than_the_staging_limit(cuda):
    from lmx import kernels as K

    frames = _frames(1, 1, 5462, 1)
    with pytest.raises(Exception, match="wider than"):
        K.pil_resize(torch.from_numpy(frames).to(cuda), 16, 1, _up(R.coeff_tables(5462, 16, R.BILINEAR), cuda), None)


# ------------------------------------------------------------------------------------------- resize, vertical
@pytest.mark.parametrize("filt", [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize("sh,dh", [(21, 8), (8, 21)])
@pytest.mark.parametrize("w,off,form", [(16, 0, "16 bytes"), (48, 0, "16 bytes"), (4, 0, "dword"), (16, 4, "dword"), (5, 0, "neither"),
                                        (16, 1, "neither"), (455, 3, "neither"), (2, 0, "neither"), (1, 0, "byte"), (1, 1, "byte")])
def test_resize_v(cuda, w, off, form, sh, dh, filt):
    """Row lengths and base addresses of each kind: a multiple of 16 bytes (16 bytes per thread and tap row), of 4 bytes only, and
    neither (both a dword per thread at the bytes' own address; rows of 15, 6 and 1365 bytes end in a piece moved back into its
    neighbour), and rows shorter than a dword (a byte per thread).  Many taps (21 -> 8) and 1-2 (8 -> 21), two frames."""
    from lmx import kernels as K

    assert {"16 bytes": (w * 3) % 16 == 0 and off % 16 == 0, "dword": (w * 3) % 4 == 0 and off % 4 == 0 and ((w * 3) % 16 or off % 16),
            "neither": w * 3 >= 4 and bool((w * 3) % 4 or off % 4), "byte": w * 3 < 4}[form]
    frames = _frames(2, sh, w, sh * 100 + w)
    ref = np.stack([R.resize_u8_reference(f, w, dh, filt) for f in frames], 0)
    pil = np.stack([np.asarray(Image.fromarray(f).resize((w, dh), PIL_FILT[filt])) for f in frames], 0)
    assert np.array_equal(ref, pil), "the numpy reference and Pillow disagree"
    got = K.pil_resize(_offset_view(frames, off, cuda), w, dh, None, _up(R.coeff_tables(sh, dh, filt), cuda)).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref), f"v {form}: w {w} offset {off} {sh} -> {dh} {filt}"


def test_resize_both_passes(cuda):
    """The two passes chained as lmx/sam.py chains them (the vertical pass reads the horizontal pass's output)."""
    from lmx import kernels as K

    frames = _frames(2, 27, 48, 9)
    ref = np.stack([R.resize_u8_reference(f, 32, 15, R.BILINEAR) for f in frames], 0)
    got = K.pil_resize(torch.from_numpy(frames).to(cuda), 32, 15, _up(R.coeff_tables(48, 32, R.BILINEAR), cuda),
                       _up(R.coeff_tables(27, 15, R.BILINEAR), cuda)).cpu().numpy()
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------- im2col
def _im2col_ref(img, lut, IH, IW, KH, KW, stride, pad, ldo):
    """numpy gather: lut[c, byte] inside the rh x rw image, zeros on the rest of the IH x IW canvas and its padding, zero columns
    from K to ldo."""
    n, rh, rw, _ = img.shape
    canvas = np.zeros((n, IH + 2 * pad, IW + 2 * pad, 3), np.float16)
    for c in range(3):
        canvas[:, pad:pad + rh, pad:pad + rw, c] = lut[c][img[..., c]].astype(np.float16)
    OH, OW = (IH + 2 * pad - KH) // stride + 1, (IW + 2 * pad - KW) // stride + 1
    out = np.zeros((n, OH, OW, ldo), np.float16)
    for ky in range(KH):
        for kx in range(KW):
            k = (ky * KW + kx) * 3
            out[..., k:k + 3] = canvas[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride]
    return out.reshape(n * OH * OW, ldo)


IM2COL_CASES = [
    # n, rh, rw, IH, IW, KH, KW, stride, pad, ldo
    (1, 17, 23, 32, 32, 7, 7, 4, 3, 152),    # the image ends inside a token's window; token rows 5-7 are padding; 8 tokens a row
    (1, 8, 290, 8, 300, 7, 7, 4, 3, 152),    # the band form (IH < IW): 75 tokens a row = a run of 64 and one of 11
    (1, 32, 32, 32, 32, 7, 7, 4, 3, 152),    # an image equal to the canvas
    (2, 19, 261, 24, 264, 7, 7, 4, 3, 152),  # two frames, rows of 783 bytes (every dword misalignment), the second run ends in the image
    (1, 9, 3, 12, 512, 7, 7, 4, 3, 160),     # an image narrower than one window; whole runs of padding; ldo with an all-zero chunk
    (2, 20, 40, 32, 48, 16, 16, 16, 0, 768),
    (1, 20, 40, 32, 48, 16, 16, 16, 0, 776),
    (2, 11, 13, 16, 16, 5, 5, 2, 1, 80),
    (1, 11, 13, 16, 16, 7, 7, 2, 3, 152),    # 7 x 7 at another stride: the generic form
]


@pytest.mark.parametrize("n,rh,rw,IH,IW,KH,KW,stride,pad,ldo", IM2COL_CASES)
def test_im2col(cuda, n, rh, rw, IH, IW, KH, KW, stride, pad, ldo):
    from lmx import kernels as K

    img = np.random.default_rng(rh * 100 + rw).integers(0, 256, (n, rh, rw, 3), dtype=np.uint8)
    lut = R.norm_lut(R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert not (lut.astype(np.float16) == 0).any()  # a value taken from the image is never the zero of the padding
    for off in (0, 1):
        got = K.im2col_u8(_offset_view(img, off, cuda), torch.from_numpy(lut).to(cuda), IH, IW, KH, KW, stride, pad, ldo).cpu().numpy()
        ref = _im2col_ref(img, lut, IH, IW, KH, KW, stride, pad, ldo)
        assert got.shape == ref.shape and np.array_equal(got, ref), f"im2col {(n, rh, rw, IH, IW, KH, KW, stride, pad, ldo)} offset {off}"


# ------------------------------------------------------------------------------------------- NMS candidate filter
def _nms_pred(n, A, nc, conf, seed):
    """Boxes on a 24-pixel grid, every fifth the copy of its neighbour (suppressed when the classes agree).  The best score of a
    row is uniform in (0.05, 0.95) in a random class, the others below it.  Rows 0-3 of every image: the maximum in the first
    class, in the last class, twice (first and last class), and exactly equal to conf."""
    g = np.random.default_rng(seed)
    pred = np.zeros((n, A, 4 + nc), np.float32)
    a = np.arange(A)
    a = np.where(a % 5 == 4, a - 1, a)
    pred[..., 0] = 12 + 24 * (a % 40)
    pred[..., 1] = 12 + 24 * (a // 40)
    pred[..., 2:4] = g.uniform(8, 20, (n, A, 2))
    best = g.uniform(0.05, 0.95, (n, A)).astype(np.float32)
    arg = g.integers(0, nc, (n, A))
    sc = (best[..., None] * g.uniform(0, 0.9, (n, A, nc))).astype(np.float32)
    np.put_along_axis(sc, arg[..., None], best[..., None], 2)
    top = np.float32(0.97)
    for row, cols in ((0, (0,)), (1, (nc - 1,)), (2, (0, nc - 1)), (3, (nc // 2,))):
        if row < A:
            v = np.float32(conf) if row == 3 else top
            sc[:, row] = np.minimum(sc[:, row], np.float32(0.5) * v) if v > 0 else 0
            for c in cols:
                sc[:, row, c] = v
    pred[..., 4:] = sc
    return pred


@pytest.mark.parametrize("nc", [1, 2, 17, 80, 4, 300])
def test_nms_filter(cuda, nc):
    """Through lmx.kernels.nms against oracle.nms.non_max_suppression on the same pred: boxes, scores, classes, src and counts.
    nc 80: 16-byte loads, 21 lanes a row; nc 4: the same with 2 lanes a row; nc 300: rows of 76 pieces, more than a wave; nc 1 / 2 /
    17: row lengths that are no multiple of four floats, dword loads.  A around the 64 lanes of a wave; one and three images (a wave
    then holds rows of several images); conf that no anchor, about half of them and every anchor passes."""
    from lmx import kernels as K

    for A in (1, 63, 64, 65, 1000):
        for n in (1, 3):
            for conf, what in ((2.0, "none"), (0.5, "half"), (0.01, "all")):
                pred = _nms_pred(n, A, nc, conf, A * 10 + n)
                best = pred[..., 4:].max(-1)
                passing = (best > np.float32(conf)).sum(1)
                if what == "none":
                    assert (passing == 0).all()
                elif what == "all":
                    assert (passing == A - (A > 3)).all()  # row 3 equals conf and stays out
                elif A >= 63:
                    assert (passing > A // 4).all() and (passing < 3 * A // 4).all()
                out = K.nms(torch.from_numpy(pred).to(cuda), conf, 0.7, A)
                b, s, c, src, cnt = (t.cpu().numpy() for t in out)
                for i in range(n):
                    rb, rs, rc, rsrc = ONMS.non_max_suppression(pred[i], conf, max_det=A)
                    k = len(rsrc)
                    tag = f"nc {nc} A {A} n {n} conf {conf} image {i}"
                    assert cnt[i] == k, f"{tag}: count {cnt[i]} != {k}"
                    assert np.array_equal(src[i, :k], rsrc) and (src[i, k:] == -1).all(), f"{tag}: src"
                    assert np.array_equal(c[i, :k], rc), f"{tag}: classes"
                    assert np.array_equal(s[i, :k], rs) and np.array_equal(b[i, :k], rb), f"{tag}: scores / boxes"
                    assert 3 not in rsrc.tolist(), f"{tag}: a score equal to conf passed"
                    if what != "none" and A > 2:
                        assert {0, 1, 2} <= set(rsrc.tolist()) and rc[rsrc == 2][0] == 0, f"{tag}: rows 0-2"


# ------------------------------------------------------------------------------------------- Detect decode
@pytest.mark.parametrize("guard", [64, 63])
@pytest.mark.parametrize("nc,ldh", [(1, 68), (80, 144), (17, 84), (8, 80), (83, 148)])
def test_detect_decode_rows(cuda, nc, ldh, guard):
    """Grids of 3 x 5 and 1 x 1 in one pred of two images, between rows that must stay untouched.  nc 80 / 8: rows of whole 16-byte
    pieces (aligned with guard 64, 4 bytes off with guard 63); nc 1 / 17 / 83: row lengths that are no multiple of four floats, so
    the rows start at every dword offset, and 1 or 3 scores are left after the pieces."""
    from lmx import kernels as K

    n, gap = 2, 3
    levels = [(3, 5, 8.0, 31), (1, 1, 32.0, 32)]
    A = gap + sum(h * w + gap for h, w, _, _ in levels)
    tot = n * A * (4 + nc)
    buf = torch.full((tot + 2 * guard,), SENT, dtype=torch.float32, device=cuda)
    pred = buf[guard:guard + tot].view(n, A, 4 + nc)
    assert pred.data_ptr() % 16 == (0 if guard == 64 else 12)
    ok = torch.zeros((n, A, 4 + nc), dtype=torch.bool)
    a_off = gap
    for H, W, stride, seed in levels:
        head = RR.detect_inputs(n, H, W, nc, ldh, 3.0, seed + nc)
        ref, bound = RR.detect_decode(head, nc, stride)
        K.detect_decode(head.to(cuda), pred, nc, stride, a_off)
        got = pred[:, a_off:a_off + H * W].cpu()
        rb = RR.ratio(got[..., :4], ref[..., :4], bound[..., :4])
        rs = RR.ratio(got[..., 4:], ref[..., 4:], bound[..., 4:])
        print(f"detect_decode nc {nc} {H} x {W} guard {guard}: boxes {rb:.3f}, scores {rs:.3f} x the bound")
        assert rb <= 1.0 and rs <= 1.0, f"detect_decode nc {nc} {H} x {W}: boxes {rb:.2f}, scores {rs:.2f} x the bound"
        ok[:, a_off:a_off + H * W] = True
        a_off += H * W + gap
    assert bool((pred.cpu()[~ok] == SENT).all()), f"detect_decode nc {nc}: rows outside the levels written"
    assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all())


# ------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("H,W", [(7, 5), (65, 97)])
@pytest.mark.parametrize("Cout", [8, 16, 64])
def test_stem_conv_odd_sizes(cuda, Cout, H, W):
    """Odd sizes (the right and bottom taps fall outside the frame), two images, one to eight 8-channel groups."""
    from lmx import kernels as K

    n = 2
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img, w, b = RR.stem_inputs(n, H, W, Cout, 17)
    ref, rnd, e = RR.stem_conv(img, w, b)
    tot, guard = n * Ho * Wo * Cout, 64
    buf = torch.full((tot + 2 * guard,), SENT, dtype=torch.float16, device=cuda)
    out = buf[guard:guard + tot].view(n, Ho, Wo, Cout)
    K.stem_conv(img.to(cuda), w.to(cuda), b.to(cuda), out=out)
    r = RR.ratio(out.cpu(), ref, rnd + e)
    print(f"stem_conv {(n, H, W, Cout)}: {r:.3f} x the bound")
    assert r <= 1.0, f"stem_conv {(n, H, W, Cout)}: {r:.2f} x the bound"
    assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all())
