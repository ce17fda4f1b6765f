"""The HBM-bound kernels of csrc/norm.hip and the YOLO glue of csrc/yolo.hip against the float64 references of tests/rowref.py,
each under its per-element bound (tests/test_row_ref_host.py shows the bounds have teeth), on every branch of their launchers:
the narrow, one-row (ITERS 2 / 4 / 16) and several-rows-per-wave LayerNorm kernels in every dtype pair, with and without GELU
and row strides; the second trip of every grid-stride loop (more than 2048 x 256 work items); odd and tiny shapes.  Every output
lies inside a larger buffer filled with a sentinel, and the guard rows and columns must come back untouched."""
import ctypes as C
import functools

import pytest
import torch

import rowref as R

pytestmark = pytest.mark.gpu

SENT = -1234.0  # exact in f16 and f32; no reference value comes near it
ROWS = 37       # not a multiple of the 4 (one-row kernel) or 8 (narrow kernel) rows of a workgroup
LN_CLASSES = {"narrow": (4, 112, 124, 128), "iters2": (132, 224, 448, 512), "iters4": (516, 768, 1024), "iters16": (1028, 1280, 4096)}
DT = {"f32": torch.float32, "f16": torch.float16}
GRID_CAP = 2048 * 256  # grid_for(): launches above this many work items take a second trip of the grid-stride loop


def _guarded(rows, cols, dtype, dev, ld=None, guard_rows=2):
    """(buffer, view): a [rows, cols] view with row stride ld inside a sentinel-filled buffer with guard rows on both sides."""
    ld = ld or cols
    buf = torch.full((rows + 2 * guard_rows, ld), SENT, dtype=dtype, device=dev)
    return buf, buf[guard_rows:guard_rows + rows, :cols]


def _guards_intact(buf, view):
    saved = view.clone()
    view.fill_(SENT)
    ok = bool((buf == SENT).all())
    view.copy_(saved)
    return ok


@functools.lru_cache(maxsize=None)
def _ln_case(rows, D, kind, in_dt, act):
    """(x as the kernel reads it (CPU), gamma, beta, eps, ref, aux), shared by the output dtypes and strides."""
    g, b = R.affine(D, 3)
    x = R.stress_rows(kind, rows, D, 5).to(DT[in_dt])
    eps = 1e-6 if act else 1e-5  # LayerNorm2d + GELU of the SAM neck uses 1e-6
    ref, aux = R.layernorm(x.double(), g, b, eps, act)
    return x, g, b, eps, ref, aux


def _run_ln(cuda, rows, D, kind, in_dt, out_dt, act, strided=False):
    from lmx import kernels as K

    x, g, b, eps, ref, aux = _ln_case(rows, D, kind, in_dt, act)
    xbuf, xv = _guarded(rows, D, DT[in_dt], cuda, D + 8 if strided else D)
    xv.copy_(x)
    ybuf, yv = _guarded(rows, D, DT[out_dt], cuda, D + 12 if strided else D)
    K.layernorm(xv, g.to(cuda), b.to(cuda), eps, out=yv, act=K.ACT_GELU if act else K.ACT_NONE)
    got = yv.cpu()
    f16 = out_dt == "f16"
    r = R.ratio(got, ref, R.ln_bound(ref, aux, act, f16))
    assert r <= 1.0, f"layernorm rows={rows} D={D} {kind} {in_dt}->{out_dt} act={act} strided={strided}: {r:.2f} x the bound"
    assert _guards_intact(ybuf, yv), f"layernorm D={D} {in_dt}->{out_dt}: wrote outside its rows / columns"
    return R.ln_unit_ratio(got, ref, aux, act, f16)


@pytest.mark.parametrize("out_dt", DT)
@pytest.mark.parametrize("in_dt", DT)
@pytest.mark.parametrize("cls", LN_CLASSES)
def test_layernorm_branch(cuda, cls, in_dt, out_dt):
    widths = LN_CLASSES[cls]
    worst = 0.0
    for D in widths:
        for act in (False, True):
            for kind in R.STRESSES:
                worst = max(worst, _run_ln(cuda, ROWS, D, kind, in_dt, out_dt, act))
    for act in (False, True):  # column slices of wider buffers; one row
        worst = max(worst, _run_ln(cuda, ROWS, widths[1], "mixed", in_dt, out_dt, act, strided=True))
        worst = max(worst, _run_ln(cuda, 1, widths[-1], "bigmean", in_dt, out_dt, act, strided=True))
    print(f"layernorm {cls} {in_dt}->{out_dt}: GPU ratio {R.fmt(worst)} of the unit bound (C_LN {R.C_LN})")


# ---- the several-rows-per-wave kernel: rows >= 16384, f32 -> f16, no activation, D <= 1024
@functools.lru_cache(maxsize=None)
def _rows_input(rows, D):
    g, b = R.affine(D, 3)
    return R.stress_rows("mixed", rows, D, 8).float(), g, b


def _rows_launch(cuda, x, g, b, ldx=None, ldy=None):
    from lmx import kernels as K

    rows, D = x.shape
    xbuf, xv = _guarded(rows, D, torch.float32, cuda, ldx)
    xv.copy_(x)
    ybuf, yv = _guarded(rows, D, torch.float16, cuda, ldy)
    K.layernorm(xv, g.to(cuda), b.to(cuda), 1e-5, out=yv)
    assert _guards_intact(ybuf, yv), f"layernorm rows={rows} D={D}: wrote outside its rows / columns"
    return yv.cpu()


@pytest.mark.parametrize("rows,D,strided", [(16384, 132, False), (16385, 516, True), (24581, 448, False), (24581, 1024, False)])
def test_layernorm_rows_kernel(cuda, rows, D, strided):
    """24581 = 3 * 8192 + 5: five waves walk four rows, the others three, so the prefetch of row r + 8192 is skipped at different
    trips.  Every row is compared in float64."""
    x, g, b = _rows_input(rows, D)
    got = _rows_launch(cuda, x, g, b, *((D + 8, D + 12) if strided else ()))
    worst = 0.0
    for r0 in range(0, rows, 4096):
        sl = slice(r0, min(rows, r0 + 4096))
        ref, aux = R.layernorm(x[sl].double(), g, b, 1e-5)
        r = R.ratio(got[sl], ref, R.ln_bound(ref, aux, False, True))
        assert r <= 1.0, f"layernorm_rows rows={rows} D={D} rows {r0}..: {r:.2f} x the bound"
        worst = max(worst, R.ln_unit_ratio(got[sl], ref, aux, False, True))
    print(f"layernorm rows kernel {rows} x {D}: GPU ratio {R.fmt(worst)} of the unit bound (C_LN {R.C_LN})")


@pytest.mark.parametrize("D", (448, 1024))
def test_layernorm_bits_do_not_depend_on_the_row_count(cuda, D):
    """The launcher switches kernels on rows = frames x tokens, so on the batch: the first 16383 rows of a 24581-row launch
    (several rows per wave) must equal, bit for bit, a 16383-row launch on the same rows (one row per wave)."""
    x, g, b = _rows_input(24581, D)
    many = _rows_launch(cuda, x, g, b)
    few = _rows_launch(cuda, x[:16383], g, b)
    diff = int((many[:16383] != few).sum())
    assert torch.equal(many[:16383], few), f"D={D}: {diff} outputs differ across the 16384-row switch"


# ---- tokens
def _raw(name):
    from lmx import _lib

    return getattr(_lib.load(), name)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("in_dt", DT)
@pytest.mark.parametrize("B,T,D", [(3, 201, 1024), (2, 7, 260), (1, 1, 4)])
def test_token_mean(cuda, B, T, D, in_dt):
    from lmx import _lib
    from lmx import kernels as K

    worst = 0.0
    for kind in R.STRESSES:
        x = R.stress_rows(kind, B * T, D, 7).to(DT[in_dt])
        ref, bound = R.token_mean(x.double(), B, T, D)
        d_x = x.to(cuda)
        obuf, ov = _guarded(B, D, torch.float32, cuda)
        _lib.check(_raw("lmx_k_token_mean")(d_x.data_ptr(), K._DT[x.dtype], ov.data_ptr(), B, T, D, _stream(cuda)), "lmx_k_token_mean")
        r = R.ratio(ov.cpu(), ref, bound)
        assert r <= 1.0, f"token_mean {(B, T, D)} {kind} {in_dt}: {r:.2f} x the bound"
        assert _guards_intact(obuf, ov) and torch.equal(K.token_mean(d_x, B, T, D), ov)
        worst = max(worst, r)
    print(f"token_mean {(B, T, D)} {in_dt}: GPU ratio {R.fmt(worst)} of the bound")


@pytest.mark.parametrize("B,np_,n_prefix,D", [(3, 10, 2, 64), (2, 196, 0, 384), (11, 196, 5, 1024)])
def test_assemble_tokens(cuda, B, np_, n_prefix, D):
    """(11, 196, 5, 1024) has 565 k float4 work items: the grid-stride trip.  lmx.kernels.assemble_tokens admits pos = None (and
    prefix = None without prefix tokens); the guarded launches go to the C entry, which takes the output pointer."""
    from lmx import _lib
    from lmx import kernels as K

    T = np_ + n_prefix
    assert (B * T * (D // 4) > GRID_CAP) == (B == 11)
    g = R._rng(13)
    patch, prefix, pos = (3 * R._rn(g, B * np_, D)).half(), R._rn(g, max(n_prefix, 1), D).float(), R._rn(g, T, D).float()
    d_patch, d_prefix, d_pos = patch.to(cuda), prefix.to(cuda) if n_prefix else None, pos.to(cuda)
    for use_pos in (True, False):
        ref = R.assemble_tokens(patch, prefix, pos if use_pos else None, B, np_, n_prefix, D)
        obuf, ov = _guarded(B * T, D, torch.float32, cuda)
        ptr = [t.data_ptr() if t is not None else None for t in (d_patch, d_prefix, d_pos if use_pos else None)]
        _lib.check(_raw("lmx_k_assemble_tokens")(*ptr, ov.data_ptr(), B, np_, n_prefix, D, _stream(cuda)), "lmx_k_assemble_tokens")
        assert torch.equal(ov.cpu(), ref), f"assemble_tokens {(B, np_, n_prefix, D)} pos={use_pos}"
        assert _guards_intact(obuf, ov)
        assert torch.equal(K.assemble_tokens(d_patch, d_prefix, d_pos if use_pos else None, B, np_, n_prefix, D), ov)


@pytest.mark.parametrize("B,T,H,hd,n_prefix", [(2, 14, 3, 64, 5), (2, 10, 3, 64, 0), (3, 10, 2, 80, 1), (2, 9, 3, 80, 0),
                                               (2, 14, 2, 96, 5), (1, 12, 3, 96, 1), (8, 1025, 16, 64, 1)])
def test_rope(cuda, B, T, H, hd, n_prefix):
    """On the q and the k slice of a [B T, 3 H hd] buffer inside a wider one; v, the prefix tokens and the guards keep their bits.
    (8, 1025, 16, 64) has 1 048 576 work items: the grid-stride trips."""
    from lmx import kernels as K

    assert (B * (T - n_prefix) * H * hd // 8 > GRID_CAP) == (B == 8)
    D = H * hd
    qkv, cos_t, sin_t = R.rope_inputs(B, T, H, hd, n_prefix, 9)
    buf, view = _guarded(B * T, 3 * D, torch.float16, cuda, 3 * D + 8)
    view.copy_(qkv)
    d_cos, d_sin = cos_t.to(cuda), sin_t.to(cuda)
    for part in (0, 1):
        K.rope(view[:, part * D:(part + 1) * D], B, T, H, hd, n_prefix, d_cos, d_sin)
    got = view.cpu()
    worst = 0.0
    for part in (0, 1):
        x, o = qkv[:, part * D:(part + 1) * D], got[:, part * D:(part + 1) * D]
        ref, rnd, e = R.rope(x, B, T, H, hd, n_prefix, cos_t, sin_t)
        r = R.ratio(o, ref, rnd + e)
        assert r <= 1.0, f"rope {(B, T, H, hd, n_prefix)} part {part}: {r:.2f} x the bound"
        assert torch.equal(o.view(B, T, D)[:, :n_prefix], x.view(B, T, D)[:, :n_prefix]), "prefix tokens rotated"
        worst = max(worst, R.excess(o, ref, rnd, e))
    assert torch.equal(got[:, 2 * D:], qkv[:, 2 * D:]), "rope touched the v slice"
    assert _guards_intact(buf, view)
    print(f"rope {(B, T, H, hd, n_prefix)}: GPU ratio {R.fmt(worst)} of the float32 part of the bound")


# ---- YOLO glue
def _flat_guarded(shape, dtype, dev, guard=64):
    """A dense tensor of `shape` inside a flat sentinel-filled buffer with `guard` elements on both sides."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), SENT, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n].view(shape)


@pytest.mark.parametrize("n,H,W,Cout", [(2, 64, 96, 16), (1, 65, 97, 8), (1, 7, 5, 64), (3, 864, 1024, 16)])
def test_stem_conv(cuda, n, H, W, Cout):
    """Odd H / W put the bottom / right taps outside the frame; 7 x 5 is all border; 3 x 432 x 512 outputs are 663 k work items:
    the grid-stride trip."""
    from lmx import kernels as K

    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert (n * Ho * Wo > GRID_CAP) == (n == 3)
    img, w, b = R.stem_inputs(n, H, W, Cout, 11)
    ref, rnd, e = R.stem_conv(img, w, b)
    obuf, ov = _flat_guarded((n, Ho, Wo, Cout), torch.float16, cuda)
    K.stem_conv(img.to(cuda), w.to(cuda), b.to(cuda), out=ov)
    got = ov.cpu()
    r = R.ratio(got, ref, rnd + e)
    assert r <= 1.0, f"stem_conv {(n, H, W, Cout)}: {r:.2f} x the bound"
    assert _guards_intact(obuf, ov)
    print(f"stem_conv {(n, H, W, Cout)}: GPU ratio {R.fmt(R.excess(got, ref, rnd, e))} of the float32 part of the bound")


@pytest.mark.parametrize("n,H,W,C", [(2, 20, 12, 16), (1, 3, 4, 8), (1, 1, 1, 8), (2, 80, 80, 512)])
def test_maxpool5_upsample2(cuda, n, H, W, C):
    """Channel slices of wider buffers, bit for bit; grids smaller than the 5 x 5 window; (2, 80, 80, 512) is 819 k (pool) and
    3.3 M (upsample) work items: the grid-stride trips."""
    from lmx import kernels as K

    assert (n * H * W * C // 8 > GRID_CAP) == (C == 512)
    x = R.pool_inputs(n, H, W, C, 4)
    src = torch.full((n, H, W, C + 16), SENT, dtype=torch.float16, device=cuda)
    src[..., 8:8 + C] = x.to(cuda)
    dst = torch.full((n + 2, H, W, C + 8), SENT, dtype=torch.float16, device=cuda)
    pv = dst[1:n + 1, :, :, :C]
    K.maxpool5(src[..., 8:8 + C], pv)
    pooled = R.maxpool5(x)
    assert torch.equal(pv.cpu(), pooled), f"maxpool5 {(n, H, W, C)}"
    assert _guards_intact(dst, pv) and torch.equal(src[..., 8:8 + C].cpu(), x)
    up = torch.full((n + 2, 2 * H, 2 * W, C + 24), SENT, dtype=torch.float16, device=cuda)
    uv = up[1:n + 1, :, :, 16:16 + C]
    K.upsample2(pv, uv)
    assert torch.equal(uv.cpu(), R.upsample2(pooled)), f"upsample2 {(n, H, W, C)}"
    assert _guards_intact(up, uv)


def test_detect_decode(cuda):
    """Every level of R.DETECT_CASES: nc 80 / 3 / 1 (nc % 4 != 0: some of an anchor's four lanes have no class left), head rows
    wider than 64 + nc, logits scaled up to one dominant bin and to exp underflow; the 21-frame levels are 537 600 and 530 880
    lanes (the grid-stride trip, with and without dead lanes in it).  Levels of one (n, nc) share one pred: the rows before, between
    and after them must stay untouched."""
    from lmx import kernels as K

    box = sig = 0.0
    preds = {}  # levels of one (n, nc) go into one pred
    for i, case in enumerate(R.DETECT_CASES):
        preds.setdefault((case[0], case[3]), []).append((i, case))
    assert max(len(c) for c in preds.values()) == 2
    for (n, nc), cases in preds.items():
        gap = 3
        A = gap + sum(c[1] * c[2] + gap for _, c in cases)
        pbuf, pred = _flat_guarded((n, A, 4 + nc), torch.float32, cuda)
        ok = torch.zeros((n, A, 4 + nc), dtype=torch.bool)
        a_off = gap
        for i, (n_, H, W, nc_, ldh, scale) in cases:
            assert (n * H * W * 4 > GRID_CAP) == (n == 21)
            stride = 8.0 * 2 ** (i % 3)
            head = R.detect_inputs(n, H, W, nc, ldh, scale, 20 + i)
            ref, bound = R.detect_decode(head, nc, stride)
            K.detect_decode(head.to(cuda), pred, nc, stride, a_off)
            got = pred[:, a_off:a_off + H * W].cpu()
            rb = R.ratio(got[..., :4], ref[..., :4], bound[..., :4])
            rs = R.ratio(got[..., 4:], ref[..., 4:], bound[..., 4:])
            assert rb <= 1.0 and rs <= 1.0, f"detect_decode {(n, H, W, nc, ldh, scale)}: boxes {rb:.2f}, scores {rs:.2f} x the bound"
            box, sig = max(box, rb * R.K_BOX), max(sig, rs * R.K_SIG)
            ok[:, a_off:a_off + H * W] = True
            a_off += H * W + gap
        assert bool((pred.cpu()[~ok] == SENT).all()), f"detect_decode nc={nc}: rows outside the levels written"
        assert bool((pbuf[:64] == SENT).all()) and bool((pbuf[-64:] == SENT).all())
    print(f"detect_decode: GPU ratio boxes {R.fmt(box)} (K_BOX {R.K_BOX}), scores {R.fmt(sig)} (K_SIG {R.K_SIG})")


@pytest.mark.parametrize("total", (1, 255, 257, 1000))
def test_scale_boxes(cuda, total):
    from lmx import kernels as K

    padx, pady, gain, w, h = 0.0, 140.0, 1 / 3, 1920.0, 1080.0  # a 1080p frame letterboxed to 640
    boxes = R.box_inputs(total, 30 + total, padx, pady, gain, w, h)
    r64, r32 = R.scale_boxes(boxes, padx, pady, gain, w, h)
    buf, view = _flat_guarded((total, 4), torch.float32, cuda)
    view.copy_(boxes)
    K.scale_boxes(view, padx, pady, gain, w, h)
    got = view.cpu()
    ulps = R.ulps32(got, r64)
    print(f"scale_boxes total={total}: {ulps} ulp from the rounded float64 result; "
          f"{'bit-equal to' if torch.equal(got, r32) else 'differs from'} float32 arithmetic with an IEEE division")
    assert ulps <= 1 and _guards_intact(buf, view)
