"""The bounds of tests/rowref.py have teeth (CPU only): the float64 references agree with torch.nn.functional in float64 where
torch has the operation, the float32 restatements of the kernels' arithmetic stay under half of each bound on every stress and
width, and each modelled defect misses its kernel's bound by at least TEETH x on the stress named for it.
tests/test_gpu_rowwise.py holds the kernels themselves to the same bounds."""
import pytest
import torch
import torch.nn.functional as F

import rowref as R

LN_WIDTHS = (4, 112, 132, 448, 516, 1024, 1028, 4096)  # narrow, ITERS 2 / 4 / 16, with and without a ragged last float4 step
ROWS = 37


def test_references_agree_with_torch_float64():
    for D in (112, 448, 1028):
        g, b = R.affine(D, 1)
        x = R.stress_rows("mixed", ROWS, D, 2)
        ref, (_, pre) = R.layernorm(x, g, b, 1e-5, act=True)
        tl = F.layer_norm(x, (D,), g.double(), b.double(), 1e-5)
        assert float((pre - tl).abs().max()) < 1e-11 and float((ref - F.gelu(tl)).abs().max()) < 1e-11
        assert float((R.gelu(x, tanh=True) - F.gelu(x, approximate="tanh")).abs().max()) < 1e-12
        xg = x.clone().requires_grad_()
        F.gelu(xg).sum().backward()
        assert float((R.gelu_grad(x) - xg.grad).abs().max()) < 1e-12
    for shape in ((2, 64, 96, 16), (1, 65, 97, 8), (1, 7, 5, 64)):
        img, w, b = R.stem_inputs(*shape, 3)
        ref = R.stem_conv(img, w, b)[0]
        tc = F.silu(F.conv2d(img.double().permute(0, 3, 1, 2) / 255, w.double().permute(3, 2, 0, 1), b.double(), stride=2, padding=1))
        assert ref.shape == tc.permute(0, 2, 3, 1).shape and float((ref - tc.permute(0, 2, 3, 1)).abs().max()) < 1e-13
        assert {0, 255} <= set(img[:, 0].unique().tolist()) and {0, 255} <= set(img[:, :, -1].unique().tolist())
    for shape in ((2, 20, 12, 16), (1, 3, 4, 8), (1, 1, 1, 8)):
        x = R.pool_inputs(*shape, 4)
        assert bool((x == -65504).any()) and bool((x == 0).any())
        tp = F.max_pool2d(x.double().permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)
        assert torch.equal(R.maxpool5(x).double(), tp)
        tu = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)
        assert torch.equal(R.upsample2(x).double(), tu)
    assert float(R.maxpool5(R.pool_inputs(2, 20, 12, 16, 4)).min()) == -65504  # a window of nothing but the identity element
    n, H, W, nc = 2, 5, 7, 3
    head = R.detect_inputs(n, H, W, nc, 72, 2.0, 5)
    ref = R.detect_decode(head, nc, 16.0)[0]
    dist = (head[..., :64].double().reshape(n, H * W, 4, 16).softmax(-1) * torch.arange(16.0).double()).sum(-1)
    assert float((ref[..., 2] - (dist[..., 0] + dist[..., 2]) * 16).abs().max()) < 1e-12
    assert float((ref[..., 4:] - head[..., 64:64 + nc].double().reshape(n, H * W, nc).sigmoid()).abs().max()) < 1e-15


def test_half_ulp16():
    v = torch.tensor([1.0, 1.9990234375, 2.0, 2.0 ** -14, 2.0 ** -15, 0.0, -3.0, 65504.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -10, 2.0 ** 4])
    assert torch.equal(R.half_ulp16(v), want.double())
    x = (torch.linspace(-8, 8, 100001).exp2() * 255).double()  # f32 values from the subnormal range up to 65280
    assert bool(((x.half().double() - x).abs() <= R.half_ulp16(x)).all())


def test_stress_rows_are_what_they_say():
    for kind in R.STRESSES:
        x = R.stress_rows(kind, ROWS, 448, 6)
        assert len({tuple(r[:4].tolist()) for r in x.float()}) == ROWS, "every row distinct"
        assert len({tuple(r[:4].tolist()) for r in x.half()}) == ROWS
    big, small, mixed = (R.stress_rows(k, ROWS, 448, 6) for k in ("bigmean", "small", "mixed"))
    assert float((big.mean(1).abs() / big.std(1)).min()) > 80
    assert 0.5e-5 < float(small.var(1).min()) and float(small.var(1).max()) < 2e-5
    assert float(mixed[0].std()) > 2 and float(mixed[1].mean()) > 49 and float(mixed[2].std()) < 4e-3


@pytest.mark.parametrize("D", LN_WIDTHS)
def test_layernorm_f32_within_half_bound(D):
    g, b = R.affine(D, 3)
    worst = 0.0
    for kind in R.STRESSES:
        for dt in (torch.float32, torch.float16):
            x = R.seen(R.stress_rows(kind, ROWS, D, 5), dt)
            for act in (False, True):
                for eps in (1e-5, 1e-6):
                    ref, aux = R.layernorm(x, g, b, eps, act)
                    got = R.layernorm_f32(x.float(), g, b, eps, act)
                    worst = max(worst, R.ln_unit_ratio(got, ref, aux, act, False))
                    assert R.ratio(got, ref, R.ln_bound(ref, aux, act, False)) <= 0.5, (kind, dt, act, eps)
                    assert R.ratio(got.half(), ref, R.ln_bound(ref, aux, act, True)) <= 1.0, (kind, dt, act, eps)
    print(f"layernorm float32 restatement D={D}: {R.fmt(worst)} of the unit bound (C_LN / 2 = {R.C_LN / 2})")
    assert worst <= R.C_LN / 2


@pytest.mark.parametrize("defect", R.LN_DEFECTS)
def test_layernorm_defect_misses_bound(defect):
    kind, act = R.DEFECT_STRESS[defect], defect == "gelu_tanh"
    for D in (112, 132, 448, 1024, 4096):
        g, b = R.affine(D, 3)
        x = R.seen(R.stress_rows(kind, ROWS, D, 5), torch.float32)
        for eps in (1e-5, 1e-6):
            ref, aux = R.layernorm(x, g, b, eps, act)
            miss = R.ratio(R.layernorm(x, g, b, eps, act, defect=defect)[0], ref, R.ln_bound(ref, aux, act, False))
            print(f"defect {defect} on {kind} D={D} eps={eps}: {R.fmt(miss)} x the bound")
            assert miss >= R.TEETH, f"{defect} D={D}: within {miss:.1f} x the bound: the bound has no teeth"


def test_token_mean_f32_within_half_bound():
    for B, T, D in ((3, 201, 1024), (2, 7, 260), (1, 1, 4)):
        for kind in R.STRESSES:
            for dt in (torch.float32, torch.float16):
                x = R.seen(R.stress_rows(kind, B * T, D, 7), dt)
                ref, bound = R.token_mean(x, B, T, D)
                r = R.ratio(R.token_mean_f32(x.float(), B, T, D), ref, bound)
                print(f"token_mean float32 restatement {(B, T, D)} {kind} {dt}: {R.fmt(r)} of the bound")
                assert r <= 0.5


@pytest.mark.parametrize("hd", (64, 80, 96))
def test_rope_f32_and_defects(hd):
    for n_prefix in (0, 1, 5):
        B, T, H = 2, n_prefix + 9, 3
        x, c, s = R.rope_inputs(B, T, H, hd, n_prefix, 9)
        q = x[:, :H * hd]
        ref, rnd, e = R.rope(q, B, T, H, hd, n_prefix, c, s)
        got = R.rope_f32(q, B, T, H, hd, n_prefix, c, s)
        r = R.excess(got, ref, rnd, e)
        print(f"rope float32 restatement hd={hd} n_prefix={n_prefix}: {R.fmt(r)} of the float32 part")
        assert r <= 0.5 and torch.equal(got.view(B, T, -1)[:, :n_prefix], q.view(B, T, -1)[:, :n_prefix])
        for defect in ("rope_no_neg", "rope_prefix"):
            if defect == "rope_prefix" and not n_prefix:
                continue
            miss = R.ratio(R.rope(q, B, T, H, hd, n_prefix, c, s, defect=defect)[0], ref, rnd + e)
            print(f"defect {defect} hd={hd} n_prefix={n_prefix}: {R.fmt(miss)} x the bound")
            assert miss >= R.TEETH


@pytest.mark.parametrize("shape", ((2, 64, 96, 16), (1, 65, 97, 8), (1, 7, 5, 64)))
def test_stem_conv_f32_and_defect(shape):
    img, w, b = R.stem_inputs(*shape, 11)
    ref, rnd, e = R.stem_conv(img, w, b)
    r = R.excess(R.stem_conv_f32(img, w, b), ref, rnd, e)
    miss = R.ratio(R.stem_conv(img, w, b, defect="stem_pad_clamp")[0], ref, rnd + e)
    print(f"stem_conv float32 restatement {shape}: {R.fmt(r)} of the float32 part; defect stem_pad_clamp: {R.fmt(miss)} x the bound")
    assert r <= 0.5 and miss >= R.TEETH


def test_detect_decode_f32_sets_the_constants():
    """K_BOX and K_SIG are 4x what the float32 restatement reaches on the GPU test's own inputs: recomputed here at K = 1."""
    box = sig = 0.0
    for i, (n, H, W, nc, ldh, scale) in enumerate(R.DETECT_CASES):
        head = R.detect_inputs(n, H, W, nc, ldh, scale, 20 + i)
        assert ldh % 4 == 0 and ldh > 64 + nc
        ref, bound = R.detect_decode(head, nc, 8.0 * 2 ** (i % 3))
        got = R.detect_decode_f32(head, nc, 8.0 * 2 ** (i % 3))
        box = max(box, R.ratio(got[..., :4], ref[..., :4], bound[..., :4]) * R.K_BOX)
        sig = max(sig, R.ratio(got[..., 4:], ref[..., 4:], bound[..., 4:]) * R.K_SIG)
        if i < 3:
            miss = R.ratio(R.detect_decode(head, nc, 8.0 * 2 ** (i % 3), defect="decode_anchor0")[0], ref, bound)
            print(f"defect decode_anchor0 on {(n, H, W, nc)}: {R.fmt(miss)} x the bound")
            assert miss >= R.TEETH
    e = torch.exp(R.detect_inputs(*R.DETECT_CASES[2][:5], 40.0, 22)[..., :16] - 100.0)
    assert bool((e.float() == 0).any()), "scale 40 must underflow exp in float32"
    print(f"detect_decode float32 restatement: boxes {R.fmt(box)} (K_BOX {R.K_BOX}), scores {R.fmt(sig)} (K_SIG {R.K_SIG})")
    assert box <= R.K_BOX / 2 and sig <= R.K_SIG / 2
    assert R.K_BOX <= 4 * box + 1 and R.K_SIG <= 4 * sig + 1, "the constants are 4x the measured ratios, no more"


def test_scale_boxes_f32_within_one_ulp():
    pad, gain, w, h = (0.0, 140.0), 1 / 3, 1920.0, 1080.0  # a 1080p frame letterboxed to 640
    for total in (1, 255, 257, 1000):
        boxes = R.box_inputs(total, 30 + total, pad[0], pad[1], gain, w, h)
        r64, r32 = R.scale_boxes(boxes, pad[0], pad[1], gain, w, h)
        assert R.ulps32(r64, r32) <= 1
        if total == 1000:
            for c, hi in enumerate((w, h, w, h)):
                assert bool((r64[:, c] == 0).any()) and bool((r64[:, c] == hi).any()), "every clip edge straddled"
                assert bool(((r64[:, c] > 0) & (r64[:, c] < hi)).any())
