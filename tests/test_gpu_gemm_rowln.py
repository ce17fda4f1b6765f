"""lmx_k_gemm with ln_out (include/lmx.h; csrc/gemm2.hip gemm2_rowln_kernel, route dma_128xrow_ln): the residual GEMM whose tile holds
whole rows and writes the LayerNorm of its f32 result as f16 from the same launch (Hiera stage 3: the attention projection writes
layer_norm2's rows).

  1. the f32 result is torch.equal to the same operands without ln_out (the 256 x 256 LDS-DMA tiling or, below 512 rows, the
     register-staged kernel): the same MFMA sequence in ascending k and the same epilogue rounding;
  2. the f16 LayerNorm rows are within tests/rowref.py's float64 bound, C_LN 2^-24 (|ref| + |g| rstd (|x - mu| + max |x|)) plus half an
     f16 ulp, evaluated on the f32 values the device wrote — and are the bits lmx_k_layernorm returns for those values (the kernel
     restates layernorm_rows_kernel's arithmetic in its reduction order: that is what keeps the model's output unchanged);
  3. a row alone (M = 1), inside M = 129 and inside M = 4096 has the same bits in both outputs;
  4. two launches on the same inputs return the same bits;
  5. the route is asserted before every launch;
  6. Hiera-B+ with ln_out in its plan returns the bits of the plan with the two launches, and runs 15 LayerNorm launches fewer.

Rows: N = K = 448 with M = 1, 127, 128, 129 (both sides of the 128-row tile edge), 257 (three tiles, the last one a single row) and 4096
(32 tiles: one frame), and N = K = 224 at M = 129 (a row narrower than the tile: the second float4 of most lanes is outside the row;
K = 224 ends inside a 64-deep k-tile).  The f32 rows land in the four families of rowref.stress_rows (3 N + 0.5; a mean 100 x the spread;
a variance the size of eps; rows alternating between the three) because the residual is chosen as family - (A W^T + bias).  Both outputs
lie in sentinel-filled buffers whose guard rows and columns must come back untouched."""
import functools

import pytest
import torch

import rowref as R

pytestmark = pytest.mark.gpu

ROWLN = "dma_128xrow_ln"
SENT = -1234.0
EPS = 1e-5  # rowref's "small" family has a variance of this size
MS = (1, 127, 128, 129, 257, 4096)
SHAPES = [(448, 448, M) for M in MS] + [(224, 224, 129)]
MMAX = {448: 4096, 224: 129}


def _guarded(rows, cols, dtype, dev, ld=None, guard_rows=2):
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
def _operands(N, K, kind, dev):
    """(a f16 [MMAX, K], w f16 [N, K], bias, gamma, beta, res f32 [MMAX, N]) on the device; every M of the shape list is a prefix.
    res = family - (a w^T + bias) with the product taken from the library itself (an f32 GEMM without residual), so that the rows the
    kernel writes are the family's to within an f32 rounding."""
    from lmx import kernels as K_

    M = MMAX[N]
    g = torch.Generator().manual_seed(N + 7)
    a = torch.randn((M, K), generator=g).half().to(dev)
    w = (torch.randn((N, K), generator=g) * K ** -0.5).half().to(dev)
    bias = torch.randn((N,), generator=g).to(dev)
    gamma, beta = (t.to(dev) for t in R.affine(N, 3))
    prod = K_.gemm(a, w, bias=bias, out_dtype=torch.float32)
    res = (R.stress_rows(kind, M, N, 5) - prod.cpu().double()).float().to(dev)
    return a, w, bias, gamma, beta, res


def _plain(a, w, bias, res):
    from lmx import kernels as K_

    M, K = a.shape
    N = w.shape[0]
    got = K_.gemm_route(M, N, K, out_dtype=torch.float32, res=True)  # (M < 512: the register-staged kernel; 4096 rows: an LDS-DMA tiling)
    assert got == ("v1_128x128" if M < 512 else "dma_256x128x64_s3_stag"), f"without ln_out M={M} N={N} K={K}: {got}"
    return K_.gemm(a, w, bias=bias, res=res, out_dtype=torch.float32)


def _rowln(a, w, bias, res, gamma, beta, strided=False, in_place=False):
    """-> (x f32, h f16, guards intact): the launch with ln_out, both outputs inside sentinel buffers (strided: row strides N + 8 / N + 12);
    in_place: the residual IS the output buffer, as the model's residual stream is."""
    from lmx import kernels as K_

    M, K = a.shape
    N = w.shape[0]
    assert K_.gemm_route(M, N, K, out_dtype=torch.float32, res=True, ln_out=True, ldc=N + 8 if strided else None) == ROWLN
    xbuf, x = _guarded(M, N, torch.float32, a.device, N + 8 if strided else N)
    hbuf, h = _guarded(M, N, torch.float16, a.device, N + 12 if strided else N)
    if in_place:
        x.copy_(res)
        res = x
    K_.gemm(a, w, bias=bias, res=res, out=x, ln_out=(h, gamma, beta, EPS))
    return x, h, _guards_intact(xbuf, x) and _guards_intact(hbuf, h)


@pytest.mark.parametrize("kind", R.STRESSES)
@pytest.mark.parametrize("N,K,M", SHAPES, ids=[f"N{n}K{k}M{m}" for n, k, m in SHAPES])
def test_rowln_matches_the_plain_gemm_and_the_float64_layernorm(cuda, N, K, M, kind):
    from lmx import kernels as K_

    a, w, bias, gamma, beta, res = _operands(N, K, kind, cuda)
    a, res = a[:M], res[:M]
    want = _plain(a, w, bias, res)
    worst = 0.0
    for strided, in_place in ((False, False), (True, True)):
        what = f"N={N} K={K} M={M} {kind} strided={strided} in_place={in_place}"
        x, h, intact = _rowln(a, w, bias, res, gamma, beta, strided, in_place)
        assert intact, f"{what}: wrote outside its rows / columns"
        assert torch.equal(x, want), f"{what}: {int((x != want).sum())} f32 outputs differ from the launch without ln_out"
        ref, aux = R.layernorm(x.cpu().double(), gamma.cpu(), beta.cpu(), EPS)
        r = R.ratio(h.cpu(), ref, R.ln_bound(ref, aux, False, True))
        u = R.ln_unit_ratio(h.cpu(), ref, aux, False, True)
        worst = max(worst, u)
        print(f"gemm ln_out {what}: {r:.3f} of the bound, {R.fmt(u)} of the unit bound (C_LN {R.C_LN})")
        assert r <= 1.0, f"{what}: LayerNorm rows at {r:.2f} x the bound"
        sep = K_.layernorm(x.contiguous(), gamma, beta, EPS)
        assert torch.equal(h, sep), f"{what}: {int((h != sep).sum())} LayerNorm outputs differ from lmx_k_layernorm on the same rows"
        x2, h2, _ = _rowln(a, w, bias, res, gamma, beta, strided, in_place)
        assert torch.equal(x2, x) and torch.equal(h2, h), f"{what}: a second launch returned other bits"
    print(f"gemm ln_out N={N} K={K} M={M} {kind}: GPU ratio {R.fmt(worst)} of the unit bound (C_LN {R.C_LN})")


@pytest.mark.parametrize("N,K", [(448, 448), (224, 224)])
def test_rowln_rows_do_not_depend_on_the_batch(cuda, N, K):
    """Every row of the M = 129 problem alone (M = 1: a one-row tile) and, at N = 448, inside M = 4096 (the row sits in another tile, at
    another place of it, beside other rows): the same bits in both outputs."""
    a, w, bias, gamma, beta, res = _operands(N, K, "mixed", cuda)
    x129, h129, _ = _rowln(a[:129], w, bias, res[:129], gamma, beta)
    for i in range(129):
        x1, h1, _ = _rowln(a[i:i + 1], w, bias, res[i:i + 1], gamma, beta)
        assert torch.equal(x1[0], x129[i]) and torch.equal(h1[0], h129[i]), f"N={N}: row {i} alone differs from the row inside M = 129"
    if MMAX[N] > 129:
        M = MMAX[N]
        xm, hm, _ = _rowln(a, w, bias, res, gamma, beta)
        assert torch.equal(xm[:129], x129) and torch.equal(hm[:129], h129), f"N={N}: rows inside M = {M} differ from M = 129"
        # the same 129 rows at the END of a batch: another tile and another place inside it (4096 - 129 = 31 tiles - 1 row)
        sh = M - 129
        xs, hs, _ = _rowln(torch.cat((a[129:], a[:129])), w, bias, torch.cat((res[129:], res[:129])), gamma, beta)
        assert torch.equal(xs[sh:], x129) and torch.equal(hs[sh:], h129), f"N={N}: rows at the end of M = {M} differ from M = 129"


def test_hiera_stage3_uses_rowln_and_keeps_its_bits(cuda):
    """Hiera-B+ on one frame: the 15 same-width blocks of stage 3 run their projection with ln_out and drop their layer_norm2 launch,
    and every stage and FPN output is bit-identical to the plan with the two launches (the encoder's proj_ln switched off: no record of its plan has ln_out)."""
    import numpy as np

    from lmx import kernels as K_
    from lmx import sam, synth, weights

    cfg = sam.hiera_b_plus()
    enc = sam.HieraEncoder(cfg, weights.synth_state_dict(sam.param_spec(cfg), 5), cuda)
    frames = torch.from_numpy(np.stack([synth.synth_frame(3, 41)], 0)).to(cuda)

    def run():
        K_.start_launch_trace()
        out = enc.encode(frames)
        torch.cuda.synchronize()
        _, shapes = K_.stop_launch_trace(by_shape=True)
        rowln = sum(r["launches"] for (_, key), r in shapes.items() if key.startswith("gemm ") and key.endswith(" ln_out"))
        ln448 = sum(r["launches"] for (_, key), r in shapes.items() if key.startswith("layernorm ") and " D=448 " in key)
        return out, rowln, ln448

    new, rowln, ln448 = run()
    assert [i for i, p in enumerate(enc.plan(1, enc.grid0)) if p.ln_out] == list(range(6, 21))
    enc.proj_ln = False
    assert not any(p.ln_out for p in enc.plan(1, enc.grid0))
    old, rowln_old, ln448_old = run()
    assert (rowln, rowln_old) == (15, 0) and ln448_old - ln448 == 15, (rowln, rowln_old, ln448, ln448_old)
    for name in ("fpn", "stages"):
        for lvl, (a, b) in enumerate(zip(new[name], old[name])):
            assert torch.equal(a, b), f"{name}[{lvl}]: {int((a != b).sum())} values differ from the two-launch plan"
