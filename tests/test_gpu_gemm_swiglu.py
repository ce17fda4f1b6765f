"""lmx_k_gemm with the gated epilogue LMX_ACT_SWIGLU (include/lmx.h) against float64, through every kernel an fc1 of the gated
DINO shapes can reach, plus batch invariance across those kernels and the rejected descriptors.

Kernels and thresholds (csrc/gemm.hip lmx_k_gemm, csrc/gemm2.hip lmx_gemm2_launch; mirrored by `_variant` below and asserted, so
a change of the launch rules shows up here rather than silently shrinking the coverage):
  M < 512                                                            -> v1   register-staged 128 x 128 (gemm.hip)
  K >= 448, tiles256 >= 200, q256 >= 0.75, N fills >= 85 % of its 256s -> Z    256 x 256 x 64, 2 slots
  else K >= 1792 or ceil(M/256) * ceil(N/128) <= 256                 -> T    256 x 128 x 64, 3 slots, staggered
  else                                                               -> C    256 x 128 x 32, 3 slots
Each M below sits one row under or on a threshold of its (K, N).

Error bound.  tests/test_gpu_kernels.py (test_gemm_plain) accepts an f16-output GEMM value x = a . w + b, with these input
scales, within  t(x) = 2e-3 + 2e-3 |x|  of the reference, whatever K.  The gated output is the product s * silu(g) * u of two
such values (rounded to f16 once, as that GEMM's output is).  Propagating t through the product, with |silu'| <= L = 1.1
(max of silu' is 1.0998 at x = 2.3994):
    | silu(g + dg) (u + du) - silu(g) u |  <=  L t(g) |u|  +  |silu(g)| t(u)  +  L t(g) t(u)
and the LayerScale multiplies it:  tol = |s| * ( L t(g) |u| + |silu(g)| t(u) + L t(g) t(u) ),  g, u, s the float64 values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {  # (K, N) -> M values: 511 | 512 straddle v1 / LDS-DMA, the others the tiling rules of that shape
    (384, 3072): (511, 512, 2560, 2561),               # T up to 10 m-tiles (10 * 24 = 240 tiles), C beyond; K < 448: never Z
    (1280, 10240): (511, 512, 768, 769, 1024, 1025),   # T up to 3 m-tiles (240 tiles), C at 4, Z from 5 (200 256-tiles, q = 0.78)
    (1536, 8192): (511, 512, 1024, 1025, 1536, 1537),  # T up to 4 m-tiles (256 tiles), C at 5 - 6, Z from 7 (224 256-tiles)
}
EXPECT = {
    (384, 3072): ("v1", "T", "T", "C"),
    (1280, 10240): ("v1", "T", "T", "C", "C", "Z"),
    (1536, 8192): ("v1", "T", "T", "C", "C", "Z"),
}


def _variant(M, N, K):
    """The kernel lmx_k_gemm launches for a dense f16 problem with aligned operands (the rules quoted in the module docstring)."""
    if M < 512:
        return "v1"
    mt, nt256 = (M + 255) // 256, (N + 255) // 256
    tiles256 = mt * nt256
    q256 = tiles256 / (((tiles256 + 255) // 256) * 256)
    nfrac = N / (nt256 * 256)
    if K >= 448 and tiles256 >= 200 and q256 >= 0.75 and nfrac >= 0.85:
        return "Z"
    if K < 448 and 224 <= N <= 1536 and N % 256 and nfrac >= 0.85 and tiles256 >= 200 and q256 >= 0.75:
        return "E" if K > 128 else "Z"
    return "T" if (K >= 1792 or mt * ((N + 127) // 128) <= 256) else "C"


def test_m_values_cover_every_reachable_kernel():
    for (K, N), Ms in SHAPES.items():
        assert tuple(_variant(M, N, K) for M in Ms) == EXPECT[(K, N)], (K, N)
    assert {v for e in EXPECT.values() for v in e} == {"v1", "T", "C", "Z"}


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def _silu64(x):
    return x / (1 + torch.exp(-x))


def _sample_rows(M):
    """First / last rows, the rows around every 16 / 64 / 128 / 256-row tile edge near the ends, and a spread."""
    s = {0, 1, 15, 16, 63, 64, 127, 128, 255, 256, M - 257, M - 256, M - 129, M - 128, M - 65, M - 17, M - 16, M - 2, M - 1}
    s |= set(range(7, M, max(M // 40, 1)))
    return torch.tensor(sorted(r for r in s if 0 <= r < M))


@pytest.mark.parametrize("bias", ["zero_bias", "bias"])
@pytest.mark.parametrize("scale", ["no_scale", "scale"])
@pytest.mark.parametrize("K,N", list(SHAPES))
def test_gated_gemm_matches_float64_and_rows_do_not_depend_on_m(cuda, K, N, scale, bias):
    """Every M of SHAPES: all output columns of a row sample within the propagated bound (module docstring) of float64
    s * silu(x Wg^T + bg) * (x Wu^T + bu); then the rows of each smaller launch equal, bit for bit, the same rows of every larger
    one — each pair of kernels among v1 / T / C / Z that the shape reaches."""
    from lmx import dino
    from lmx import kernels as Kk

    I, Ms = N // 2, SHAPES[(K, N)]
    a = _rand((max(Ms), K), 1).half()
    wg, wu = _rand((I, K), 2, K ** -0.5).half(), _rand((I, K), 3, K ** -0.5).half()
    if bias == "bias":
        bg, bu = _rand((I,), 4), _rand((I,), 5)
    else:
        bg, bu = torch.zeros(I), torch.zeros(I)
    s = _rand((I,), 6) if scale == "scale" else None
    w = torch.from_numpy(dino.pack_gated(wg.numpy(), wu.numpy())).to(cuda)
    b = torch.from_numpy(dino.pack_gated(bg.numpy(), bu.numpy())).to(cuda)
    ad = a.to(cuda)
    sd = s.to(cuda) if s is not None else None
    wg64, wu64 = wg.to(cuda).double(), wu.to(cuda).double()
    outs, worst = {}, 0.0
    for M in Ms:
        got = Kk.gemm(ad[:M], w, bias=b, act=Kk.ACT_SWIGLU, scale=sd)
        assert tuple(got.shape) == (M, I) and got.dtype == torch.float16
        outs[M] = got
        rows = _sample_rows(M).to(cuda)
        x = ad[rows].double()
        g = x @ wg64.t() + bg.to(cuda).double()
        u = x @ wu64.t() + bu.to(cuda).double()
        sv = sd.double().abs() if sd is not None else 1.0
        ref = _silu64(g) * u * (sd.double() if sd is not None else 1.0)
        tg, tu = 2e-3 + 2e-3 * g.abs(), 2e-3 + 2e-3 * u.abs()
        tol = sv * (1.1 * tg * u.abs() + _silu64(g).abs() * tu + 1.1 * tg * tu)
        err = (got[rows].double() - ref).abs()
        ratio = float((err / tol).max())
        worst = max(worst, ratio)
        print(f"swiglu K={K} N={N} M={M} ({_variant(M, N, K)}) {scale} {bias}: max err {float(err.max()):.3e}, max err/tol {ratio:.4f}")
        assert bool(torch.isfinite(got).all())
        assert ratio <= 1.0, f"M={M} ({_variant(M, N, K)}): {int((err > tol).sum())} values outside the bound, worst ratio {ratio:.3f}"
    for i, m_small in enumerate(Ms):
        for m_big in Ms[i + 1:]:
            assert torch.equal(outs[m_small], outs[m_big][:m_small]), \
                f"rows of the M={m_small} launch ({_variant(m_small, N, K)}) differ inside the M={m_big} launch ({_variant(m_big, N, K)})"


def test_output_stride_and_untouched_padding(cuda):
    """C with ldc > N/2 (a column slice of a wider buffer), both kernels: the columns beyond N/2 stay untouched."""
    from lmx import dino
    from lmx import kernels as Kk

    K, I = 384, 1536
    wg, wu = _rand((I, K), 2, K ** -0.5).half(), _rand((I, K), 3, K ** -0.5).half()
    w = torch.from_numpy(dino.pack_gated(wg.numpy(), wu.numpy())).to(cuda)
    for M in (201, 1608):
        a = _rand((M, K), 1).half().to(cuda)
        buf = torch.full((M, I + 64), 7.0, dtype=torch.float16, device=cuda)
        Kk.gemm(a, w, act=Kk.ACT_SWIGLU, out=buf[:, :I])
        assert torch.equal(buf[:, :I], Kk.gemm(a, w, act=Kk.ACT_SWIGLU))
        assert bool((buf[:, I:] == 7.0).all())


def test_rejected_descriptors(cuda):
    """N % 32 != 0, a residual, pooled rows and an f32 output return LMX_EINVAL (-1) with a message that names the epilogue."""
    from lmx import kernels as Kk

    a = torch.zeros((1024, 64), dtype=torch.float16, device=cuda)
    w = torch.zeros((256, 64), dtype=torch.float16, device=cuda)
    cases = {
        "N % 32": lambda: Kk.gemm(a, w[:48], act=Kk.ACT_SWIGLU),
        "residual": lambda: Kk.gemm(a, w, act=Kk.ACT_SWIGLU, res=torch.zeros((1024, 256), dtype=torch.float16, device=cuda)),
        "pooled rows": lambda: Kk.gemm(a, w, act=Kk.ACT_SWIGLU, pool_hw=(32, 32)),
        "f32 out": lambda: Kk.gemm(a, w, act=Kk.ACT_SWIGLU, out_dtype=torch.float32),
    }
    for what, fn in cases.items():
        with pytest.raises(Kk.LmxError, match=r"rc=-1.*SWIGLU") as e:
            fn()
        print(what, "->", e.value)
    with pytest.raises(Kk.LmxError, match=r"rc=-1.*bad act"):
        Kk.gemm(a, w, act=5)


def test_unfused_form_agrees(cuda):
    """Plain GEMM to the 2I-wide f16 buffer + lmx_k_swiglu (the timing reference) computes the same function: it rounds gate and
    up to f16 before the product, so it is compared at that rounding (2^-10 relative on each factor), not bit for bit."""
    from lmx import dino
    from lmx import kernels as Kk

    M, K, I = 1608, 384, 1536
    a = _rand((M, K), 1).half().to(cuda)
    wg, wu = _rand((I, K), 2, K ** -0.5).half(), _rand((I, K), 3, K ** -0.5).half()
    b = _rand((2 * I,), 4)
    fused = Kk.gemm(a, torch.from_numpy(dino.pack_gated(wg.numpy(), wu.numpy())).to(cuda),
                    bias=torch.from_numpy(dino.pack_gated(b[:I].numpy(), b[I:].numpy())).to(cuda), act=Kk.ACT_SWIGLU)
    gu = Kk.gemm(a, torch.cat([wg, wu], 0).to(cuda), bias=b.to(cuda))
    unfused = Kk.swiglu(gu)
    g, u = gu[:, :I].double(), gu[:, I:].double()
    tol = 2.0 ** -10 * (1.1 * g.abs() * u.abs() + _silu64(g).abs() * u.abs()) + 2.0 ** -10 * (_silu64(g) * u).abs() + 1e-6
    assert bool(((fused.double() - unfused.double()).abs() <= tol).all())
