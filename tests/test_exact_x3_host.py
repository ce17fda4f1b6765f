"""The x3 model of tests/x3ref.py on the CPU: the split reconstructs an f32 value to 2^-22, the x3 dot product of the exact
plan meets the per-element bound tests/test_gpu_exact.py holds the kernels to, and the same product with `lo` or `wlo`
dropped (an f16-only operand) misses it by a wide factor — the bound has teeth without a GPU."""
import numpy as np
import pytest
import torch

import x3ref as X
from lmx.exact import split_rows_x3

# the GEMM bound of tests/test_gpu_exact.py (C_GEMM there): |got - ref| <= C * (sum_k |x_k w_k| + |b|)
C_GEMM = 2.0 ** -21


def test_x3_split_reconstructs_f32_to_2_pow_22():
    rng = np.random.default_rng(0)
    # |x| from 2^-13 (below it lo leaves the normal f16 range: lmx.h) to 65504 (the f16 maximum), both signs
    mag = np.minimum(np.exp2(rng.uniform(-13, 16, 20000)), 65504)
    x = torch.from_numpy((mag * np.sign(rng.standard_normal(20000))).astype(np.float32))
    hi, lo = X.x3_split(x)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    v = hi.double() + lo.double() / 2048
    rel = float(((v - x.double()).abs() / x.double().abs()).max())
    assert rel <= 2.0 ** -22, rel
    # the value alone, hi only, is 2^-12 off: the lo channel carries eleven more bits
    assert float(((hi.double() - x.double()).abs() / x.double().abs()).max()) > 2.0 ** -13
    packed = X.x3_pack(x.view(4, -1), g=[1000, 2000, 2000])
    assert packed.shape == (4, 15000)
    assert torch.equal(X.x3_hi(packed, [1000, 2000, 2000]), X.x3_hi2(packed, [1000, 2000, 2000]))
    assert torch.equal(X.x3_value(packed, [1000, 2000, 2000]), v.view(4, -1))


@pytest.mark.parametrize("K,groups", [(64, None), (120, [40, 80]), (160, [64, 48, 48]), (288, [32] * 9)])
def test_x3_dot_meets_the_bound_and_f16_operands_do_not(K, groups):
    rng = np.random.default_rng(K)
    M, N = 192, 64
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32))
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    gl = groups or [K]
    w3, sc, e = split_rows_x3(w, gl)
    bs = torch.from_numpy(np.ldexp(b, e).astype(np.float32)).double() * torch.from_numpy(sc).double()
    ref = x.double() @ torch.from_numpy(w).double().t() + torch.from_numpy(b).double()
    den = X.abs_dot(x, w) + torch.from_numpy(np.abs(b)).double()
    a3 = X.x3_pack(x, gl)
    for dot in (X.x3_dot, X.f32_chain_dot):  # exact sums, and an f32 accumulator rounded per 32 columns
        r = X.ratio(dot(a3, w3, sc) + bs, ref, den)
        assert r <= C_GEMM, (dot.__name__, r)
    r = X.ratio(X.f32_chain_dot(a3, w3, sc) + bs, ref, den)
    t_lo = X.ratio(X.f32_chain_dot(X.x3_pack(x, gl, drop_lo=True), w3, sc) + bs, ref, den)
    t_wlo = X.ratio(X.f32_chain_dot(a3, X.drop_wlo(w3, gl), sc) + bs, ref, den)
    print(f"K={K}: x3 ratio 2^{np.log2(r):.2f}, lo dropped {t_lo / C_GEMM:.0f} x the bound, wlo dropped {t_wlo / C_GEMM:.0f} x")
    assert t_lo >= 100 * C_GEMM and t_wlo >= 100 * C_GEMM, (t_lo / C_GEMM, t_wlo / C_GEMM)
