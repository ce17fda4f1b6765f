"""The route rule of lmx_gemm_desc.ln_out (include/lmx.h), asked of the library's own selection without a GPU: a request that carries
ln_out takes the 128-rows-by-whole-row kernel at EVERY M (a layer's choice: a frame's bits must not depend on its batch), and a request
the kernel was not built for is an argument error, never another kernel."""
import pytest
import torch

from lmx import kernels as K

F16, F32 = torch.float16, torch.float32
ROWLN = "dma_128xrow_ln"


@pytest.mark.parametrize("M", [1, 127, 128, 129, 511, 512, 4096, 122880])
@pytest.mark.parametrize("N,K_", [(448, 448), (224, 224), (448, 64), (16, 8)])
def test_rowln_is_selected_for_every_row_count(M, N, K_):
    assert K.gemm_route(M, N, K_, out_dtype=F32, res=True, ln_out=True) == ROWLN


def test_without_ln_out_the_routes_are_the_old_ones():
    assert K.gemm_route(1, 448, 448, out_dtype=F32, res=True) == "v1_128x128"
    assert K.gemm_route(122880, 448, 448, out_dtype=F32, res=True) == "dma_256x256x64_s2"


REFUSED = {
    "N=896": dict(N=896),
    "N=464 (> 448)": dict(N=464),
    "N=440 (not a multiple of 16)": dict(N=440),
    "K=1792": dict(K_=1792),
    "K=456 (> 448)": dict(K_=456),
    "f16 output": dict(out_dtype=F16),
    "no residual": dict(res=False),
    "broadcast residual": dict(res_rows=4),
    "split-K": dict(split_k=2),
    "a_rep": dict(K_=192, a_rep=2),
    "activation": dict(act=K.ACT_GELU),
    "scale": dict(scale=True),
}


@pytest.mark.parametrize("why", REFUSED)
@pytest.mark.parametrize("M", [1, 4096, 122880])
def test_rowln_refuses_what_it_was_not_built_for(M, why):
    kw = dict(N=448, K_=448, out_dtype=F32, res=True)
    kw.update(REFUSED[why])
    N, K_ = kw.pop("N"), kw.pop("K_")
    with pytest.raises(K.LmxError, match="ln_out"):
        K.gemm_route(M, N, K_, ln_out=True, **kw)
    # the same request without ln_out is a valid launch of another kernel: the refusal is ln_out's
    # (a_rep is built into the LDS-DMA kernel only: M >= 512)
    if not (why == "a_rep" and M < 512):
        assert K.gemm_route(M, N, K_, **kw)



def test_launch_trace_counts_the_layernorm_rows():
    """start_launch_trace's algorithmic bytes of the launch: A + W + f32 residual + f32 result, plus the f16 LayerNorm rows."""
    import ctypes as C

    M, N, K_ = 122880, 448, 448
    d = K.GemmDesc()
    d.A = d.W = d.C = d.res = 4096
    d.M, d.N, d.K, d.out_dtype = M, N, K_, K.F32
    plain = K._work("lmx_k_gemm", [C.byref(d)])
    d.ln_out = 4096
    cls, flops, by, key = K._work("lmx_k_gemm", [C.byref(d)])
    assert by == 2 * M * K_ + 2 * N * K_ + 8 * M * N + 2 * M * N == plain[2] + 2 * M * N
    assert flops == plain[1] and cls == "gemm/hbm-bound" and key == plain[3] + " ln_out"
