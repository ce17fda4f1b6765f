"""Thin torch-tensor front end of the C-ABI (include/lmx.h).  PyTorch is used for device memory and streams only:
every function below checks shapes/strides on the host, fills the C descriptor and enqueues ONE liblmx kernel on
torch's current HIP stream.  No arithmetic happens in Python and there is no fallback path."""
import ctypes as C
import os
import threading

import torch

from . import _lib
from ._lib import AttnDesc, GemmDesc, LmxError, check

F16, F32 = 0, 1
ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_SWIGLU = 0, 1, 2, 3, 4
_DT = {torch.float16: F16, torch.float32: F32}


_tls = threading.local()  # .dev: device of the launch being issued by THIS thread (read by the launch trace only)


def _stream(dev):
    """The HIP stream the launch goes to: torch's current stream OF THE OPERANDS' DEVICE `dev` (what _dev returned), not of
    the current device.  The device is passed explicitly: two threads driving two devices do not share any state here."""
    _tls.dev = dev
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(*ts):
    """Every operand must live in HBM, all on one device; returns that device (the argument of _stream)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise LmxError("lmx kernels take device (HBM) tensors only; got a CPU tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise LmxError(f"lmx kernels: operands on different devices ({dev} and {t.device})")
    if dev is None:
        raise LmxError("lmx kernels: no device operand")
    return dev


def _rows(t, what):
    """2-D row-major view: last dim contiguous; returns (rows, cols, row_stride)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise LmxError(f"{what}: expected a 2-D tensor with contiguous last dim, got shape {tuple(t.shape)} "
                       f"strides {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


# ---- which kernel a launch would take (lmx_h_*_route, include/lmx.h).  lmx_k_gemm, lmx_k_attention and lmx_k_layernorm choose their
# kernel from sizes that grow with the batch; these ask the library's own selection for shapes, without tensors and without a GPU.
_ROUTE_PTR = 4096  # stands for every operand: the route functions check pointers for null and alignment only, and never follow them


def _route_name(fn, *args):
    name = C.create_string_buffer(64)
    check(fn(*args, name, len(name)), fn.__name__)
    return name.value.decode()


def gemm_route(M, N, K, *, out_dtype=torch.float16, act=ACT_NONE, scale=False, res=False, res_rows=0, a_rep=1, pool_hw=None,
               lda=None, ldc=None, ldr=None, ln_out=False, split_k=1):
    """The kernel gemm() launches for a [M, K] x [N, a_rep * K] problem (scale, res, ln_out: whether one is given; lda / ldc / ldr
    default to dense rows; split_k: the descriptor's, for the rules that refuse it): 'v1_128x64', 'dma_256x128x64_s3_stag',
    'dma_128xrow_ln', ...; LmxError where gemm() raises it."""
    d = GemmDesc()
    d.A = d.W = d.C = d.bias = _ROUTE_PTR
    d.scale = _ROUTE_PTR if scale else None
    d.res = _ROUTE_PTR if res else None
    d.M, d.N, d.K = M, N, a_rep * K
    d.lda = K if lda is None else lda
    d.ldc = (N // 2 if act == ACT_SWIGLU else N) if ldc is None else ldc
    d.ldr = (N if ldr is None else ldr) if res else 0
    d.res_rows, d.a_rep = res_rows, a_rep
    d.act, d.out_dtype, d.a_mode = act, _DT[out_dtype], 0
    if pool_hw:
        d.a_mode, d.H, d.W_ = 2, int(pool_hw[0]), int(pool_hw[1])
    if ln_out:
        d.ln_out = d.ln_gamma = d.ln_beta = _ROUTE_PTR
        d.ld_ln, d.ln_eps = N, 1e-6
    if split_k > 1:
        d.split_k, d.split_stride = split_k, M * d.ldc
    return _route_name(_lib.load().lmx_h_gemm_route, C.byref(d))


def conv3x3_route(n, H, W, cin, cout, *, stride=1, out_dtype=torch.float16, act=ACT_SILU, res=False, scale=False, split_k=1):
    """The kernel conv3x3() launches for n dense NHWC frames of H x W x cin."""
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    d = GemmDesc()
    d.A = d.W = d.C = d.bias = _ROUTE_PTR
    d.scale = _ROUTE_PTR if scale else None
    d.res = _ROUTE_PTR if res else None
    d.lda, d.ldc, d.ldr = cin, cout, (cout if res else 0)
    d.M, d.N, d.K = n * Ho * Wo, cout, 9 * cin
    d.act, d.out_dtype, d.a_mode = act, _DT[out_dtype], 1
    d.H, d.W_, d.Cin, d.conv_stride, d.Ho, d.Wo = H, W, cin, stride, Ho, Wo
    if split_k > 1:
        d.split_k, d.split_stride = split_k, n * Ho * Wo * cout
    return _route_name(_lib.load().lmx_h_gemm_route, C.byref(d))


def attention_route(B, H, Tq, Tk, hd, *, window=None, pad=False, rel_S=0, ld=None):
    """The kernel attention() launches (window as there; pad: whether pad_k and pad_v are given; rel_S > 0: with the
    relative-position tables of an S x S grid; ld: the row stride of q / k / v / out, H * hd if None)."""
    d = AttnDesc()
    d.Q = d.K = d.V = d.O = _ROUTE_PTR
    d.ldq = d.ldk = d.ldv = d.ldo = H * hd if ld is None else ld
    d.B, d.H, d.Tq, d.Tk, d.hd = B, H, Tq, Tk, hd
    d.scale = 1.0
    if window is not None:
        d.mode = 1
        d.Gh, d.Gw, d.ws, d.q_stride = window["Gh"], window["Gw"], window["ws"], window.get("q_stride", 1)
        d.pad_k = d.pad_v = _ROUTE_PTR if pad else None
    if rel_S:
        d.rel, d.rel_S = _ROUTE_PTR, rel_S
    return _route_name(_lib.load().lmx_h_attn_route, C.byref(d))


def layernorm_route(rows, D, in_dtype=torch.float32, out_dtype=torch.float16, act=ACT_NONE):
    """The kernel layernorm() launches: 'narrow', 'rows_it2', 'row_it16', ..."""
    return _route_name(_lib.load().lmx_h_layernorm_route, _DT[in_dtype], _DT[out_dtype], rows, D, act)


def pooled_gemm_ok(M, N):
    """Shapes lmx_k_gemm's pooled-row mode (a_mode 2) is built for (the LDS-DMA kernel); smaller ones take GEMM + maxpool2."""
    return M >= 512 and N >= 96 and N % 8 == 0


def gemm(a, w, bias=None, act=ACT_NONE, scale=None, res=None, out=None, out_dtype=torch.float16, res_rows=0, pool_hw=None, a_rep=1,
         ln_out=None):
    """out[M,N] = res + scale * act(a[M,K] @ w[N,K]^T + bias)   (lmx_k_gemm, a_mode 0).
    a_rep > 1: w is [N, a_rep*K] and a's K columns are walked a_rep times (w = [whi | wlo]: f16 activations against 22-bit
    weights in one launch).
    res_rows > 0: res is a [res_rows, N] table broadcast over the batch (row m uses res[m % res_rows]).
    pool_hw=(H, W): the rows of `a` are an [n, H, W] token grid and the result is the 2 x 2 max-pool of the product over that
    grid, [M/4, N] in [n, H/2, W/2] order (a_mode 2: the bits of gemm(...) followed by maxpool2, without the full-size
    intermediate).
    act=ACT_SWIGLU: w [2I, K] and bias [2I] hold gate and up rows interleaved by 16 (lmx.dino.pack_gated); the result is
    scale * silu(gate) * up with N/2 = I columns (scale [I]); f16 out, no residual.
    ln_out=(h, gamma, beta, eps): the same launch also writes h = LayerNorm(out) as f16 [M, N] (gamma, beta f32 [N]) from the f32
    rows it stores — the bits of layernorm(out, gamma, beta, eps) without its pass over out.  A kernel of its own at every M, for
    an f32 result with a residual, N <= 448 and K <= 448 only (lmx_gemm_desc.ln_out, include/lmx.h); anything else raises."""
    dev = _dev(a, w, bias, scale, res, out, *(ln_out[:3] if ln_out is not None else ()))
    M, K, lda = _rows(a, "gemm A")
    N, K2, ldw = _rows(w, "gemm W")
    if K2 != a_rep * K or ldw != K2:
        raise LmxError(f"gemm: W must be contiguous [N,{a_rep}*K]; A K={K}, W shape {tuple(w.shape)}")
    if a.dtype != torch.float16 or w.dtype != torch.float16:
        raise LmxError("gemm: A and W must be float16")
    Mout = M // 4 if pool_hw else M
    Nout = N // 2 if act == ACT_SWIGLU else N
    if out is None:
        out = torch.empty((Mout, Nout), dtype=out_dtype, device=a.device)
    Mo, No, ldc = _rows(out, "gemm C")
    if (Mo, No) != (Mout, Nout):
        raise LmxError(f"gemm: out shape {tuple(out.shape)} != ({Mout},{Nout})")
    d = GemmDesc()
    d.A, d.W, d.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.scale = scale.data_ptr() if scale is not None else None
    d.lda, d.ldc, d.ldr = lda, ldc, 0
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N):
        raise LmxError("gemm: bias must be float32 [N]")
    if scale is not None and (scale.dtype != torch.float32 or scale.numel() != Nout):
        raise LmxError("gemm: scale must be float32 [N] (ACT_SWIGLU: [N/2])")
    if res is not None:
        Mr, Nr, ldr = _rows(res, "gemm res")
        if (Mr, Nr) != ((res_rows or M), N) or res.dtype != out.dtype:
            raise LmxError("gemm: residual must match out's shape and dtype")
        d.res, d.ldr = res.data_ptr(), ldr
    d.res_rows = res_rows
    d.M, d.N, d.K = M, N, a_rep * K
    d.act, d.out_dtype, d.a_mode, d.a_rep = act, _DT[out.dtype], 0, a_rep
    if pool_hw:
        d.a_mode, d.H, d.W_ = 2, int(pool_hw[0]), int(pool_hw[1])
    if ln_out is not None:
        h, g, b, eps = ln_out
        Mh, Nh, ldh = _rows(h, "gemm ln_out")
        if (Mh, Nh) != (Mout, Nout) or h.dtype != torch.float16:
            raise LmxError(f"gemm: ln_out must be float16 [{Mout},{Nout}], got {h.dtype} {tuple(h.shape)}")
        if any(t.dtype != torch.float32 or t.numel() != Nout or not t.is_contiguous() for t in (g, b)):
            raise LmxError("gemm: ln_out's gamma and beta must be contiguous float32 [N]")
        d.ln_out, d.ln_gamma, d.ln_beta, d.ld_ln, d.ln_eps = h.data_ptr(), g.data_ptr(), b.data_ptr(), ldh, float(eps)
    check(_lib.load().lmx_k_gemm(C.byref(d), _stream(dev)), "lmx_k_gemm")
    return out


def im2col_u8(img, lut, IH, IW, KH, KW, stride, pad, ldo):
    """u8 [n,rh,rw,3] at the top-left of an IH x IW zero canvas -> f16 [n*OH*OW, ldo] (lmx_k_im2col_u8)."""
    dev = _dev(img, lut)
    n, rh, rw, c = img.shape
    if c != 3 or img.dtype != torch.uint8 or not img.is_contiguous():
        raise LmxError("im2col_u8: img must be contiguous uint8 [n,h,w,3]")
    OH, OW = (IH + 2 * pad - KH) // stride + 1, (IW + 2 * pad - KW) // stride + 1
    out = torch.empty((n * OH * OW, ldo), dtype=torch.float16, device=img.device)
    check(_lib.load().lmx_k_im2col_u8(_ptr(img), _ptr(lut), _ptr(out), n, rh, rw, IH, IW, KH, KW, stride, pad, ldo,
                                      _stream(dev)), "lmx_k_im2col_u8")
    return out


def maxpool2(x, out):
    """2x2/s2 max pool, NHWC f16 or f32, channel slices allowed (lmx_k_maxpool2)."""
    dev = _dev(x, out)
    n, H, W, Cc, ps = _nhwc(x, "maxpool2 x")
    no, Ho, Wo, Co, pso = _nhwc(out, "maxpool2 out")
    if (no, Ho, Wo, Co) != (n, H // 2, W // 2, Cc) or x.dtype != out.dtype:
        raise LmxError("maxpool2: shape/dtype mismatch")
    check(_lib.load().lmx_k_maxpool2(_ptr(x), ps, _ptr(out), pso, _DT[x.dtype], n, H, W, Cc, _stream(dev)), "lmx_k_maxpool2")
    return out


def cast_f16(x, out=None):
    dev = _dev(x, out)
    rows, cols, lds = _rows(x, "cast src")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float16, device=x.device)
    check(_lib.load().lmx_k_cast_f32_f16(_ptr(x), lds, _ptr(out), out.stride(0), rows, cols, _stream(dev)),
          "lmx_k_cast_f32_f16")
    return out


def hiera_band(windows, q_strides, grid, nh, nw):
    """Stage-1 token rows of a Hiera trunk that depend on a frame resized to nh x nw on its 4 * grid canvas, 0 = no band
    (lmx_h_hiera_band, include/lmx.h: host arithmetic, no GPU).  windows / q_strides: the block plan, window 0 = global attention."""
    nb = len(windows)
    if nb != len(q_strides):
        raise LmxError("hiera_band: windows and q_strides must be the same length")
    band = C.c_int(0)
    check(_lib.load().lmx_h_hiera_band((C.c_int * nb)(*windows), (C.c_int * nb)(*q_strides), nb, grid, nh, nw, C.byref(band)),
          "lmx_h_hiera_band")
    return band.value


def hiera_bands(windows, q_strides, grid, nh, nw):
    """The same band sized block by block: (rows per block), the token rows of the grid each block reads that it has to run on; the
    whole grid from the first global block on, and everywhere where there is no band (lmx_h_hiera_bands, include/lmx.h)."""
    nb = len(windows)
    if nb != len(q_strides):
        raise LmxError("hiera_bands: windows and q_strides must be the same length")
    rows = (C.c_int * nb)()
    check(_lib.load().lmx_h_hiera_bands((C.c_int * nb)(*windows), (C.c_int * nb)(*q_strides), nb, grid, nh, nw, rows), "lmx_h_hiera_bands")
    return tuple(rows)


def _hiera_config(cfg):
    """lmx.sam.HieraConfig -> lmx_hiera_config_t."""
    c = _lib.HieraConfig()
    ns = len(cfg.blocks)
    if not (len(cfg.dims) == len(cfg.heads) == len(cfg.windows) == ns) or ns > c.MAX_STAGES or len(cfg.global_blocks) > c.MAX_GLOBAL \
            or len(cfg.fpn_top_down) > c.MAX_STAGES or len(cfg.pos_bkg) != 2:
        raise LmxError(f"hiera plan: a configuration of {ns} stages, {len(cfg.global_blocks)} global blocks does not fit lmx_hiera_config_t")
    c.hidden, c.n_stages, c.n_global, c.q_pool_stages, c.fpn_dim, c.n_top_down, c.image, c.eps = \
        cfg.hidden, ns, len(cfg.global_blocks), cfg.q_pool_stages, cfg.fpn_dim, len(cfg.fpn_top_down), cfg.image, cfg.eps
    for name in ("blocks", "dims", "heads", "windows", "global_blocks", "pos_bkg", "fpn_top_down"):
        for i, v in enumerate(getattr(cfg, name)):
            getattr(c, name)[i] = v
    return c


def _hiera_records(recs):
    return [tuple(getattr(r, f) for f, _ in _lib.HieraBlock._fields_) for r in recs]


def hiera_plan_rows_host(cfg, n, rows, lowest=0):
    """lmx_h_hiera_plan_rows (include/lmx.h): lmx.sam.hiera_plan(cfg, n, rows, lowest=lowest) of the default encoder as computed in C,
    one tuple of integers per block in lmx.sam.BlockPlan's field order (lmx.sam.native_plan turns them into BlockPlans)."""
    c = _hiera_config(cfg)
    nb = C.c_int(0)
    check(_lib.load().lmx_h_hiera_blocks(C.byref(c), C.byref(nb)), "lmx_h_hiera_blocks")
    if len(rows) != nb.value:
        raise LmxError(f"hiera_plan_rows_host: {len(rows)} row counts for {nb.value} blocks")
    recs = (_lib.HieraBlock * nb.value)()
    check(_lib.load().lmx_h_hiera_plan_rows(C.byref(c), n, (C.c_int * nb.value)(*rows), lowest, recs), "lmx_h_hiera_plan_rows")
    return _hiera_records(recs)


def hiera_plan_host(cfg, n, nh, nw, lowest=0):
    """lmx_h_hiera_plan (include/lmx.h): (the settled rows per block for n frames resized to nh x nw, the plan on them as tuples of
    integers as in hiera_plan_rows_host) — what HieraEncoder(band="blocks")._settle computes, in C."""
    c = _hiera_config(cfg)
    nb = C.c_int(0)
    check(_lib.load().lmx_h_hiera_blocks(C.byref(c), C.byref(nb)), "lmx_h_hiera_blocks")
    recs, rows = (_lib.HieraBlock * nb.value)(), (C.c_int * nb.value)()
    check(_lib.load().lmx_h_hiera_plan(C.byref(c), n, nh, nw, lowest, recs, rows), "lmx_h_hiera_plan")
    return tuple(rows), _hiera_records(recs)


def band_join(band, table, H):
    """[n, H, W, D]: rows < Hb of each image from band [n, Hb, W, D], rows >= Hb from table [(H - Hb) * W, D], the same for every
    image (lmx_k_band_join).  f16 or f32, contiguous."""
    dev = _dev(band, table)
    if band.dim() != 4 or table.dim() != 2 or not band.is_contiguous() or not table.is_contiguous():
        raise LmxError("band_join: band must be contiguous [n, Hb, W, D] and table contiguous [(H - Hb) * W, D]")
    n, Hb, W, D = band.shape
    if band.dtype not in _DT or table.dtype != band.dtype or tuple(table.shape) != ((H - Hb) * W, D):
        raise LmxError(f"band_join: table {table.dtype} {tuple(table.shape)} does not hold rows {Hb} .. {H - 1} of a {band.dtype} "
                       f"[{H}, {W}, {D}] grid")
    out = torch.empty((n, H, W, D), dtype=band.dtype, device=band.device)
    check(_lib.load().lmx_k_band_join(_ptr(band), _ptr(table), _ptr(out), _DT[band.dtype], n, H, Hb, W, D, _stream(dev)),
          "lmx_k_band_join")
    return out


def _nhwc(t, what):
    """[n,H,W,C] view of (a channel slice of) a dense NHWC buffer; returns (n,H,W,C,pixel_stride)."""
    if t.dim() != 4 or t.stride(3) != 1:
        raise LmxError(f"{what}: expected NHWC with contiguous channels, got {tuple(t.shape)} / {t.stride()}")
    n, H, W, Cc = t.shape
    ps = t.stride(2)
    if t.stride(1) != W * ps or (n > 1 and t.stride(0) != H * W * ps):
        raise LmxError(f"{what}: not a channel slice of a dense NHWC buffer: strides {t.stride()}")
    return n, H, W, Cc, ps


def split_k_for(px_per_frame, N, K, cin):
    """Split factor of an f32-output 3 x 3 convolution in the exact plan (lmx_k_gemm split_k): K = 27 Cin against a handful of
    256 x 256 tiles per frame leaves most of the 256 CUs idle at the reference schedule's 10 frames (M = 9600, N = 256, K = 6912:
    38 tiles, 122 us).  The factor is a function of the LAYER — pixels of ONE frame, N, K — never of the batch: the summation
    order, and so a frame's bits, must not depend on the batch the frame rides in.  1 = no split (also outside the LDS-DMA
    kernel's shapes)."""
    if N < 64 or N % 8 or cin % 32:
        return 1
    tiles1 = -(-px_per_frame // 256) * -(-N // 256)  # tiles one frame contributes
    nk = K // 64
    s = min(8, nk // 8, 32 // tiles1)
    return s if s >= 2 else 1


def conv3x3(x, w, bias=None, act=ACT_SILU, stride=1, res=None, out=None, scale=None, out_dtype=torch.float16, split_k=1):
    """3x3 / pad 1 convolution as implicit GEMM (lmx_k_gemm, a_mode 1).  x: NHWC f16 (may be a channel slice),
    w: f16 [Cout, 9*Cin] packed (ky,kx,ci); out: NHWC f16 or f32 (may be a channel slice of a wider buffer);
    scale: f32 [Cout] applied after bias + activation (the exact plan's power-of-two row scales)."""
    dev = _dev(x, w, bias, res, out, scale)
    n, H, W, Cin, ps = _nhwc(x, "conv3x3 x")
    Cout = w.shape[0]
    if w.dim() != 2 or w.shape[1] != 9 * Cin or not w.is_contiguous():
        raise LmxError(f"conv3x3: W must be contiguous [Cout, 9*Cin={9 * Cin}], got {tuple(w.shape)}")
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    parts = None
    if split_k > 1:  # S partial outputs [S, n, Ho, Wo, Cout] f32; the consumer (split3 nsum=S) adds them up
        if out is not None or res is not None or act != ACT_NONE or out_dtype != torch.float32:
            raise LmxError("conv3x3: split_k needs a fresh f32 output, no residual, no activation")
        parts = torch.empty((split_k, n, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
        out = parts[0]
    if out is None:
        out = torch.empty((n, Ho, Wo, Cout), dtype=out_dtype, device=x.device)
    no, Ho2, Wo2, Co2, pso = _nhwc(out, "conv3x3 out")
    if (no, Ho2, Wo2, Co2) != (n, Ho, Wo, Cout):
        raise LmxError(f"conv3x3: out shape {tuple(out.shape)} != {(n, Ho, Wo, Cout)}")
    d = GemmDesc()
    d.A, d.W, d.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    if scale is not None and (scale.dtype != torch.float32 or scale.numel() != Cout):
        raise LmxError("conv3x3: scale must be float32 [Cout]")
    d.scale = scale.data_ptr() if scale is not None else None
    d.lda, d.ldc, d.ldr = ps, pso, 0
    if res is not None:
        nr, Hr, Wr, Cr, psr = _nhwc(res, "conv3x3 res")
        if (nr, Hr, Wr, Cr) != (n, Ho, Wo, Cout) or res.dtype != out.dtype:
            raise LmxError("conv3x3: residual must match out")
        d.res, d.ldr = res.data_ptr(), psr
    d.M, d.N, d.K = n * Ho * Wo, Cout, 9 * Cin
    d.act, d.out_dtype, d.a_mode = act, _DT[out.dtype], 1
    d.H, d.W_, d.Cin, d.conv_stride, d.Ho, d.Wo = H, W, Cin, stride, Ho, Wo
    if parts is not None:
        d.split_k, d.split_stride = split_k, parts.stride(0)
    check(_lib.load().lmx_k_gemm(C.byref(d), _stream(dev)), "lmx_k_gemm(conv3x3)")
    return out if parts is None else parts


def conv1x1(x, w, bias=None, act=ACT_SILU, res=None, out=None, out_dtype=torch.float16, scale=None):
    """1x1 convolution = GEMM over the pixels of an NHWC tensor (channel slices allowed on both sides)."""
    n, H, W, Cin, ps = _nhwc(x, "conv1x1 x")
    a = x.as_strided((n * H * W, Cin), (ps, 1))
    Cout = w.shape[0]
    if out is None:
        out = torch.empty((n, H, W, Cout), dtype=out_dtype, device=x.device)
    no, Ho, Wo, Co, pso = _nhwc(out, "conv1x1 out")
    o2 = out.as_strided((n * H * W, Cout), (pso, 1))
    r2 = None
    if res is not None:
        nr, Hr, Wr, Cr, psr = _nhwc(res, "conv1x1 res")
        r2 = res.as_strided((n * H * W, Cout), (psr, 1))
    gemm(a, w, bias=bias, act=act, res=r2, out=o2, scale=scale)
    return out


def layernorm(x, gamma, beta, eps, out=None, out_dtype=torch.float16, act=ACT_NONE):
    dev = _dev(x, gamma, beta, out)
    rows, D, ldx = _rows(x, "layernorm x")
    if out is None:
        out = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    r2, D2, ldy = _rows(out, "layernorm y")
    if (r2, D2) != (rows, D):
        raise LmxError("layernorm: out shape mismatch")
    check(_lib.load().lmx_k_layernorm(_ptr(x), _DT[x.dtype], ldx, _ptr(gamma), _ptr(beta), _ptr(out), _DT[out.dtype],
                                      ldy, rows, D, float(eps), act, _stream(dev)), "lmx_k_layernorm")
    return out


def pack_bits(mask):
    """u8 [..., h, w] (0 / non-0) -> u8 [..., h, ceil(w/8)], numpy.packbits bit order."""
    dev = _dev(mask)
    if mask.dtype not in (torch.uint8, torch.bool) or not mask.is_contiguous():
        raise LmxError("pack_bits: contiguous uint8 / bool tensor expected")
    w = mask.shape[-1]
    rows = mask.numel() // w
    out = torch.empty(tuple(mask.shape[:-1]) + ((w + 7) // 8,), dtype=torch.uint8, device=mask.device)
    check(_lib.load().lmx_k_pack_bits(_ptr(mask), rows, w, _ptr(out), _stream(dev)), "lmx_k_pack_bits")
    return out


YUV_LAYOUTS = {"nv12": 0, "i420": 1}  # LMX_YUV_NV12, LMX_YUV_I420
YUV_MATRICES = {"bt601": 0, "bt709": 1}  # LMX_YUV_BT601, LMX_YUV_BT709


def yuv_frames(y, c, h, w, layout="nv12", matrix="bt601", v=None):
    """(lmx_yuv_frames_t, n, device) of decoder frames held in uint8 device tensors, pitches and frame strides taken from the
    tensors' strides: y [n, >= h, >= w] (or [rows, cols]: one frame), c the interleaved U V plane [n, >= h/2, >= w] (nv12) or the U
    plane [n, >= h/2, >= w/2] with `v` the V plane of the same strides (i420).  Rows are contiguous; everything else is free: a
    pitched surface is a slice of a wider tensor, a plane at any address a slice of a byte buffer."""
    if layout not in YUV_LAYOUTS or matrix not in YUV_MATRICES:
        raise LmxError(f"yuv_frames: layout {layout!r} / matrix {matrix!r}: one of {tuple(YUV_LAYOUTS)} and one of {tuple(YUV_MATRICES)}")
    planes = [("y", y, h, w), ("c", c, h // 2, w if layout == "nv12" else w // 2)]
    if (v is not None) != (layout == "i420"):
        raise LmxError("yuv_frames: i420 takes the V plane in v, nv12 takes none")
    if v is not None:
        planes.append(("v", v, h // 2, w // 2))
    dev = _dev(y, c, v)
    views = []
    for name, t, rows, cols in planes:
        t = t.unsqueeze(0) if t.dim() == 2 else t
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[1] < rows or t.shape[2] < cols or (t.shape[2] > 1 and t.stride(2) != 1):
            raise LmxError(f"yuv_frames: {name} must be uint8 [n, >= {rows}, >= {cols}] with contiguous rows, got {tuple(t.shape)} strides {t.stride()}")
        views.append(t)
    n = views[0].shape[0]
    if any(t.shape[0] != n for t in views):
        raise LmxError("yuv_frames: the planes hold different numbers of frames")
    if v is not None and views[1].stride() != views[2].stride():
        raise LmxError("yuv_frames: the U and the V plane must have the same pitch and frame stride")
    # an empty tensor has no address; n = 0 follows no pointer, and the V plane's says "there is one"
    ptrs = [_ptr(t) if t.numel() else C.c_void_p(_ROUTE_PTR) for t in views]
    f = _lib.YuvFrames(ptrs[0], ptrs[1], ptrs[2] if v is not None else None, views[0].stride(1), views[1].stride(1),
                       views[0].stride(0), views[1].stride(0), YUV_LAYOUTS[layout], YUV_MATRICES[matrix])
    return f, n, dev


def yuv420_to_bgr(y, c, h, w, layout="nv12", matrix="bt601", v=None, out=None):
    """NV12 / I420 frames (yuv_frames' tensors) -> BGR u8 [n,h,w,3] (lmx_k_yuv420_to_bgr, csrc/yuv.hip): limited range, 20-bit fixed
    point, nearest chroma.  `out`: a contiguous uint8 [n,h,w,3] tensor at any address."""
    f, n, dev = yuv_frames(y, c, h, w, layout, matrix, v)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous() or out.device != dev:
        raise LmxError(f"yuv420_to_bgr: out must be a contiguous uint8 [{n},{h},{w},3] tensor on {dev}")
    check(_lib.load().lmx_k_yuv420_to_bgr(C.byref(f), n, int(h), int(w), _ptr(out), _stream(dev)), "lmx_k_yuv420_to_bgr")
    return out


def yuv420_to_bgr_roi(y, c, h, w, roi, layout="nv12", matrix="bt601", v=None, out=None):
    """The window roi = (x, y, w, h) of NV12 / I420 frames of h x w (yuv_frames' tensors) -> BGR u8 [n, roi h, roi w, 3]
    (lmx_k_yuv420_to_bgr_roi, csrc/yuv.hip): pixel (i, j) of the window is pixel (x + i, y + j) of yuv420_to_bgr, at any parity of the
    window; the full-frame window gives yuv420_to_bgr's bytes.  `out`: a contiguous uint8 [n, roi h, roi w, 3] tensor at any address."""
    f, n, dev = yuv_frames(y, c, h, w, layout, matrix, v)
    rx, ry, rw, rh = (int(t) for t in roi)
    rect = _lib.Rect(rx, ry, rw, rh)
    shape = (n, max(rh, 0), max(rw, 0), 3)  # an empty or outside window is refused by the call, with its message
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise LmxError(f"yuv420_to_bgr_roi: out must be a contiguous uint8 {list(shape)} tensor on {dev}")
    check(_lib.load().lmx_k_yuv420_to_bgr_roi(C.byref(f), n, int(h), int(w), C.byref(rect), _ptr(out) if out.numel() else C.c_void_p(_ROUTE_PTR),
                                              _stream(dev)), "lmx_k_yuv420_to_bgr_roi")
    return out


def bgr_to_yuv420(frames, layout="nv12", matrix="bt601", out=None):
    """BGR u8 [n,h,w,3] -> what an encoder takes (lmx_k_bgr_to_yuv420, csrc/yuv.hip): (y [n,h,w], c [n,h/2,w]) for nv12, (y, u, v) with
    u, v [n,h/2,w/2] for i420; limited range, 20-bit fixed point, chroma from the 2 x 2 sums.  The source's row pitch and frame stride
    are the tensor's strides, so a window `frames[:, y0:y1, x0:x1]` of larger frames is converted where it lies, without a copy; pixels
    are packed (strides 3 and 1).  `out`: the planes to write, uint8 with contiguous rows and any pitch, stride and address (u and v with
    the same strides); h and w are even."""
    if layout not in YUV_LAYOUTS or matrix not in YUV_MATRICES:
        raise LmxError(f"bgr_to_yuv420: layout {layout!r} / matrix {matrix!r}: one of {tuple(YUV_LAYOUTS)} and one of {tuple(YUV_MATRICES)}")
    dev = _dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or (frames.numel() and (frames.stride(3) != 1 or frames.stride(2) != 3)):
        raise LmxError(f"bgr_to_yuv420: frames must be uint8 [n,h,w,3] with packed pixels, got {frames.dtype} {tuple(frames.shape)} strides {frames.stride()}")
    n, h, w, _ = frames.shape
    shapes = [(n, h, w), (n, h // 2, w)] if layout == "nv12" else [(n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)]
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in shapes)
    out = tuple(out)
    if len(out) != len(shapes) or any(t.dtype != torch.uint8 or tuple(t.shape) != s or t.device != dev or (t.shape[2] > 1 and t.stride(2) != 1)
                                      for t, s in zip(out, shapes)):
        raise LmxError(f"bgr_to_yuv420: out must be {len(shapes)} uint8 planes {shapes} with contiguous rows on {dev}")
    if layout == "i420" and out[1].stride() != out[2].stride():
        raise LmxError("bgr_to_yuv420: the U and the V plane must have the same pitch and frame stride")
    ptrs = [_ptr(t) if t.numel() else C.c_void_p(_ROUTE_PTR) for t in out]
    o = _lib.YuvOut(ptrs[0], ptrs[1], ptrs[2] if layout == "i420" else None, out[0].stride(1), out[1].stride(1), out[0].stride(0), out[1].stride(0),
                    YUV_LAYOUTS[layout], YUV_MATRICES[matrix])
    src = _ptr(frames) if frames.numel() else C.c_void_p(_ROUTE_PTR)
    check(_lib.load().lmx_k_bgr_to_yuv420(src, frames.stride(1), frames.stride(0), n, h, w, C.byref(o), _stream(dev)), "lmx_k_bgr_to_yuv420")
    return out


def frame_quality(frames, out=None):
    """BGR u8 [n,h,w,3] -> int64 [n,4] = per frame (Σ g, Σ lap, Σ lap², h * w) of the 8-bit gray image and its ksize-1 Laplacian under
    BORDER_REFLECT_101 (lmx_k_frame_quality, csrc/quality.hip): exact integer sums, what lmx.services.curation.visual_scores turns into
    the blur and brightness scores of clip-curation main.py:276-289.  `frames` is contiguous and may start at any byte address (a view
    into a byte buffer); `out`: a contiguous int64 [n,4] tensor, which needs no clearing."""
    dev = _dev(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise LmxError(f"frame_quality: frames must be contiguous uint8 [n,h,w,3], got {frames.dtype} {tuple(frames.shape)} strides {frames.stride()}")
    n, h, w, _ = frames.shape
    if out is None:
        out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n, 4) or not out.is_contiguous() or out.device != dev:
        raise LmxError(f"frame_quality: out must be a contiguous int64 [{n},4] tensor on {dev}")
    lib = _lib.load()
    nws = int(lib.lmx_frame_quality_workspace_bytes(n, h, w))
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev) if nws > 0 else None
    check(lib.lmx_k_frame_quality(_ptr(frames), n, h, w, _ptr(out), _ptr(ws), _stream(dev)), "lmx_k_frame_quality")
    return out


# ---- the vector store (include/lmx.h "Vector store", csrc/vstore.hip) ---------------------------------------------------------------
VSTORE_DT = {torch.float32: 1, torch.float64: 2}  # LMX_VSTORE_F32, LMX_VSTORE_F64


def unit_rows(raw, out=None):
    """raw f32 or f64 [n,D], contiguous -> f32 unit rows [n,D] (lmx_k_unit_rows): the sum of squares in double in the pinned 256-partial
    order, (float)((double)x / (sqrt(ss) + 1e-8)).  `out`: a [n,D] f32 view whose rows are contiguous (a slice of a gallery)."""
    dev = _dev(raw, out)
    if raw.dim() != 2 or not raw.is_contiguous() or raw.dtype not in VSTORE_DT:
        raise LmxError(f"unit_rows: raw must be a contiguous f32 or f64 [n,D] tensor, got {raw.dtype} {tuple(raw.shape)} strides {raw.stride()}")
    n, D = raw.shape
    if out is None:
        out = torch.empty((n, D), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (n, D) or _rows(out, "unit_rows out")[2] < D:
        raise LmxError(f"unit_rows: out must be an f32 [{n},{D}] tensor with contiguous rows")
    check(_lib.load().lmx_k_unit_rows(_ptr(raw), VSTORE_DT[raw.dtype], n, D, _ptr(out), out.stride(0) if n > 1 else D, _stream(dev)), "lmx_k_unit_rows")
    return out


def cosine_topk(gallery, queries, k, limits=None):
    """gallery f32 unit rows [N,D] (rows contiguous, any row stride that is a multiple of 4), queries f32 unit rows [Q,D], limits None or
    int32 [Q] -> (scores f32 [Q,k], slots int32 [Q,k]) by lmx_k_cosine_topk: per query the k best of the slots [0, limits[q]) in descending
    score, exact ties to the lower slot, slot -1 / score 0 past the visible rows."""
    dev = _dev(gallery, queries, limits)
    if gallery.dtype != torch.float32 or queries.dtype != torch.float32 or queries.dim() != 2 or not queries.is_contiguous():
        raise LmxError(f"cosine_topk: f32 gallery and contiguous f32 queries [Q,D], got {gallery.dtype} and {queries.dtype} {tuple(queries.shape)}")
    N, D, ldg = _rows(gallery, "cosine_topk gallery")
    Q = queries.shape[0]
    if queries.shape[1] != D:
        raise LmxError(f"cosine_topk: queries of {queries.shape[1]} elements against rows of {D}")
    if limits is not None and (limits.dtype != torch.int32 or tuple(limits.shape) != (Q,) or not limits.is_contiguous()):
        raise LmxError(f"cosine_topk: limits must be a contiguous int32 [{Q}] tensor")
    lib = _lib.load()
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    slots = torch.empty((Q, k), dtype=torch.int32, device=dev)
    nws = int(lib.lmx_h_cosine_topk_workspace(N, Q, k))
    ws = torch.empty((max(nws, 8),), dtype=torch.uint8, device=dev)
    check(lib.lmx_k_cosine_topk(_ptr(gallery), N, D, ldg if N > 1 else max(ldg, D), _ptr(queries), Q, _ptr(limits), k, _ptr(scores), _ptr(slots),
                                _ptr(ws), _stream(dev)), "lmx_k_cosine_topk")
    return scores, slots


# ---- the weight tables of the TCN, the gait transformer, the graph transformer and GraphGPS -------------------------------------------
# Which tensors a configuration calls for, their names, shapes and the pointer of lmx_<model>_weights_t each one fills, and which
# configurations are accepted at all, are stated once, in the library (include/lmx.h lmx_h_<model>_tensors; csrc/weights_table.h).
def _model_config(Struct, who, ints):
    """Struct (a lmx_<model>_weights_t) with the integers of `ints`, {field: an int, or a tuple for an array field}, and null pointers.
    ctypes cuts a value that does not fit an int32 field without a word, so such a value is refused here; so are more blocks than
    `channels`, the one array field, has entries."""
    w = Struct()
    for name, v in ints.items():
        if isinstance(v, tuple) and len(v) > len(getattr(w, name)):
            raise LmxError(f"{who}: n_blocks {len(v)} outside 1 .. {len(getattr(w, name))}")
        for x in v if isinstance(v, tuple) else (v,):
            if int(x) != x or not -2 ** 31 <= x < 2 ** 31:
                raise LmxError(f"{who}: {name} {x} is not an int32")
        if isinstance(v, tuple):
            getattr(w, name)[:len(v)] = [int(x) for x in v]
        else:
            setattr(w, name, int(v))
    return w


def _ints(Struct, *values):
    """{field: value} where the arguments come in the order of the struct's leading int32 fields (xfm, gfm, gnn)"""
    return dict(zip((n for n, _ in Struct._fields_), values))


def _model_rows(model, who, w):
    """lmx_h_<model>_tensors for the configuration in `w`: [(name, shape, pointer_at)] in the order of the weight image and of
    pack_tensors.  A configuration outside the list of include/lmx.h is refused in the library's words, `who` in front, the field named."""
    lib, n = _lib.load(), C.c_int(0)
    fn = getattr(lib, f"lmx_h_{model}_tensors")
    if fn(who.encode(), C.byref(w), None, 0, C.byref(n)):  # the check and the count
        raise LmxError(lib.lmx_last_error().decode("utf-8", "replace"))
    rows = (_lib.TensorRow * n.value)()
    check(fn(who.encode(), C.byref(w), rows, len(rows), C.byref(n)), f"lmx_h_{model}_tensors")
    return [(r.name.decode(), tuple(r.shape[:r.rank]), r.pointer_at) for r in rows]


def _model_shapes(model, Struct, who, ints):
    """ordered {tensor name: shape} of one network"""
    return {name: shape for name, shape, _ in _model_rows(model, who, _model_config(Struct, who, ints))}


def _model_weights(model, Struct, who, ints, tensors):
    """lmx_<model>_weights_t over packed f32 tensors (all on one GPU for the device forward, all on the CPU for the host forward): every
    tensor of the table must be there, contiguous float32 of the table's shape, and its address goes where the table says.  The
    struct keeps the tensors alive."""
    w = _model_config(Struct, who, ints)
    rows = _model_rows(model, who, w)
    devs = {t.device for t in tensors.values()}
    if len(devs) != 1:
        raise LmxError(f"{who}: tensors on different devices ({sorted(map(str, devs))})")
    for name, shape, at in rows:
        t = tensors.get(name)
        if t is None or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise LmxError(f"{who}: {name} must be a contiguous float32 tensor of shape {shape}, got "
                           f"{None if t is None else (t.dtype, tuple(t.shape))}")
        C.c_void_p.from_address(C.addressof(w) + at).value = t.data_ptr()
    w._tensors, w._device = dict(tensors), devs.pop()
    return w


# ---- the TCN gait model (include/lmx.h "The TCN gait model"; csrc/tcn.hip, csrc/host_tcn.cpp) ---------------------------------------
TCN_MAX_T = 256


def tcn_keep_bits(seed, sample, site, n_sites, count, p):
    """uint8 numpy [count]: the keep decisions of MC dropout for one (seed, sample, site) as include/lmx.h pins them
    (lmx_h_tcn_keep_bits; host arithmetic, no GPU)."""
    import numpy as np

    keep = np.empty((int(count),), np.uint8)
    check(_lib.load().lmx_h_tcn_keep_bits(int(seed) & (2 ** 64 - 1), int(sample), int(site), int(n_sites), int(count), float(p),
                                           keep.ctypes.data), "lmx_h_tcn_keep_bits")
    return keep


def _tcn_ints(input_dim, channels, k, head):
    return {"input_dim": input_dim, "n_blocks": len(channels), "k": k, "head": head, "channels": tuple(channels)}


def tcn_check_config(who, input_dim, channels, k, head):
    """The list of include/lmx.h, refused by the library itself: LmxError names the field."""
    _model_rows("tcn", who, _model_config(_lib.TcnWeights, who, _tcn_ints(input_dim, channels, k, head)))


def tcn_tensor_shapes(input_dim, channels, k, head):
    """Ordered {tensor name: shape} of one network: the names of the weight image (csrc/tcn_image.h) and of lmx.tcn.pack_tensors."""
    return _model_shapes("tcn", _lib.TcnWeights, "tcn_tensor_shapes", _tcn_ints(input_dim, channels, k, head))


def tcn_weights(input_dim, channels, k, head, tensors):
    """lmx_tcn_weights_t over the packed f32 tensors of lmx.tcn.pack_tensors (all on one GPU for tcn_forward, all on the CPU for
    tcn_forward_host).  The struct keeps the tensors alive.  Configurations outside the list of include/lmx.h are refused here with
    the field named, as the library refuses them."""
    return _model_weights("tcn", _lib.TcnWeights, "tcn_weights", _tcn_ints(input_dim, channels, k, head), tensors)


def _check_samples(who, S, p):
    """S and p as every MC-dropout forward takes them"""
    if S == 1 or S < 0 or S > 65535:
        raise LmxError(f"{who}: S {S} (0: eval mode; 2 .. 65535 samples; the standard deviation of 1 is undefined)")
    if S and not 0.0 <= p < 1.0:
        raise LmxError(f"{who}: p {p} outside [0, 1)")


def pack_seeds(seeds):
    """the low 64 bits of every seed (ints of either sign) as a contiguous uint64 numpy array: HOST memory, as the library reads them"""
    import numpy as np

    return np.ascontiguousarray(np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64))


def _gait_args(who, w, x, mask, seeds, n_samples, p, saliency, max_T, limit=""):
    """(n, T, S, the seeds as a uint64 numpy array or None) after the checks every forward of a gait model shares; `limit` words
    T's bound as the library does."""
    import numpy as np

    if x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != w.input_dim or not x.is_contiguous():
        raise LmxError(f"{who}: x must be a contiguous float32 [n, T, {w.input_dim}] tensor, got {x.dtype} {tuple(x.shape)} strides {x.stride()}")
    n, T, S = int(x.shape[0]), int(x.shape[1]), int(n_samples)
    if not 1 <= T <= max_T:
        raise LmxError(f"{who}: T {T} outside 1 .. {limit}{max_T}")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (n, T) or not mask.is_contiguous() or mask.device != x.device):
        raise LmxError(f"{who}: mask must be a contiguous uint8 [{n}, {T}] tensor on {x.device} (nonzero = masked), got {mask.dtype} "
                       f"{tuple(mask.shape)} on {mask.device}")
    if saliency and S:
        raise LmxError(f"{who}: saliency is read in eval mode only, S = {S}")
    _check_samples(who, S, p)
    if S == 0:
        return n, T, S, None
    if seeds is None:
        raise LmxError(f"{who}: S = {S} needs one seed per clip")
    if isinstance(seeds, torch.Tensor):
        if seeds.is_cuda or seeds.dtype != torch.int64:
            raise LmxError(f"{who}: seeds are HOST memory: a CPU int64 tensor, a numpy uint64 array or a list of ints")
        seeds = seeds.numpy().view(np.uint64)
    sd = pack_seeds(seeds) if isinstance(seeds, (list, tuple)) else np.ascontiguousarray(seeds)
    if sd.dtype != np.uint64 or sd.shape != (n,):
        raise LmxError(f"{who}: seeds must be {n} 64-bit values, got {sd.dtype} {sd.shape}")
    return n, T, S, sd


def _gait_forward(model, host, w, x, mask, seeds, n_samples, p, saliency, trunk):
    """What tcn_forward, tcn_forward_host, xfm_forward and xfm_forward_host share: the checks, pred / stats / saliency / trunk allocated
    where x lives, and the call of lmx_k_<model>_forward (device: with a seed workspace, on torch's stream) or lmx_h_<model>_forward
    (host).  Returns (pred, stats, saliency or None, trunk or None); only the transformer takes a mask and gives a saliency."""
    xfm = model == "xfm"
    who = f"{model}_forward_host" if host else f"{model}_forward"
    if host:
        if x.is_cuda or w._device.type != "cpu":
            raise LmxError(f"{who} takes CPU tensors and CPU weights")
        dev = torch.device("cpu")
    else:
        dev = _dev(x)
        if w._device != dev:
            raise LmxError(f"{who}: the weights are on {w._device}, x is on {dev}")
    n, T, S, sd = _gait_args(who, w, x, mask, seeds, n_samples, p, saliency, *((w.max_len, "max_len ") if xfm else (TCN_MAX_T,)))
    smax = max(S, 1)
    pred = torch.empty((n, smax), dtype=torch.float32, device=dev)
    stats = torch.empty((n, 2), dtype=torch.float32, device=dev)
    sal = torch.empty((n, T), dtype=torch.float32, device=dev) if saliency else None
    tr = torch.empty((n, smax, T, w.d_model if xfm else w.channels[w.n_blocks - 1]), dtype=torch.float32, device=dev) if trunk else None
    lib, name = _lib.load(), f"lmx_{'h' if host else 'k'}_{model}_forward"
    args = [C.byref(w), _ptr(x)] + [_ptr(mask)] * xfm + [C.c_void_p(sd.ctypes.data if sd is not None else 0), n, T, S, float(p), _ptr(pred),
                                                          _ptr(stats)] + [_ptr(sal)] * xfm + [_ptr(tr)]
    if not host:
        ws = torch.empty((max(int(getattr(lib, f"lmx_{model}_workspace_bytes")(n)), 8) // 8,), dtype=torch.int64, device=dev)
        args += [_ptr(ws), _stream(dev)]
    check(getattr(lib, name)(*args), name)
    return pred, stats, sal, tr


def tcn_forward(w, x, seeds, n_samples, p, trunk=False):
    """The whole TCN for n clips and S samples in ONE launch (lmx_k_tcn_forward, csrc/tcn.hip): x f32 [n, T, input_dim] on the device,
    seeds: n 64-bit values on the host -> (pred f32 [n, max(S, 1)], stats f32 [n, 2] = mean and unbiased std, trunk f32
    [n, max(S, 1), T, C] or None).  S = 0 is eval mode; S = 1 is refused.  `w`: tcn_weights over device tensors."""
    pred, stats, _, tr = _gait_forward("tcn", False, w, x, None, seeds, n_samples, p, False, trunk)
    return pred, stats, tr


def tcn_forward_host(w, x, seeds, n_samples, p, trunk=False):
    """lmx_h_tcn_forward: the same network in plain C++ on CPU tensors, with the same keep bits (no GPU).  `w`: tcn_weights over CPU
    tensors; returns CPU tensors."""
    pred, stats, _, tr = _gait_forward("tcn", True, w, x, None, seeds, n_samples, p, False, trunk)
    return pred, stats, tr


def tcn_features(keypoints, n_kp, bbox, target=125):
    """lmx_h_tcn_features: keypoints f64 [T0, 20, 2], n_kp int32 [T0], bbox f64 [T0, 4] (numpy) -> f32 numpy [target, 44]."""
    import numpy as np

    kp, nk, bb = (np.ascontiguousarray(keypoints, np.float64), np.ascontiguousarray(n_kp, np.int32), np.ascontiguousarray(bbox, np.float64))
    T0 = len(nk)
    if kp.shape != (T0, 20, 2) or bb.shape != (T0, 4):
        raise LmxError(f"tcn_features: keypoints {kp.shape} / bbox {bb.shape} for {T0} frames")
    out = np.empty((int(target), 44), np.float32)
    check(_lib.load().lmx_h_tcn_features(kp.ctypes.data, nk.ctypes.data, bb.ctypes.data, T0, int(target), out.ctypes.data), "lmx_h_tcn_features")
    return out


# ---- the gait transformer (include/lmx.h "The gait transformer"; csrc/xfm.hip, csrc/host_xfm.cpp) -------------------------------------
def xfm_check_config(who, input_dim, d_model, n_heads, n_layers, ff, head, max_len):
    """The list of include/lmx.h, refused by the library itself: LmxError names the field."""
    _model_rows("xfm", who, _model_config(_lib.XfmWeights, who, _ints(_lib.XfmWeights, input_dim, d_model, n_heads, n_layers, ff, head, max_len)))


def xfm_tensor_shapes(input_dim, d_model, n_heads, n_layers, ff, head, max_len):
    """Ordered {tensor name: shape} of one network: the names of the weight image (csrc/xfm_image.h) and of lmx.xfm.pack_tensors."""
    return _model_shapes("xfm", _lib.XfmWeights, "xfm_tensor_shapes", _ints(_lib.XfmWeights, input_dim, d_model, n_heads, n_layers, ff, head, max_len))


def xfm_weights(input_dim, d_model, n_heads, n_layers, ff, head, max_len, tensors):
    """lmx_xfm_weights_t over the packed f32 tensors of lmx.xfm.pack_tensors (all on one GPU for xfm_forward, all on the CPU for
    xfm_forward_host).  The struct keeps the tensors alive.  Configurations outside the list of include/lmx.h are refused here with
    the field named, as the library refuses them."""
    return _model_weights("xfm", _lib.XfmWeights, "xfm_weights", _ints(_lib.XfmWeights, input_dim, d_model, n_heads, n_layers, ff, head, max_len),
                          tensors)


def xfm_forward(w, x, mask, seeds, n_samples, p, saliency=False, trunk=False):
    """The whole gait transformer for n clips and S samples in ONE launch (lmx_k_xfm_forward, csrc/xfm.hip): x f32 [n, T, input_dim] and
    mask (None or uint8 [n, T], nonzero = masked) on the device, seeds: n 64-bit values on the host -> (pred f32 [n, max(S, 1)], stats f32
    [n, 2] = mean and unbiased std, saliency f32 [n, T] or None (S = 0 only), trunk f32 [n, max(S, 1), T, D] or None)."""
    return _gait_forward("xfm", False, w, x, mask, seeds, n_samples, p, saliency, trunk)


def xfm_forward_host(w, x, mask, seeds, n_samples, p, saliency=False, trunk=False):
    """lmx_h_xfm_forward: the same network in plain C++ on CPU tensors, with the same keep bits (no GPU).  `w`: xfm_weights over CPU
    tensors; returns CPU tensors."""
    return _gait_forward("xfm", True, w, x, mask, seeds, n_samples, p, saliency, trunk)


def xfm_mask(kp_conf, n_kp, det_conf, target=125):
    """lmx_h_xfm_mask: keypoint confidences f64 [T0, 20], n_kp int32 [T0], detection confidences f64 [T0] (numpy) -> uint8 numpy [target],
    1 = masked."""
    import numpy as np

    kc, nk, dc = (np.ascontiguousarray(kp_conf, np.float64), np.ascontiguousarray(n_kp, np.int32), np.ascontiguousarray(det_conf, np.float64))
    T0 = len(nk)
    if kc.shape != (T0, 20) or dc.shape != (T0,):
        raise LmxError(f"xfm_mask: confidences {kc.shape} / detection confidences {dc.shape} for {T0} frames")
    out = np.empty((int(target),), np.uint8)
    check(_lib.load().lmx_h_xfm_mask(kc.ctypes.data, nk.ctypes.data, dc.ctypes.data, T0, int(target), out.ctypes.data), "lmx_h_xfm_mask")
    return out


# ---- pose series (include/lmx.h "Pose series"; csrc/tleap.hip, csrc/host_tleap.cpp) ----------------------------------------------------
TLEAP_TRAINED, TLEAP_HEURISTIC = 0, 1


def tleap_record_dtype():
    """lmx_tleap_record_t as a numpy structured dtype (536 bytes)."""
    import numpy as np

    return np.dtype([("frame", "<i4"), ("det", "<i4"), ("bbox", "<f8", (4,)), ("confidence", "<f8"), ("n_kp", "<i4"), ("reserved", "<i4"),
                     ("keypoints", "<f8", (20, 3))])


def tleap_series(boxes, scores, cls, counts, kpts, hw, clip_first, target=125, cow_classes=(), host=False):
    """lmx_k_tleap_series (host=True: lmx_h_tleap_series on CPU tensors): the detector's outputs boxes f32 [F, max_det, 4], scores f32
    [F, max_det], cls i32 [F, max_det], counts i32 [F] and kpts f32 [F, max_det, K, ndim] (None: the heuristic mode over `cow_classes`)
    for n clips, clip c owning frames clip_first[c] .. clip_first[c + 1] -> (rows i32 [n], records uint8 [F * max_det, 536] to view with
    tleap_record_dtype, series f32 [n, target, 44], mask uint8 [n, target]).  ONE launch; tensors stay where the operands are."""
    import numpy as np

    ops = [boxes, scores, cls, counts] + ([kpts] if kpts is not None else [])
    if host:
        if any(t.is_cuda for t in ops):
            raise LmxError("tleap_series(host=True) takes CPU tensors")
        dev = torch.device("cpu")
    else:
        dev = _dev(*ops)
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise LmxError(f"tleap_series: boxes of shape {tuple(boxes.shape)}, not [F, max_det, 4]")
    F, max_det = int(boxes.shape[0]), int(boxes.shape[1])
    want = {"boxes": (boxes, torch.float32, (F, max_det, 4)), "scores": (scores, torch.float32, (F, max_det)),
            "cls": (cls, torch.int32, (F, max_det)), "counts": (counts, torch.int32, (F,))}
    K, ndim = 0, 0
    if kpts is not None:
        if kpts.dim() != 4:
            raise LmxError(f"tleap_series: kpts of shape {tuple(kpts.shape)}, not [F, max_det, K, ndim]")
        K, ndim = int(kpts.shape[2]), int(kpts.shape[3])
        want["kpts"] = (kpts, torch.float32, (F, max_det, K, ndim))
    for name, (t, dt, shape) in want.items():
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise LmxError(f"tleap_series: {name} is {t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}, expected {dt} {shape}")
    first = np.ascontiguousarray(clip_first, np.int32)
    if first.ndim != 1 or len(first) < 2:
        raise LmxError("tleap_series: clip_first holds the n + 1 bounds of n >= 1 clips")
    n, target = len(first) - 1, int(target)
    cow = np.ascontiguousarray(list(cow_classes), np.int32)
    rows = torch.empty((n,), dtype=torch.int32, device=dev)
    records = torch.empty((max(F * max_det, 1), 536), dtype=torch.uint8, device=dev)
    series = torch.empty((n, max(target, 1), 44), dtype=torch.float32, device=dev)
    mask = torch.empty((n, max(target, 1)), dtype=torch.uint8, device=dev)
    h, w = hw
    lib = _lib.load()
    args = [_ptr(boxes), _ptr(scores), _ptr(cls), _ptr(counts), _ptr(kpts), K, ndim, F, max_det, int(h), int(w), C.c_void_p(first.ctypes.data), n,
            target, TLEAP_TRAINED if kpts is not None else TLEAP_HEURISTIC, C.c_void_p(cow.ctypes.data if len(cow) else 0), len(cow), _ptr(rows),
            _ptr(records), _ptr(series), _ptr(mask)]
    if host:
        check(lib.lmx_h_tleap_series(*args), "lmx_h_tleap_series")
    else:
        ws = torch.empty((max(int(lib.lmx_tleap_workspace_bytes(F, max_det)), 8) // 8,), dtype=torch.int64, device=dev)
        check(lib.lmx_k_tleap_series(*args, _ptr(ws), _stream(dev)), "lmx_k_tleap_series")
    return rows, records, series, mask


def tleap_locomotion(records, names):
    """lmx_h_tleap_locomotion: a clip's records (numpy, tleap_record_dtype) and the 20 slot names -> {key: float} with the keys the
    reference would have set, in its order."""
    import numpy as np

    rec = np.ascontiguousarray(records, tleap_record_dtype())
    if len(names) != 20:
        raise LmxError(f"tleap_locomotion: {len(names)} names for 20 keypoint slots")
    arr = (C.c_char_p * 20)(*[str(n).encode() for n in names])
    out = _lib.TleapLocomotion()
    check(_lib.load().lmx_h_tleap_locomotion(C.c_void_p(rec.ctypes.data if len(rec) else 0), len(rec), arr, C.byref(out)), "lmx_h_tleap_locomotion")
    return {k: float(getattr(out, k)) for i, k in enumerate(_lib.TleapLocomotion.KEYS) if out.present >> i & 1}


# ---- the graph transformer (include/lmx.h "The graph transformer"; csrc/gfm.hip, csrc/host_gfm.cpp) -----------------------------------
GFM_MAX_NODES = 95


def gfm_check_config(who, input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd):
    """The list of include/lmx.h, refused by the library itself: LmxError names the field."""
    shape = (input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd)
    _model_rows("gfm", who, _model_config(_lib.GfmWeights, who, _ints(_lib.GfmWeights, *shape)))


def gfm_tensor_shapes(input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd):
    """Ordered {tensor name: shape} of one network: the fields of lmx_gfm_weights_t (`layer.{l}.<field>` for the per-layer ones), the
    names of lmx.gfm.pack_tensors."""
    shape = (input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd)
    return _model_shapes("gfm", _lib.GfmWeights, "gfm_tensor_shapes", _ints(_lib.GfmWeights, *shape))


def gfm_weights(input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd, tensors):
    """lmx_gfm_weights_t over the f32 tensors of lmx.gfm.pack_tensors (all on one GPU for gfm_forward, all on the CPU for
    gfm_forward_host).  The struct keeps the tensors alive.  Configurations outside the list of include/lmx.h are refused here with
    the field named, as the library refuses them."""
    shape = (input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd)
    return _model_weights("gfm", _lib.GfmWeights, "gfm_weights", _ints(_lib.GfmWeights, *shape), tensors)


def gfm_graph(embeddings, timestamps, k, max_degree, max_spd):
    """lmx_h_gfm_graph: f32 embeddings [N, E], None or f32 timestamps [N] (numpy) -> dict of numpy arrays: edges int32 [E, 2] (src, dst),
    edge_attr f32 [E, 3], deg_in / deg_out uint8 [N], idx uint8 [N, N], win int32 [N, N] (host arithmetic, no GPU)."""
    import numpy as np

    emb = np.ascontiguousarray(embeddings, np.float32)
    if emb.ndim != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise LmxError(f"gfm_graph: embeddings must be [N, E], got {emb.shape}")
    N, E = emb.shape
    if N > GFM_MAX_NODES:
        raise LmxError(f"gfm_graph: N {N} outside 1 .. {GFM_MAX_NODES}")
    ts = None if timestamps is None else np.ascontiguousarray(timestamps, np.float32)
    if ts is not None and ts.shape != (N,):
        raise LmxError(f"gfm_graph: timestamps {ts.shape} for {N} nodes")
    cap = max(N * min(max(int(k), 0), N - 1) + 2 * (N - 1), 1)
    edges, attr, ne = np.zeros((cap, 2), np.int32), np.zeros((cap, 3), np.float32), np.zeros((1,), np.int32)
    din, dout, idx, win = np.zeros((N,), np.uint8), np.zeros((N,), np.uint8), np.zeros((N, N), np.uint8), np.zeros((N, N), np.int32)
    check(_lib.load().lmx_h_gfm_graph(emb.ctypes.data, ts.ctypes.data if ts is not None else None, N, E, int(k), int(max_degree), int(max_spd),
                                      edges.ctypes.data, attr.ctypes.data, ne.ctypes.data, din.ctypes.data, dout.ctypes.data, idx.ctypes.data,
                                      win.ctypes.data), "lmx_h_gfm_graph")
    n = int(ne[0])
    return {"edges": edges[:n].copy(), "edge_attr": attr[:n].copy(), "deg_in": din, "deg_out": dout, "idx": idx, "win": win}


class _GraphBatch:
    """What GfmBatch and GnnBatch share: n graphs of differing N, nodes and edges concatenated on `device`, the two offset arrays on the
    host, and struct(), which fills _STRUCT's pointers from the attributes named in _FIELDS (None: a null pointer)."""

    def __init__(self, graphs, device):
        import numpy as np

        self.n, self.device = len(graphs), torch.device(device)
        self.sizes = [int(np.asarray(g["x"]).shape[0]) for g in graphs]
        self.n_edges = [len(g["edges"]) for g in graphs]
        self.node_off = np.zeros((self.n + 1,), np.int32)
        self.edge_off = np.zeros((self.n + 1,), np.int32)
        self.node_off[1:] = np.cumsum(self.sizes)
        self.edge_off[1:] = np.cumsum(self.n_edges)
        self.nodes, self.edges = int(self.node_off[-1]), int(self.edge_off[-1])
        F = int(np.asarray(graphs[0]["x"]).shape[1]) if graphs else 1
        self.input_dim = F
        if any(np.asarray(g["x"]).ndim != 2 or np.asarray(g["x"]).shape[1] != F for g in graphs):
            raise LmxError(f"{type(self).__name__}: every x must be [N, input_dim] with one input_dim")
        self.x = self._cat([g["x"] for g in graphs], np.float32, (F,))

    def _cat(self, parts, dtype, tail=()):
        import numpy as np

        parts = [np.ascontiguousarray(p, dtype).reshape((-1,) + tail) for p in parts]
        a = np.concatenate(parts, 0) if parts else np.zeros((0,) + tail, dtype)
        if a.shape[0] == 0:
            a = np.zeros((1,) + tail, dtype)  # a pointer the library may look at, never follow
        return torch.from_numpy(a).to(self.device)

    def _check_entries(self, wants):
        for key, want in wants:
            if max(want, 1) != getattr(self, key).shape[0]:
                raise LmxError(f"{type(self).__name__}: {key} has {getattr(self, key).shape[0]} entries, the graphs call for {want}")

    def struct(self):
        g = self._STRUCT()
        g.n = self.n
        g.node_off_host, g.edge_off_host = self.node_off.ctypes.data, self.edge_off.ctypes.data
        for name in self._FIELDS:
            t = getattr(self, name)
            setattr(g, name, t.data_ptr() if t is not None else None)
        return g


class GfmBatch(_GraphBatch):
    """n graphs of differing N as lmx_gfm_graphs_t wants them: nodes, edges and matrices concatenated on `device`, the two offset arrays
    on the host.  graphs: dicts with x f32 [N, F], timestamps None or f32 [N], and gfm_graph's arrays; targets: None or one node per graph."""
    _STRUCT, _FIELDS = _lib.GfmGraphs, ("x", "timestamps", "has_time", "deg_in", "deg_out", "idx", "win", "edge_attr", "target")

    def __init__(self, graphs, device, targets=None):
        import numpy as np

        super().__init__(graphs, device)
        self.cells = int(sum(s * s for s in self.sizes))
        timed = [g.get("timestamps") is not None for g in graphs]
        self.has_time = torch.from_numpy(np.array(timed + [False], np.uint8)).to(self.device) if any(timed) else None
        self.timestamps = None
        if any(timed):
            ts = [np.ascontiguousarray(g["timestamps"], np.float32) if t else np.zeros((s,), np.float32) for g, t, s in zip(graphs, timed, self.sizes)]
            self.timestamps = torch.from_numpy(np.concatenate(ts)).to(self.device)
        for key, dtype in (("deg_in", np.uint8), ("deg_out", np.uint8), ("idx", np.uint8), ("win", np.int32)):
            setattr(self, key, self._cat([g[key] for g in graphs], dtype))
        self.edge_attr = self._cat([g["edge_attr"] for g in graphs], np.float32, (3,))
        self._check_entries((("deg_in", self.nodes), ("deg_out", self.nodes), ("idx", self.cells), ("win", self.cells)))
        self.target = None
        if targets is not None:
            if len(targets) != self.n:
                raise LmxError(f"GfmBatch: {len(targets)} targets for {self.n} graphs")
            self.target = torch.from_numpy(np.array(list(targets) + [0], np.int32)).to(self.device)


def _graph_front(model, host, w, batch, n_samples):
    """(who, device, S) of a graph model's forward after what both check first: the batch's class, where the batch and the weights
    live, and the feature count."""
    who, cls = f"{model}_forward_host" if host else f"{model}_forward", GfmBatch if model == "gfm" else GnnBatch
    if not isinstance(batch, cls):
        raise LmxError(f"{who}: the graphs come as a {cls.__name__}")
    if host:
        if batch.device.type != "cpu" or w._device.type != "cpu":
            raise LmxError(f"{who} takes CPU tensors and CPU weights")
        dev = torch.device("cpu")
    else:
        dev = _dev(batch.x)
        if w._device != dev:
            raise LmxError(f"{who}: the weights are on {w._device}, the graphs are on {dev}")
    if batch.n and batch.input_dim != w.input_dim:
        raise LmxError(f"{who}: x has {batch.input_dim} features, the network takes {w.input_dim}")
    return who, dev, int(n_samples)


def _graph_run(model, host, who, dev, w, batch, seeds, S, p, outs, ws_bytes):
    """The shared back: one seed per graph, then lmx_h_<model>_forward (host) or lmx_k_<model>_forward with a workspace of
    ws_bytes(lib) bytes on torch's stream; outs: the output tensors (or None) in the order of the C signature."""
    sd = None
    if S:
        if seeds is None:
            raise LmxError(f"{who}: S = {S} needs one seed per graph")
        sd = pack_seeds(seeds)
        if sd.shape != (batch.n,):
            raise LmxError(f"{who}: seeds must be {batch.n} 64-bit values, got {sd.shape}")
    lib, g, name = _lib.load(), batch.struct(), f"lmx_{'h' if host else 'k'}_{model}_forward"
    args = [C.byref(w), C.byref(g), C.c_void_p(sd.ctypes.data if sd is not None else 0), S, float(p)] + [_ptr(t) for t in outs]
    if not host:
        ws = torch.empty((max(int(ws_bytes(lib)), 16) // 16 + 1, 2), dtype=torch.int64, device=dev)
        args += [_ptr(ws), _stream(dev)]
    check(getattr(lib, name)(*args), name)


def _trunk_views(tr, batch, smax, D):
    """graph g's [max(S, 1), N_g, D] of the trunk buffer (None without one)"""
    if tr is None:
        return None
    return [tr[int(batch.node_off[i]) * smax:int(batch.node_off[i + 1]) * smax].reshape(smax, batch.sizes[i], D) for i in range(batch.n)]


def _gfm_forward(host, w, batch, seeds, n_samples, p, node, attn, trunk, vn):
    who, dev, S = _graph_front("gfm", host, w, batch, n_samples)
    for i, s in enumerate(batch.sizes):
        if not 1 <= s <= GFM_MAX_NODES:
            raise LmxError(f"{who}: graph {i} has N = {s} nodes, outside 1 .. {GFM_MAX_NODES}")
    _check_samples(who, S, p)
    if (node or attn) and S:
        raise LmxError(f"{who}: node_pred and attn_to_target are read in eval mode only, S = {S}")
    if attn and batch.target is None:
        raise LmxError(f"{who}: attn_to_target without targets")
    n, nodes, smax, D = batch.n, batch.nodes, max(S, 1), w.d_model

    def buf(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    outs = [buf(n, smax), buf(n, 2), buf(nodes) if node else None, buf(nodes) if attn else None, buf(nodes * smax, D) if trunk else None,
            buf(n, smax, D) if vn else None]
    _graph_run("gfm", host, who, dev, w, batch, seeds, S, p, outs, lambda lib: lib.lmx_gfm_workspace_bytes(n, batch.cells, w.n_heads))
    pred, stats, npred, at, tr, vv = outs
    return pred, stats, npred, at, _trunk_views(tr, batch, smax, D), vv


def gfm_forward(w, batch, seeds, n_samples, p, node=False, attn=False, trunk=False, vn=False):
    """The whole graph transformer for n graphs and S samples in ONE launch behind the bias kernel (lmx_k_gfm_forward, csrc/gfm.hip):
    batch a GfmBatch on the device, seeds: n 64-bit values on the host -> (pred f32 [n, max(S, 1)], stats f32 [n, 2], node_pred f32
    [sum N] or None, attn_to_target f32 [sum N] or None (both S = 0 only), trunk: a list of [max(S, 1), N_g, D] views or None, vn f32
    [n, max(S, 1), D] or None)."""
    return _gfm_forward(False, w, batch, seeds, n_samples, p, node, attn, trunk, vn)


def gfm_forward_host(w, batch, seeds, n_samples, p, node=False, attn=False, trunk=False, vn=False):
    """lmx_h_gfm_forward: the same network in plain C++ on a CPU GfmBatch, with the same keep bits (no GPU)."""
    return _gfm_forward(True, w, batch, seeds, n_samples, p, node, attn, trunk, vn)


# ---- GraphGPS (include/lmx.h "GraphGPS"; csrc/gnn.hip, csrc/host_gnn.cpp) ---------------------------------------------------------------
GNN_MAX_NODES = 95
GNN_MAX_EDGES = 663
GNN_MAX_LAYERS = 4
GNN_LAP_K = 8
GNN_RW_K = 16


def gnn_check_config(who, input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim):
    """The list of include/lmx.h, refused by the library itself: LmxError names the field."""
    shape = (input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim)
    _model_rows("gnn", who, _model_config(_lib.GnnWeights, who, _ints(_lib.GnnWeights, *shape)))


def gnn_tensor_shapes(input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim):
    """Ordered {tensor name: shape} of one network: the fields of lmx_gnn_weights_t (`layer.{l}.<field>` for the per-layer ones; the
    last layer has no edge update), the names of lmx.gnn.pack_tensors."""
    shape = (input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim)
    return _model_shapes("gnn", _lib.GnnWeights, "gnn_tensor_shapes", _ints(_lib.GnnWeights, *shape))


def gnn_weights(input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim, tensors):
    """lmx_gnn_weights_t over the f32 tensors of lmx.gnn.pack_tensors (all on one GPU for gnn_forward, all on the CPU for
    gnn_forward_host).  The struct keeps the tensors alive."""
    shape = (input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim)
    return _model_weights("gnn", _lib.GnnWeights, "gnn_weights", _ints(_lib.GnnWeights, *shape), tensors)


def gnn_graph(embeddings, timestamps, k):
    """lmx_h_gnn_graph: f32 embeddings [N, E], None or f64 timestamps [N] (numpy) -> dict of numpy arrays: edges int32 [E, 2] (src, dst),
    edge_attr f32 [E, 3], csr_ptr int32 [N + 1], csr_edge int32 [E], deg int32 [N], lap f32 [N, 8], rw f32 [N, 16] (host arithmetic)."""
    import numpy as np

    emb = np.ascontiguousarray(embeddings, np.float32)
    if emb.ndim != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise LmxError(f"gnn_graph: embeddings must be [N, E], got {emb.shape}")
    N, E = emb.shape
    if N > GNN_MAX_NODES:
        raise LmxError(f"gnn_graph: N {N} outside 1 .. {GNN_MAX_NODES}")
    ts = None if timestamps is None else np.ascontiguousarray(timestamps, np.float64)
    if ts is not None and ts.shape != (N,):
        raise LmxError(f"gnn_graph: timestamps {ts.shape} for {N} nodes")
    cap = max(N * min(max(int(k), 1), max(N - 1, 1)) + 2 * (N - 1), 1)
    edges, attr, ne = np.zeros((cap, 2), np.int32), np.zeros((cap, 3), np.float32), np.zeros((1,), np.int32)
    ptr, cse, deg = np.zeros((N + 1,), np.int32), np.zeros((cap,), np.int32), np.zeros((N,), np.int32)
    lap, rw = np.zeros((N, GNN_LAP_K), np.float32), np.zeros((N, GNN_RW_K), np.float32)
    check(_lib.load().lmx_h_gnn_graph(emb.ctypes.data, ts.ctypes.data if ts is not None else None, N, E, int(k), edges.ctypes.data, attr.ctypes.data,
                                      ne.ctypes.data, ptr.ctypes.data, cse.ctypes.data, deg.ctypes.data, lap.ctypes.data, rw.ctypes.data),
          "lmx_h_gnn_graph")
    n = int(ne[0])
    return {"edges": edges[:n].copy(), "edge_attr": attr[:n].copy(), "csr_ptr": ptr, "csr_edge": cse[:n].copy(), "deg": deg, "lap": lap, "rw": rw}


def gnn_laplacian(edges, N):
    """lmx_h_gnn_laplacian: the double-precision eigendecomposition behind the Laplacian encoding of an edge list int32 [E, 2] over N
    nodes -> (eigenvalues f64 [N] ascending, eigenvectors f64 [N, N], column c for eigenvalue c)."""
    import numpy as np

    e = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    lam, vec = np.zeros((int(N),), np.float64), np.zeros((int(N), int(N)), np.float64)
    check(_lib.load().lmx_h_gnn_laplacian(e.ctypes.data if len(e) else None, len(e), int(N), lam.ctypes.data, vec.ctypes.data), "lmx_h_gnn_laplacian")
    return lam, vec


class GnnBatch(_GraphBatch):
    """n graphs of differing N as lmx_gnn_graphs_t wants them: nodes and edges concatenated on `device`, the two offset arrays on the
    host.  graphs: dicts with x f32 [N, F] and gnn_graph's arrays."""
    _STRUCT, _FIELDS = _lib.GnnGraphs, ("x", "lap", "rw", "edge_src", "edge_dst", "edge_attr", "csr_ptr", "csr_edge", "deg")

    def __init__(self, graphs, device):
        import numpy as np

        super().__init__(graphs, device)
        self.max_n, self.max_e = max(self.sizes, default=0), max(self.n_edges, default=0)
        self.lap = self._cat([g["lap"] for g in graphs], np.float32, (GNN_LAP_K,))
        self.rw = self._cat([g["rw"] for g in graphs], np.float32, (GNN_RW_K,))
        self.edge_src = self._cat([np.asarray(g["edges"], np.int32).reshape(-1, 2)[:, 0] for g in graphs], np.int32)
        self.edge_dst = self._cat([np.asarray(g["edges"], np.int32).reshape(-1, 2)[:, 1] for g in graphs], np.int32)
        self.edge_attr = self._cat([g["edge_attr"] for g in graphs], np.float32, (3,))
        for key in ("csr_ptr", "csr_edge", "deg"):
            setattr(self, key, self._cat([g[key] for g in graphs], np.int32))
        self._check_entries((("lap", self.nodes), ("rw", self.nodes), ("deg", self.nodes), ("csr_ptr", self.nodes + self.n),
                             ("csr_edge", self.edges), ("edge_attr", self.edges)))


def _gnn_forward(host, w, batch, seeds, n_samples, p, trunk):
    who, dev, S = _graph_front("gnn", host, w, batch, n_samples)
    _check_samples(who, S, p)
    for i, (s, e) in enumerate(zip(batch.sizes, batch.n_edges)):
        if not 1 <= s <= GNN_MAX_NODES:
            raise LmxError(f"{who}: graph {i} has N = {s} nodes, outside 1 .. {GNN_MAX_NODES}")
        if e > GNN_MAX_EDGES:
            raise LmxError(f"{who}: graph {i} has E = {e} edges, more than {GNN_MAX_EDGES}")
        if S and s < 2:
            raise LmxError(f"{who}: graph {i} has N = 1 node: BatchNorm has no batch statistics with S = {S}")
    n, nodes, smax, D = batch.n, batch.nodes, max(S, 1), w.d_model

    def buf(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    outs = ([buf(nodes, S), buf(nodes, 2), None, None, None] if S else [None, None, buf(n), buf(nodes), buf(nodes)]) + \
        [buf(nodes * smax, D) if trunk else None]
    _graph_run("gnn", host, who, dev, w, batch, seeds, S, p, outs,
               lambda lib: lib.lmx_gnn_workspace_bytes(n, S, batch.max_n, batch.max_e, w.d_model, w.n_layers))
    return (*outs[:5], _trunk_views(outs[5], batch, smax, D))


def gnn_forward(w, batch, seeds, n_samples, p, trunk=False):
    """The live network of GraphGPS for n graphs and S samples in ONE launch (lmx_k_gnn_forward, csrc/gnn.hip): batch a GnnBatch on the
    device, seeds: n 64-bit values on the host -> (node_mc f32 [sum N, S], stats f32 [sum N, 2] = mean and unbiased std (both None when
    S = 0), graph_pred f32 [n], node_pred f32 [sum N], attn_weights f32 [sum N] (all three None when S > 0), trunk: a list of
    [max(S, 1), N_g, D] views or None)."""
    return _gnn_forward(False, w, batch, seeds, n_samples, p, trunk)


def gnn_forward_host(w, batch, seeds, n_samples, p, trunk=False):
    """lmx_h_gnn_forward: the same network in plain C++ on a CPU GnnBatch, with the same keep bits (no GPU)."""
    return _gnn_forward(True, w, batch, seeds, n_samples, p, trunk)


def pack_records(rec, n_rows=None, row_maps=(), field_map=None, n_valid=None, out=None):
    """dict of per-frame tensors [n_k, ...] on one device -> (uint8 [n_rows, stride], layout): lmx.dist.pack_records' bytes from ONE
    launch that stores every byte of the matrix once (csrc/records.hip); `out` (uint8 [n_rows, stride], contiguous) needs no clearing.
    Without maps every field has the same n rows, record row r is row r of each field and n_rows - n padding rows follow.
    row_maps: int32 [n_valid] device tensors, entry r = the source row of record row r or -1 (zeros); field_map: {name: index into
    row_maps} for the fields that follow one (the others keep the identity and give zeros past their last row); n_valid: rows whose
    `valid` word is 1 (default: the fields' row count without maps, n_rows with them); the rows behind them are padding, all zeros."""
    from . import dist

    names = sorted(rec)
    dev = _dev(*[rec[k] for k in names], *row_maps)
    field_map = dict(field_map or {})
    rows = {k: int(rec[k].shape[0]) for k in names}
    n = max(rows.values()) if not row_maps else None
    if n_rows is None:
        if n is None:
            raise LmxError("pack_records: n_rows is needed with row maps")
        n_rows = n
    n_rows = int(n_rows)
    if n_valid is None:
        n_valid = n if n is not None else n_rows
    layout, stride = dist.record_layout(rec)
    if len(layout) > _lib.RecordLayout.MAX_FIELDS or len(row_maps) > _lib.RecordLayout.MAX_MAPS:
        raise LmxError(f"pack_records: {len(layout)} fields and {len(row_maps)} maps; at most {_lib.RecordLayout.MAX_FIELDS} and {_lib.RecordLayout.MAX_MAPS}")
    if not row_maps:
        for k in names:
            if rows[k] != n:
                raise LmxError(f"pack_records: field {k} has {rows[k]} rows, expected {n}")
        if n_rows < n:
            raise LmxError(f"pack_records: {n} records do not fit {n_rows} rows")
    for m in row_maps:
        if m.dtype != torch.int32 or m.dim() != 1 or int(m.shape[0]) != n_valid or not m.is_contiguous():
            raise LmxError(f"pack_records: a row map is a contiguous int32 [{n_valid}] tensor (one entry per valid row)")
    keep = []  # the dense views the launch reads
    fields = (_lib.RecordField * max(1, len(layout)))()
    for f, (name, dtype, tail, off, nb) in zip(fields, layout):
        src = rec[name].contiguous()
        keep.append(src)
        which = field_map.pop(name, -1)
        if not -1 <= which < len(row_maps):
            raise LmxError(f"pack_records: field {name} follows map {which} of {len(row_maps)}")
        if nb == 0:
            raise LmxError(f"pack_records: field {name} has empty rows")
        f.src, f.row_bytes, f.offset, f.map, f.n_src = src.data_ptr() if rows[name] else None, nb, off, which, rows[name]
    if field_map:
        raise LmxError(f"pack_records: field_map names {sorted(field_map)}, which the record does not hold")
    if out is None:
        out = torch.empty((n_rows, stride), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n_rows, stride) or not out.is_contiguous() or out.device != dev:
        raise LmxError(f"pack_records: out must be a contiguous uint8 [{n_rows}, {stride}] tensor on {dev}")
    maps = (C.c_void_p * max(1, len(row_maps)))(*[m.data_ptr() for m in row_maps])
    check(_lib.load().lmx_k_pack_records(fields, len(layout), maps, len(row_maps), n_valid, n_rows, stride, _ptr(out), _stream(dev)),
          "lmx_k_pack_records")
    return out, layout


_REC_DTYPES = (torch.uint8, torch.int32, torch.int64, torch.float32)  # LMX_REC_*


def layout_of(lay):
    """a lmx_record_layout_t as lmx.dist.record_layout gives it: ([(name, dtype, tail shape, byte offset, bytes)], stride)"""
    fields = [lay.fields[i] for i in range(lay.n_fields)]
    return [(f.name.decode(), _REC_DTYPES[f.dtype], tuple(int(f.shape[d]) for d in range(f.ndim)), int(f.offset), int(f.nbytes)) for f in fields], int(lay.stride)


def record_layout(h, w, hidden, max_det=300, scheduled=False):
    """lmx_h_record_layout: (layout, stride) of the fused step's record in lmx.dist.record_layout's form, computed by the library."""
    lay = _lib.RecordLayout()
    check(_lib.load().lmx_h_record_layout(int(h), int(w), int(hidden), int(max_det), int(bool(scheduled)), C.byref(lay)), "lmx_h_record_layout")
    return layout_of(lay)


def stream_plan(n_chunks, max_streams=4, layout="lanes"):
    """lmx_h_stream_plan: lmx.pipeline.stream_plan computed by the library."""
    if layout not in ("lanes", "rr"):
        raise ValueError(f"stream layout {layout!r}: expected 'lanes' or 'rr'")
    pool, det, emb = C.c_int(0), C.c_int(0), C.c_int(0)
    sam = (C.c_int32 * max(1, n_chunks))()
    check(_lib.load().lmx_h_stream_plan(int(n_chunks), int(max_streams), ("lanes", "rr").index(layout), C.byref(pool), C.byref(det), C.byref(emb), sam),
          "lmx_h_stream_plan")
    return pool.value, det.value, emb.value, list(sam)[:n_chunks]


def row_map(n, idx, what="idx"):
    """lmx_h_row_map: (map, ran) int32 lists of n entries for the ascending frame indices `idx` (LmxError names a bad index)."""
    idx = [int(i) for i in idx]
    arr = (C.c_int32 * max(1, len(idx)))(*idx)
    m, ran = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
    check(_lib.load().lmx_h_row_map(int(n), arr, len(idx), what.encode(), m, ran), "lmx_h_row_map")
    return list(m)[:n], list(ran)[:n]


FUSED_MLP_WIDTHS = (112, 224)  # (448 exists as a development configuration: no faster than the unfused launches, csrc/mlp.hip)
if os.environ.get("LMX_MLP448"):  # development A/B only
    FUSED_MLP_WIDTHS = (112, 224, 448)


def ln_mlp(x, gamma, beta, w1, b1, w2, b2, eps, x16=None, next_ln=None):
    """x (f32 [rows, D], updated in place) += fc2(gelu(fc1(LayerNorm(x)))) for D in FUSED_MLP_WIDTHS (csrc/mlp.hip).
    x16: optional f16 [rows, D] that also receives the updated x (saves a cast pass where an f16 copy is needed next).
    next_ln=(gamma, beta, h): h (f16 [rows, D]) receives LayerNorm(updated x; gamma, beta, eps) — the next block's first
    LayerNorm, without its launch."""
    dev = _dev(x, gamma, beta, w1, b1, w2, b2, x16, *(next_ln or ()))
    rows, D, ldx = _rows(x, "ln_mlp x")
    if x.dtype != torch.float32 or w1.dtype != torch.float16 or w2.dtype != torch.float16:
        raise LmxError("ln_mlp: x must be f32 and the weights f16")
    if tuple(w1.shape) != (4 * D, D) or tuple(w2.shape) != (D, 4 * D) or not (w1.is_contiguous() and w2.is_contiguous()):
        raise LmxError("ln_mlp: weight shapes must be [4D, D] and [D, 4D], contiguous")
    if x16 is not None and (x16.dtype != torch.float16 or tuple(x16.shape) != (rows, D) or not x16.is_contiguous()):
        raise LmxError("ln_mlp: x16 must be contiguous float16 [rows, D]")
    gn, bn, hn = next_ln if next_ln else (None, None, None)
    if hn is not None and (hn.dtype != torch.float16 or tuple(hn.shape) != (rows, D) or not hn.is_contiguous() or gn.numel() != D or bn.numel() != D):
        raise LmxError("ln_mlp: next_ln = (gamma [D], beta [D], contiguous float16 [rows, D])")
    ws = torch.empty((rows, D), dtype=torch.float16, device=x.device)  # LayerNorm output (the library's workspace)
    check(_lib.load().lmx_k_ln_mlp(_ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), rows, D,
                                   float(eps), _ptr(ws), _ptr(x16), _ptr(gn), _ptr(bn), _ptr(hn), _stream(dev)), "lmx_k_ln_mlp")
    return x


def hiera_attn8_ok(D, heads, win, Gh, Gw, q_stride):
    """Shapes lmx_k_hiera_attn8 is built for: Hiera-B+ stage 1 (D 112, 2 heads of 56), whole 8 x 8 windows, no query pooling."""
    return D == 112 and heads == 2 and win == 8 and not q_stride and Gh % 8 == 0 and Gw % 8 == 0 and os.environ.get("LMX_HIERA_ATTN8", "1") != "0"


def hiera_attn8(x, packed, n_img, Gh, Gw, heads, h=None, ln=None):
    """x (f32 [rows, D], in place) += proj(window attention(qkv(layer_norm1(x)))) for 8 x 8-token windows (csrc/hiera.hip).
    Either h = layer_norm1(x) as f16 [rows, D] (packed from pack_hiera_attn(..., ln_inside=False)) or ln = (gamma, beta, eps): the
    kernel normalises x itself (packed with ln_inside=True).  packed = (wqkv_p, bqkv_p, wo_p, bo)."""
    wq, bq, wo, bo = packed
    if (h is None) == (ln is None):
        raise LmxError("hiera_attn8: give either h or ln=(gamma, beta, eps)")
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    dev = _dev(x, h, gamma, beta, wq, bq, wo, bo)
    rows, D, ldx = _rows(x, "hiera_attn8 x")
    if x.dtype != torch.float32 or rows != n_img * Gh * Gw:
        raise LmxError("hiera_attn8: x must be float32 [n*Gh*Gw, D]")
    if h is not None and (h.dtype != torch.float16 or tuple(h.shape) != (rows, D) or not h.is_contiguous()):
        raise LmxError("hiera_attn8: h must be contiguous float16 [rows, D]")
    if ln is not None and (gamma.numel() != D or beta.numel() != D or gamma.dtype != torch.float32 or beta.dtype != torch.float32):
        raise LmxError("hiera_attn8: gamma / beta must be float32 [D]")
    if tuple(wq.shape) != (3 * heads * 64, 128) or tuple(wo.shape) != (D, heads * 64) or wq.dtype != torch.float16 or wo.dtype != torch.float16 \
            or not (wq.is_contiguous() and wo.is_contiguous()) or bq.numel() != 3 * heads * 64 or bo.numel() != D:
        raise LmxError("hiera_attn8: packed operands have the wrong shapes (lmx.sam.pack_hiera_attn)")
    check(_lib.load().lmx_k_hiera_attn8(_ptr(h), _ptr(x), ldx, _ptr(gamma), _ptr(beta), float(eps), _ptr(wq), _ptr(bq), _ptr(wo), _ptr(bo),
                                        n_img, Gh, Gw, D, heads, float((D // heads) ** -0.5), _stream(dev)), "lmx_k_hiera_attn8")
    return x


def hiera_attn4_ok(D, heads, win, Gh, Gw, q_stride):
    """Shapes lmx_k_hiera_attn4 is built for: Hiera-B+ stage 2 (D 224, 4 heads of 56), whole 4 x 4 windows, no query pooling."""
    return D == 224 and heads == 4 and win == 4 and not q_stride and Gh % 4 == 0 and Gw % 4 == 0 and os.environ.get("LMX_HIERA_ATTN4", "1") != "0"


def hiera_attn4(h, x, packed, n_img, Gh, Gw, heads):
    """x (f32 [rows, D], in place) += proj(window attention(qkv(h))) for 4 x 4-token windows, weights streamed (csrc/hiera.hip).
    h f16 [rows, D] contiguous = layer_norm1(x); packed = (w_img, bias) from lmx.sam.pack_hiera_attn4."""
    img, bias = packed
    dev = _dev(h, x, img, bias)
    rows, D, ldx = _rows(x, "hiera_attn4 x")
    if x.dtype != torch.float32 or h.dtype != torch.float16 or tuple(h.shape) != (rows, D) or not h.is_contiguous() or rows != n_img * Gh * Gw:
        raise LmxError("hiera_attn4: h must be contiguous float16 [n*Gh*Gw, D] and x float32 rows of the same count")
    if tuple(img.shape) != (4 * heads, 16384) or img.dtype != torch.float16 or not img.is_contiguous() or bias.numel() != heads * 192 + D \
            or bias.dtype != torch.float32:
        raise LmxError("hiera_attn4: packed operands have the wrong shapes (lmx.sam.pack_hiera_attn4)")
    check(_lib.load().lmx_k_hiera_attn4(_ptr(h), _ptr(x), ldx, _ptr(img), _ptr(bias), n_img, Gh, Gw, D, heads, float((D // heads) ** -0.5),
                                        _stream(dev)), "lmx_k_hiera_attn4")
    return x


def hiera_attn_pool_ok(Din, Dout, heads, win, Gh, Gw, q_stride):
    """Shapes lmx_k_hiera_attn_pool is built for: the blocks that open Hiera-B+ stage 2 (112 -> 224, 4 heads, 8 x 8 windows) and
    stage 3 (224 -> 448, 8 heads, 4 x 4 windows), pooled queries and shortcut."""
    if not q_stride or os.environ.get("LMX_HIERA_ATTN_POOL", "1") == "0":
        return False
    if (Din, Dout, heads, win) == (112, 224, 4, 8):
        return Gh % 8 == 0 and Gw % 8 == 0
    if (Din, Dout, heads, win) == (224, 448, 8, 4):  # the block that opens stage 3 (LMX_HIERA_ATTN_POOL3=0: its separate launches)
        return Gh % 4 == 0 and Gw % 4 == 0 and os.environ.get("LMX_HIERA_ATTN_POOL3", "1") != "0"
    return False


def hiera_attn_pool(h, packed, n_img, Gh, Gw, heads, Dout):
    """The attention half of Hiera's stage-opening block as one launch (csrc/hiera.hip): returns f32 [n*(Gh/2)*(Gw/2), Dout] =
    pool(proj(h)) + attn_proj(window attention(pool(q(h)), k(h), v(h))).  h f16 [n*Gh*Gw, Din] contiguous = layer_norm1(x);
    packed = (w_img, bias) from lmx.sam.pack_hiera_attn_pool."""
    img, bias = packed
    dev = _dev(h, img, bias)
    if h.dtype != torch.float16 or h.dim() != 2 or not h.is_contiguous() or h.shape[0] != n_img * Gh * Gw:
        raise LmxError("hiera_attn_pool: h must be contiguous float16 [n*Gh*Gw, Din]")
    Din = h.shape[1]
    nimg, nb = (47, Dout + heads * 192) if Din > 128 else (14, 2 * Dout + heads * 192)
    if tuple(img.shape) != (nimg, 16384) or img.dtype != torch.float16 or not img.is_contiguous() or bias.numel() != nb or bias.dtype != torch.float32:
        raise LmxError("hiera_attn_pool: packed operands have the wrong shapes (lmx.sam.pack_hiera_attn_pool)")
    out = torch.empty((n_img * (Gh // 2) * (Gw // 2), Dout), dtype=torch.float32, device=h.device)
    check(_lib.load().lmx_k_hiera_attn_pool(_ptr(h), _ptr(out), _ptr(img), _ptr(bias), n_img, Gh, Gw, Din, Dout, heads,
                                            float((Dout // heads) ** -0.5), _stream(dev)), "lmx_k_hiera_attn_pool")
    return out


def ln_mlp_img_ok(D, rows):
    """Where lmx_k_ln_mlp_img (the streamed-image form of the fused LN + MLP, csrc/hiera.hip) replaces csrc/mlp.hip's kernel: D = 112 /
    224 at EVERY row count.  It is faster only from ~1.3 M / 0.33 M rows (tools/mlp_probe.py) and 10 - 30 % slower below a third of
    that, but the two kernels sum in different orders, and a frame's result must not depend on the batch it rides in (DESIGN.md section
    3, Reproducibility: the multi-GPU JSON equals the single-GPU one whatever the sharding) — so one kernel serves all batch sizes.
    LMX_MLP_IMG=0: csrc/mlp.hip's kernel everywhere."""
    return D in (112, 224) and os.environ.get("LMX_MLP_IMG", "1") != "0"


def ln_mlp_img(x, packed, eps, x16=None, h_next=None):
    """x (f32 [rows, D], in place) += fc2(gelu(fc1(LayerNorm(x)))) with the weights as LDS images (lmx.sam.pack_ln_mlp: (w_img, bias);
    bias carries layer_norm2's and — when h_next is given — the next block's layer_norm1's vectors).  x16 / h_next: as ln_mlp."""
    img, bias = packed
    dev = _dev(x, img, bias, x16, h_next)
    rows, D, ldx = _rows(x, "ln_mlp_img x")
    nimg = 7 if D == 112 else 28
    if x.dtype != torch.float32 or tuple(img.shape) != (nimg, 16384) or img.dtype != torch.float16 or not img.is_contiguous() \
            or bias.numel() != 9 * D or bias.dtype != torch.float32:
        raise LmxError("ln_mlp_img: x must be f32 [rows, D] and the packed operands those of lmx.sam.pack_ln_mlp")
    for t, name in ((x16, "x16"), (h_next, "h_next")):
        if t is not None and (t.dtype != torch.float16 or tuple(t.shape) != (rows, D) or not t.is_contiguous()):
            raise LmxError(f"ln_mlp_img: {name} must be contiguous float16 [rows, D]")
    check(_lib.load().lmx_k_ln_mlp_img(_ptr(x), ldx, _ptr(img), _ptr(bias), rows, D, float(eps), _ptr(x16), _ptr(h_next), _stream(dev)),
          "lmx_k_ln_mlp_img")
    return x


def _attn_desc(q, k, v, out, B, H, Tq, Tk, hd, scale, window, pad_k, pad_v):
    d = AttnDesc()
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    for t in (q, k, v, out):
        if t.dtype != torch.float16 or t.stride(-1) != 1:
            raise LmxError("attention: q/k/v/out must be float16 with contiguous last dim")
    d.B, d.H, d.Tq, d.Tk, d.hd = B, H, Tq, Tk, hd
    d.scale = float(scale)
    if window is None:
        d.mode = 0
    else:
        d.mode = 1
        d.Gh, d.Gw, d.ws, d.q_stride = window["Gh"], window["Gw"], window["ws"], window.get("q_stride", 1)
        d.pad_k = pad_k.data_ptr() if pad_k is not None else None
        d.pad_v = pad_v.data_ptr() if pad_v is not None else None
    return d


def attention(q, k, v, out, B, H, Tq, Tk, hd, scale, window=None, pad_k=None, pad_v=None, rel_pos=None):
    """q/k/v/out: 2-D token-row views [rows, >=H*hd] (row stride = ld).  window = None (flat: row = b*T + t) or
    dict(Gh, Gw, ws, q_stride) for in-place window addressing on the token grid.
    rel_pos = (rel_pos_h, rel_pos_w) f32 [2S-1, hd] adds SAM v1's decomposed relative-position bias (S*S == Tk)."""
    dev = _dev(q, k, v, out, pad_k, pad_v)
    d = _attn_desc(q, k, v, out, B, H, Tq, Tk, hd, scale, window, pad_k, pad_v)
    keep = None
    if rel_pos is not None:
        rh, rw = rel_pos
        _dev(rh, rw, q)
        S = (rh.shape[0] + 1) // 2
        if S * S != Tk or Tq != Tk or rh.dtype != torch.float32 or tuple(rh.shape) != (2 * S - 1, hd) or rh.shape != rw.shape:
            raise LmxError("attention: rel_pos tables must be float32 [2S-1, hd] with S*S == Tq == Tk")
        keep = torch.empty((B * H * Tq, 2 * S), dtype=torch.float16, device=q.device)
        check(_lib.load().lmx_k_relpos_tables(C.byref(d), _ptr(rh), _ptr(rw), S, _ptr(keep), _stream(dev)), "lmx_k_relpos_tables")
        d.rel, d.rel_S = keep.data_ptr(), S
    check(_lib.load().lmx_k_attention(C.byref(d), _stream(dev)), "lmx_k_attention")
    return out


def rope(x, B, T, H, hd, n_prefix, cos_t, sin_t):
    dev = _dev(x, cos_t, sin_t)
    check(_lib.load().lmx_k_rope(_ptr(x), x.stride(0), B, T, H, hd, n_prefix, _ptr(cos_t), _ptr(sin_t), _stream(dev)),
          "lmx_k_rope")
    return x


def pil_resize(src, dw, dh, tab_h, tab_v, swap_rb=False):
    """Pillow-exact two-pass resize of u8 [n,sh,sw,3] -> [n,dh,dw,3].  tab_* = (bounds i32 [2*out], kk i32
    [out*ksize], ksize) device tensors from lmx.resample.coeff_tables; None skips that pass (size unchanged)."""
    dev = _dev(src)
    n, sh, sw, c = src.shape
    if c != 3 or src.dtype != torch.uint8 or not src.is_contiguous():
        raise LmxError("pil_resize: src must be contiguous uint8 [n,h,w,3]")
    lib = _lib.load()
    cur = src
    if tab_h is not None:
        bounds, kk, ksize = tab_h
        tmp = torch.empty((n, sh, dw, 3), dtype=torch.uint8, device=src.device)
        check(lib.lmx_k_pil_resize_h(_ptr(cur), _ptr(tmp), n, sh, sw, dw, _ptr(bounds), _ptr(kk), ksize,
                                     1 if swap_rb else 0, _stream(dev)), "lmx_k_pil_resize_h")
        cur = tmp
    elif swap_rb:
        raise LmxError("pil_resize: swap_rb needs the horizontal pass")
    if tab_v is not None:
        bounds, kk, ksize = tab_v
        w = cur.shape[2]
        dst = torch.empty((n, dh, w, 3), dtype=torch.uint8, device=src.device)
        check(lib.lmx_k_pil_resize_v(_ptr(cur), _ptr(dst), n, cur.shape[1], dh, w, _ptr(bounds), _ptr(kk), ksize,
                                     _stream(dev)), "lmx_k_pil_resize_v")
        cur = dst
    return cur


def patchify_norm(img, top, left, gh, gw, P, lut, k_pad=None):
    """-> f16 [n*gh*gw, k_pad or P*P*3] patch matrix (columns beyond P*P*3 zero)."""
    dev = _dev(img, lut)
    n, ih, iw, c = img.shape
    if c != 3 or img.dtype != torch.uint8 or not img.is_contiguous():
        raise LmxError("patchify_norm: img must be contiguous uint8 [n,h,w,3]")
    K = P * P * 3
    ldo = k_pad or K
    alloc = torch.zeros if ldo != K else torch.empty
    out = alloc((n * gh * gw, ldo), dtype=torch.float16, device=img.device)
    check(_lib.load().lmx_k_patchify_norm(_ptr(img), _ptr(out), n, ih, iw, top, left, gh, gw, P, ldo, _ptr(lut),
                                          _stream(dev)), "lmx_k_patchify_norm")
    return out


def float_resize_patchify(src, gh, gw, P, tab_h, tab_v, seg_cols, rescale, mean, std, swap_rb=False, k_pad=None):
    """u8 [n,sh,sw,3] -> f16 [n*gh*gw, k_pad or P*P*3] patch matrix (columns beyond P*P*3 zero) of the float antialiased
    resize to gh*P x gw*P: DINOv3ViTImageProcessor's rescale -> resize -> normalize in one kernel.  tab_* = (bounds i32
    [2*out], kk f32 [out*ksize], ksize) device tensors from lmx.resample.aa_tables, seg_cols from lmx.resample.segment_cols."""
    bh, kh, ksh = tab_h
    bv, kv, ksv = tab_v
    dev = _dev(src, bh, kh, bv, kv)
    n, sh, sw, c = src.shape
    if c != 3 or src.dtype != torch.uint8 or not src.is_contiguous():
        raise LmxError("float_resize_patchify: src must be contiguous uint8 [n,h,w,3]")
    if (bh.dtype, bv.dtype, kh.dtype, kv.dtype) != (torch.int32, torch.int32, torch.float32, torch.float32):
        raise LmxError("float_resize_patchify: bounds must be int32 and weights float32")
    if (bh.numel(), kh.numel(), bv.numel(), kv.numel()) != (2 * gw * P, gw * P * ksh, 2 * gh * P, gh * P * ksv):
        raise LmxError(f"float_resize_patchify: tables do not describe a {gh * P} x {gw * P} output")
    if len(mean) != 3 or len(std) != 3:
        raise LmxError("float_resize_patchify: mean and std must have 3 entries")
    K = P * P * 3
    ldo = k_pad or K
    alloc = torch.zeros if ldo != K else torch.empty
    out = alloc((n * gh * gw, ldo), dtype=torch.float16, device=src.device)
    ms = (C.c_float * 6)(*mean, *std)
    check(_lib.load().lmx_k_float_resize_patchify(_ptr(src), _ptr(out), n, sh, sw, gh, gw, P, ldo, _ptr(bh), _ptr(kh), ksh,
                                                  _ptr(bv), _ptr(kv), ksv, seg_cols, rescale, ms, 1 if swap_rb else 0,
                                                  _stream(dev)), "lmx_k_float_resize_patchify")
    return out


def assemble_tokens(patch, prefix, pos, B, np_, n_prefix, D):
    dev = _dev(patch, prefix, pos)
    out = torch.empty((B * (np_ + n_prefix), D), dtype=torch.float32, device=patch.device)
    check(_lib.load().lmx_k_assemble_tokens(_ptr(patch), _ptr(prefix), _ptr(pos), _ptr(out), B, np_, n_prefix, D,
                                            _stream(dev)), "lmx_k_assemble_tokens")
    return out


def swiglu(gu, out=None):
    """f16 [rows, 2I] (gate columns first) -> f16 [rows, I] = silu(gate) * up (lmx_k_swiglu): the unfused form of ACT_SWIGLU,
    kept as its timing reference."""
    dev = _dev(gu, out)
    rows, N, ldg = _rows(gu, "swiglu in")
    if gu.dtype != torch.float16 or N % 2:
        raise LmxError("swiglu: input must be float16 [rows, 2I]")
    if out is None:
        out = torch.empty((rows, N // 2), dtype=torch.float16, device=gu.device)
    ro, Io, ldo = _rows(out, "swiglu out")
    if (ro, Io) != (rows, N // 2) or out.dtype != torch.float16:
        raise LmxError(f"swiglu: out must be float16 ({rows},{N // 2})")
    check(_lib.load().lmx_k_swiglu(_ptr(gu), ldg, _ptr(out), ldo, rows, N // 2, _stream(dev)), "lmx_k_swiglu")
    return out


def token_mean(x, B, T, D):
    dev = _dev(x)
    out = torch.empty((B, D), dtype=torch.float32, device=x.device)
    check(_lib.load().lmx_k_token_mean(_ptr(x), _DT[x.dtype], _ptr(out), B, T, D, _stream(dev)), "lmx_k_token_mean")
    return out


def nms(pred, conf, iou=0.7, max_det=300, max_wh=7680.0):
    """pred f32 [n,A,4+nc] -> (boxes [n,max_det,4], scores, cls, src, counts) on device (lmx_k_nms)."""
    dev = _dev(pred)
    if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_contiguous():
        raise LmxError("nms: pred must be contiguous float32 [n,A,4+nc]")
    n, A, row = pred.shape
    lib = _lib.load()
    ws = torch.empty((int(lib.lmx_nms_workspace_bytes(n, A)),), dtype=torch.uint8, device=pred.device)
    boxes = torch.zeros((n, max_det, 4), dtype=torch.float32, device=pred.device)
    scores = torch.zeros((n, max_det), dtype=torch.float32, device=pred.device)
    cls = torch.zeros((n, max_det), dtype=torch.int32, device=pred.device)
    src = torch.full((n, max_det), -1, dtype=torch.int32, device=pred.device)
    counts = torch.zeros((n,), dtype=torch.int32, device=pred.device)
    check(lib.lmx_k_nms(_ptr(pred), n, A, row - 4, float(conf), float(iou), max_det, float(max_wh), _ptr(boxes),
                        _ptr(scores), _ptr(cls), _ptr(src), _ptr(counts), _ptr(ws), _stream(dev)), "lmx_k_nms")
    return boxes, scores, cls, src, counts


# ---- YOLO pieces ------------------------------------------------------------------------------------------
def letterbox(frames, geo, tables, swap_rb=True):
    """u8 [n,sh,sw,3] -> u8 [n,oh,ow,3]; geo from lmx.letterbox.geometry, tables = device (xofs, ialpha, yofs, ibeta)."""
    dev = _dev(frames)
    n, sh, sw, c = frames.shape
    if c != 3 or frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise LmxError("letterbox: frames must be contiguous uint8 [n,h,w,3]")
    out = torch.empty((n, geo.oh, geo.ow, 3), dtype=torch.uint8, device=frames.device)
    xo, ia, yo, ib = tables if tables is not None else (None, None, None, None)
    check(_lib.load().lmx_k_letterbox(_ptr(frames), _ptr(out), n, sh, sw, geo.rh, geo.rw, geo.top, geo.left, geo.oh, geo.ow,
                                      _ptr(xo), _ptr(ia), _ptr(yo), _ptr(ib), 1 if swap_rb else 0, _stream(dev)),
          "lmx_k_letterbox")
    return out


def stem_conv(img_u8, w, bias, out=None):
    dev = _dev(img_u8, w, bias, out)
    n, H, W, _ = img_u8.shape
    Cout = bias.numel()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((n, Ho, Wo, Cout), dtype=torch.float16, device=img_u8.device)
    if not out.is_contiguous() or tuple(out.shape) != (n, Ho, Wo, Cout):
        raise LmxError("stem_conv: out must be a dense NHWC tensor")
    check(_lib.load().lmx_k_stem_conv(_ptr(img_u8), _ptr(w), _ptr(bias), _ptr(out), n, H, W, Cout, _stream(dev)),
          "lmx_k_stem_conv")
    return out


def maxpool5(x, out):
    dev = _dev(x, out)
    n, H, W, Cc, ps = _nhwc(x, "maxpool5 x")
    no, Ho, Wo, Co, pso = _nhwc(out, "maxpool5 out")
    if (no, Ho, Wo, Co) != (n, H, W, Cc):
        raise LmxError("maxpool5: shape mismatch")
    check(_lib.load().lmx_k_maxpool5(_ptr(x), ps, _ptr(out), pso, n, H, W, Cc, _stream(dev)), "lmx_k_maxpool5")
    return out


def upsample2(x, out):
    dev = _dev(x, out)
    n, H, W, Cc, ps = _nhwc(x, "upsample2 x")
    no, Ho, Wo, Co, pso = _nhwc(out, "upsample2 out")
    if (no, Ho, Wo, Co) != (n, 2 * H, 2 * W, Cc):
        raise LmxError("upsample2: shape mismatch")
    check(_lib.load().lmx_k_upsample2(_ptr(x), ps, _ptr(out), pso, n, H, W, Cc, _stream(dev)), "lmx_k_upsample2")
    return out


# ---- the exact plan's x3 format (csrc/exact.hip): a value travels as the f16 channel triple [hi | lo | hi] per group ----------
def split3(x, act, out3, g=None, res3=None):
    """f32 NHWC x [n,H,W,N] (channel slices allowed) -> x3 groups of width g written into out3 [n,H,W,3N] (a channel slice of
    an x3 buffer); y = act(x) + value(res3) (lmx_k_split3).  x may be the [S, n,H,W,N] partial outputs of a split-K launch:
    they are added up in index order first."""
    dev = _dev(x, out3, res3)
    nsum, sstride = 1, 0
    if x.dim() == 5:
        nsum, sstride = x.shape[0], x.stride(0)
        x = x[0]
    n, H, W, N, ps = _nhwc(x, "split3 x")
    no, Ho, Wo, C3, pso = _nhwc(out3, "split3 out")
    g = g or N
    if x.dtype != torch.float32 or out3.dtype != torch.float16 or (no, Ho, Wo, C3) != (n, H, W, 3 * N):
        raise LmxError(f"split3: x f32 {tuple(x.shape)} -> out3 f16 {tuple(out3.shape)} (3x the channels) expected")
    ldr = 0
    if res3 is not None:
        nr, Hr, Wr, Cr, ldr = _nhwc(res3, "split3 res")
        if (nr, Hr, Wr, Cr) != (n, H, W, 3 * N) or res3.dtype != torch.float16:
            raise LmxError("split3: residual must be an x3 tensor of the output's shape")
    check(_lib.load().lmx_k_split3(_ptr(x), ps, act, _ptr(res3), ldr, _ptr(out3), pso, n * H * W, N, g, nsum, sstride, _stream(dev)),
          "lmx_k_split3")
    return out3


def maxpool5_x3(x3, out3):
    dev = _dev(x3, out3)
    n, H, W, C3, ps = _nhwc(x3, "maxpool5_x3 x")
    no, Ho, Wo, Co, pso = _nhwc(out3, "maxpool5_x3 out")
    if (no, Ho, Wo, Co) != (n, H, W, C3) or C3 % 3:
        raise LmxError("maxpool5_x3: shape mismatch")
    check(_lib.load().lmx_k_maxpool5_x3(_ptr(x3), ps, _ptr(out3), pso, n, H, W, C3 // 3, _stream(dev)), "lmx_k_maxpool5_x3")
    return out3


def stem_conv_x3(img_u8, w, bias):
    dev = _dev(img_u8, w, bias)
    n, H, W, _ = img_u8.shape
    Cout = bias.numel()
    out = torch.empty((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 3 * Cout), dtype=torch.float16, device=img_u8.device)
    check(_lib.load().lmx_k_stem_conv_x3(_ptr(img_u8), _ptr(w), _ptr(bias), _ptr(out), n, H, W, Cout, _stream(dev)),
          "lmx_k_stem_conv_x3")
    return out


def detect_decode(head, pred, nc, stride, a_off):
    """head f32 [n,H,W,ldh] dense, pred f32 [n,A,4+nc] dense."""
    dev = _dev(head, pred)
    n, H, W, ldh = head.shape
    A = pred.shape[1]
    if not head.is_contiguous() or not pred.is_contiguous() or pred.shape[2] != 4 + nc:
        raise LmxError("detect_decode: head/pred must be dense")
    check(_lib.load().lmx_k_detect_decode(_ptr(head), ldh, _ptr(pred), n, H, W, nc, float(stride), a_off, A, _stream(dev)),
          "lmx_k_detect_decode")
    return pred


def scale_boxes(boxes, padx, pady, gain, w, h):
    dev = _dev(boxes)
    if boxes.dtype != torch.float32 or not boxes.is_contiguous() or boxes.shape[-1] != 4:
        raise LmxError("scale_boxes: boxes must be dense float32 [...,4]")
    check(_lib.load().lmx_k_scale_boxes(_ptr(boxes), boxes.numel() // 4, float(padx), float(pady), float(gain), float(w),
                                        float(h), _stream(dev)), "lmx_k_scale_boxes")
    return boxes


def pose_gather(raws, strides, src, counts, kpt_shape, padx, pady, gain, w, h):
    """Keypoints of the detections NMS kept: raws = the three levels' cv4 outputs f32 [n,h,w,ldk]; src / counts from nms().
    -> f32 [n, max_det, K, ndim] in frame pixels (lmx_k_pose_gather)."""
    dev = _dev(*raws, src, counts)
    K_, ndim = kpt_shape
    ldk = raws[0].shape[-1]
    for r in raws:
        if r.dtype != torch.float32 or not r.is_contiguous() or r.dim() != 4 or r.shape[-1] != ldk:
            raise LmxError("pose_gather: levels must be dense float32 [n,h,w,ldk]")
    if src.dtype != torch.int32 or counts.dtype != torch.int32 or not src.is_contiguous():
        raise LmxError("pose_gather: src / counts must be int32")
    n, max_det = src.shape
    hw = (C.c_int32 * 6)(*[v for r in raws for v in (r.shape[1], r.shape[2])])
    st = (C.c_float * 3)(*[float(v) for v in strides])
    out = torch.empty((n, max_det, K_, ndim), dtype=torch.float32, device=src.device)
    check(_lib.load().lmx_k_pose_gather(_ptr(raws[0]), _ptr(raws[1]), _ptr(raws[2]), ldk, C.cast(hw, C.c_void_p),
                                        C.cast(st, C.c_void_p), _ptr(src), _ptr(counts), n, max_det, K_, ndim, float(padx),
                                        float(pady), float(gain), float(w), float(h), _ptr(out), _stream(dev)), "lmx_k_pose_gather")
    return out


def add_bcast(a, b, out=None, out_dtype=torch.float32):
    """out[r] = a[r] + b[r % b_rows]  (a, b float32 2-D; out float32 or float16)."""
    dev = _dev(a, b, out)
    rows, D_, lda = _rows(a, "add_bcast a")
    b_rows, Db, ldb = _rows(b, "add_bcast b")
    if Db != D_ or a.dtype not in _DT or b.dtype != torch.float32:
        raise LmxError("add_bcast: a must be float16/float32, b float32, equal width")
    if out is None:
        out = torch.empty((rows, D_), dtype=out_dtype, device=a.device)
    check(_lib.load().lmx_k_add_bcast(_ptr(a), _DT[a.dtype], lda, _ptr(b), ldb, b_rows, _ptr(out), _DT[out.dtype], out.stride(0),
                                      rows, D_, _stream(dev)), "lmx_k_add_bcast")
    return out


def attention_f32(q, k, v, B, H, Tq, Tk, hd, scale):
    """softmax(q k^T * scale) v in plain f32 for the SAM decoder's tiny attentions (lmx_k_attention_f32): q [B*Tq, >=H*hd],
    k / v [B*Tk, >=H*hd] f32 row views -> f32 [B*Tq, H*hd]."""
    dev = _dev(q, k, v)
    for t in (q, k, v):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise LmxError("attention_f32: q/k/v must be float32 2-D row views")
    out = torch.empty((B * Tq, H * hd), dtype=torch.float32, device=q.device)
    check(_lib.load().lmx_k_attention_f32(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(out), out.stride(0),
                                          B, H, Tq, Tk, hd, float(scale), _stream(dev)), "lmx_k_attention_f32")
    return out


def hyper_mask_f32(up, hyper, n, G, C_, act=ACT_NONE):
    dev = _dev(up, hyper)
    if up.dtype != torch.float32 or not up.is_contiguous():
        raise LmxError("hyper_mask_f32: up must be contiguous float32")
    logits = torch.empty((n, 4 * G, 4 * G), dtype=torch.float32, device=up.device)
    check(_lib.load().lmx_k_hyper_mask_f32(_ptr(up), _ptr(hyper), _ptr(logits), n, G, C_, act, _stream(dev)), "lmx_k_hyper_mask_f32")
    return logits


def split3_rows(x, act=ACT_NONE):
    """f32 [rows, N] (row stride allowed) -> contiguous x3 rows f16 [rows, 3N] = [hi | lo | hi] (one group): the A operand of an
    exact Linear (lmx_k_split3)."""
    dev = _dev(x)
    rows, N, ldx = _rows(x, "split3_rows x")
    if x.dtype != torch.float32 or N % 8:
        raise LmxError("split3_rows: float32 rows with N % 8 == 0 expected")
    out = torch.empty((rows, 3 * N), dtype=torch.float16, device=x.device)
    check(_lib.load().lmx_k_split3(_ptr(x), ldx, act, None, 0, _ptr(out), 3 * N, rows, N, N, 1, 0, _stream(dev)), "lmx_k_split3")
    return out


def prompt_box(boxes, sx, sy, S, gauss, corner):
    """boxes f32 [n,>=4] (row stride allowed) in frame pixels -> sparse f32 [n,2,2F] (lmx_k_prompt_box)."""
    dev = _dev(boxes, gauss, corner)
    n = boxes.shape[0]
    Fq = gauss.shape[1]
    out = torch.empty((n, 2, 2 * Fq), dtype=torch.float32, device=boxes.device)
    check(_lib.load().lmx_k_prompt_box(_ptr(boxes), boxes.stride(0), _ptr(out), n, float(sx), float(sy), float(S), _ptr(gauss),
                                       _ptr(corner), Fq, _stream(dev)), "lmx_k_prompt_box")
    return out


def hyper_mask(up, hyper, n, G, C_):
    dev = _dev(up, hyper)
    logits = torch.empty((n, 4 * G, 4 * G), dtype=torch.float32, device=up.device)
    check(_lib.load().lmx_k_hyper_mask(_ptr(up), _ptr(hyper), _ptr(logits), n, G, C_, _stream(dev)), "lmx_k_hyper_mask")
    return logits


def mask_post(logits, T, nh, nw, h, w):
    """-> (mask u8 [n,h,w], stats int64 [n,8] = area, sum_x, sum_y, min_x, min_y, max_x, max_y, 0)."""
    dev = _dev(logits)
    n, L, _ = logits.shape
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=logits.device)
    stats = torch.empty((n, 8), dtype=torch.int64, device=logits.device)
    ws = torch.empty((n, nh, nw), dtype=torch.float32, device=logits.device)
    check(_lib.load().lmx_k_mask_post(_ptr(logits), n, L, T, nh, nw, h, w, _ptr(mask), _ptr(stats), _ptr(ws), _stream(dev)),
          "lmx_k_mask_post")
    return mask, stats


def prompt_points(points, labels, boxes, sx, sy, S, gauss, point_embed, not_a_point, corner):
    """points f32 [n,Np,2], labels int32 [n,Np] (or both None with a box), boxes f32 [n,>=4] or None, frame pixels -> sparse
    f32 [n,Ns,2F] with Ns = Np + (2 if boxes else 1) (lmx_k_prompt_points).  Labels outside {-1,0,1} give NaN tokens."""
    dev = _dev(points, labels, boxes, gauss)
    Np = 0 if points is None else points.shape[1]
    if Np:
        if (points.dtype != torch.float32 or labels.dtype != torch.int32 or not points.is_contiguous() or not labels.is_contiguous()
                or points.dim() != 3 or points.shape[2] != 2 or tuple(labels.shape) != tuple(points.shape[:2])):
            raise LmxError("prompt_points: points must be contiguous f32 [n,Np,2], labels contiguous int32 [n,Np]")
    if boxes is not None and (boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] < 4 or boxes.stride(1) != 1):
        raise LmxError("prompt_points: boxes must be f32 [n,>=4] rows")
    n = points.shape[0] if Np else boxes.shape[0]
    if boxes is not None and boxes.shape[0] != n:
        raise LmxError("prompt_points: points and boxes disagree on n")
    Fq = gauss.shape[1]
    ldb = 0 if boxes is None else (boxes.stride(0) if n > 1 else boxes.shape[1])  # (a single row may carry any stride)
    out = torch.empty((n, Np + (2 if boxes is not None else 1), 2 * Fq), dtype=torch.float32, device=dev)
    check(_lib.load().lmx_k_prompt_points(_ptr(points if Np else None), _ptr(labels if Np else None), Np, _ptr(boxes), ldb,
                                          _ptr(out), n, float(sx), float(sy), float(S),
                                          _ptr(gauss), _ptr(point_embed), _ptr(not_a_point), _ptr(corner), Fq, _stream(dev)),
          "lmx_k_prompt_points")
    return out


MASK_EMBED_PARAMS = 4684  # LMX_MASK_EMBED_PARAMS


def mask_embed(mask_input, emb, params, G=64):
    """keys f32 [n*G*G,256] = emb (f32/f16 rows) + SamMaskEmbedding(mask_input f32 [n,4G,4G]) (lmx_k_mask_embed); params f32
    [MASK_EMBED_PARAMS] in lmx.h's order."""
    dev = _dev(mask_input, emb, params)
    rows, D_, lde = _rows(emb, "mask_embed emb")
    n = mask_input.shape[0]
    if (mask_input.dtype != torch.float32 or not mask_input.is_contiguous() or tuple(mask_input.shape[1:]) != (4 * G, 4 * G)
            or D_ != 256 or rows != n * G * G or emb.dtype not in _DT):
        raise LmxError(f"mask_embed: mask_input f32 [n,{4 * G},{4 * G}] and emb [n*{G * G},256] expected")
    if params.dtype != torch.float32 or params.numel() != MASK_EMBED_PARAMS or not params.is_contiguous():
        raise LmxError("mask_embed: params must be contiguous f32 [%d]" % MASK_EMBED_PARAMS)
    keys = torch.empty((rows, 256), dtype=torch.float32, device=dev)
    check(_lib.load().lmx_k_mask_embed(_ptr(mask_input), _ptr(emb), _DT[emb.dtype], lde, _ptr(params), _ptr(keys), 256, n, G,
                                       _stream(dev)), "lmx_k_mask_embed")
    return keys


def hyper_mask_multi(up, hyper, n, G, C_):
    """hyper f32 [n,M,C] against f16 up -> logits f32 [n,M,4G,4G] (lmx_k_hyper_mask_multi)."""
    dev = _dev(up, hyper)
    if hyper.dtype != torch.float32 or not hyper.is_contiguous() or hyper.dim() != 3 or hyper.shape[0] != n or hyper.shape[2] != C_:
        raise LmxError("hyper_mask_multi: hyper must be contiguous f32 [n,M,C]")
    M = hyper.shape[1]
    logits = torch.empty((n, M, 4 * G, 4 * G), dtype=torch.float32, device=up.device)
    check(_lib.load().lmx_k_hyper_mask_multi(_ptr(up), _ptr(hyper), _ptr(logits), n, M, G, C_, _stream(dev)), "lmx_k_hyper_mask_multi")
    return logits


def hyper_mask_multi_f32(up, hyper, n, G, C_, act=ACT_NONE):
    """hyper f32 [n,M,C] against f32 up -> logits f32 [n,M,4G,4G] (lmx_k_hyper_mask_multi_f32)."""
    dev = _dev(up, hyper)
    if up.dtype != torch.float32 or not up.is_contiguous():
        raise LmxError("hyper_mask_multi_f32: up must be contiguous float32")
    if hyper.dtype != torch.float32 or not hyper.is_contiguous() or hyper.dim() != 3 or hyper.shape[0] != n or hyper.shape[2] != C_:
        raise LmxError("hyper_mask_multi_f32: hyper must be contiguous f32 [n,M,C]")
    M = hyper.shape[1]
    logits = torch.empty((n, M, 4 * G, 4 * G), dtype=torch.float32, device=up.device)
    check(_lib.load().lmx_k_hyper_mask_multi_f32(_ptr(up), _ptr(hyper), _ptr(logits), n, M, G, C_, act, _stream(dev)),
          "lmx_k_hyper_mask_multi_f32")
    return logits


def mask_logits(logits, T, nh, nw, h, w):
    """Sam.postprocess_masks without the threshold: logits f32 [n,L,L] -> f32 [n,h,w] (lmx_k_mask_logits)."""
    dev = _dev(logits)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 3:
        raise LmxError("mask_logits: logits must be contiguous f32 [n,L,L]")
    n, L, _ = logits.shape
    out = torch.empty((n, h, w), dtype=torch.float32, device=logits.device)
    check(_lib.load().lmx_k_mask_logits(_ptr(logits), n, L, T, nh, nw, h, w, _ptr(out), _stream(dev)), "lmx_k_mask_logits")
    return out


def mask_score(logits, T, nh, nw, h, w, thr=0.0, off=1.0, idx=None):
    """SamAutomaticMaskGenerator's stability counts, area and box of (mask_logits(logits, ...) > thr) without the full-size
    logits: logits f32 [N,L,L] -> int64 [n,8] = count(v > thr + off), count(v > thr - off), area, min_x, min_y, max_x, max_y
    (inclusive; 0 0 0 0 when empty), 0 (lmx_k_mask_score).  idx: optional int32 [n] rows of `logits` to score (n = N
    without it); launches of at most 65535 rows."""
    dev = _dev(logits, idx)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 3:
        raise LmxError("mask_score: logits must be contiguous f32 [n,L,L]")
    N, L, _ = logits.shape
    if idx is not None:
        if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
            raise LmxError("mask_score: idx must be contiguous int32 [n]")
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
            raise LmxError(f"mask_score: idx outside 0..{N - 1}")
    n = N if idx is None else idx.numel()
    out = torch.empty((n, 8), dtype=torch.int64, device=logits.device)
    lib = _lib.load()
    for s in range(0, n, 65535):
        k = min(65535, n - s)
        src = logits[s:s + k] if idx is None else logits
        check(lib.lmx_k_mask_score(_ptr(src), k, L, T, nh, nw, h, w, float(thr), float(off), _ptr(None if idx is None else idx[s:s + k]),
                                   _ptr(out[s:s + k]), _stream(dev)), "lmx_k_mask_score")
    return out


NMS_BOXES_MAX = 16384


def nms_boxes(boxes, scores, iou, valid=None):
    """torchvision.ops.nms on device: boxes f32 [n,>=4] xyxy rows, scores f32 [n] (any sign), valid bool/u8 [n] or None ->
    (keep int32 [n]: kept indices in suppression order then -1, count int32 [1]) (lmx_k_nms_boxes)."""
    dev = _dev(boxes, scores, valid)
    n, cols, ldb = _rows(boxes, "nms_boxes boxes")
    if boxes.dtype != torch.float32 or cols < 4 or scores.dtype != torch.float32 or tuple(scores.shape) != (n,) or not scores.is_contiguous():
        raise LmxError("nms_boxes: boxes f32 [n,>=4] and scores contiguous f32 [n] expected")
    if not 0 < n <= NMS_BOXES_MAX:
        raise LmxError(f"nms_boxes: {n} candidates (1..{NMS_BOXES_MAX})")
    if valid is not None:
        if valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (n,):
            raise LmxError("nms_boxes: valid must be bool / uint8 [n]")
        valid = valid.contiguous().view(torch.uint8)
    keep = torch.empty((n,), dtype=torch.int32, device=boxes.device)
    count = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    ws = torch.empty((n * 5,), dtype=torch.float32, device=boxes.device)
    check(_lib.load().lmx_k_nms_boxes(_ptr(boxes), ldb, _ptr(scores), _ptr(valid), n, float(iou), _ptr(keep), _ptr(count), _ptr(ws),
                                      _stream(dev)), "lmx_k_nms_boxes")
    return keep, count


def contour_features(mask):
    """mask u8 [n,h,w] (0 / non-0) on device -> int64 [n,8] = 2*contourArea, unit steps, diagonal steps, min x, min y, max x,
    max y, number of external contours of the largest external contour (lmx_k_contour_features, csrc/contour.hip)."""
    dev = _dev(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous():
        raise LmxError("contour_features: mask must be contiguous uint8 [n,h,w]")
    n, h, w = mask.shape
    lib = _lib.load()
    ws = torch.empty((int(lib.lmx_contour_workspace_bytes(n, h, w)),), dtype=torch.uint8, device=mask.device)
    out = torch.empty((n, 8), dtype=torch.int64, device=mask.device)
    check(lib.lmx_k_contour_features(_ptr(mask), n, h, w, _ptr(out), _ptr(ws), _stream(dev)), "lmx_k_contour_features")
    return out


# ---- optional per-launch timing (bench.py's roofline leg) -----------------------------------------------------------
# While a trace is active every lmx_k_* entry point is bracketed by a HIP event pair recorded on the stream the launch goes
# to (torch's current stream of the operands' device), together with the ALGORITHMIC work of the call: flops and the minimal
# bytes its operands and results occupy (no re-reads, no workspace) - DESIGN.md section 3 states the per-unit figures.
LAUNCH_TRACE = None
_raw_lib = None
RIDGE_FLOP_PER_BYTE = 2500e12 / 8e12  # dense f16 MFMA peak / HBM peak (MI355X_MICROARCH.md): above it a launch is MFMA-bound


def _work(name, args):
    """(class, flops, bytes) of one C-ABI call; bytes None = not modelled (pre/post-processing glue: time share only)."""
    if name == "lmx_k_gemm":
        d = args[0]._obj
        M, N, Kd = d.M, d.N, d.K
        osz = 4 if d.out_dtype == F32 else 2
        a_bytes = 2 * M * (Kd // max(d.a_rep, 1))
        if d.a_mode == 1:  # 3x3 implicit GEMM: the input image is read once, not 9 times
            a_bytes = 2 * (M // max(d.Ho * d.Wo, 1)) * d.H * d.W_ * d.Cin
        by = a_bytes + 2 * N * Kd + osz * (M // 4 if d.a_mode == 2 else M) * (N // 2 if d.act == ACT_SWIGLU else N) + (osz * (d.res_rows or M) * N if d.res else 0)
        by += 2 * M * N if d.ln_out else 0  # the f16 LayerNorm rows of the same launch
        fl = 2.0 * M * N * Kd
        key = f"gemm M={M} N={N} K={Kd} out={'f32' if osz == 4 else 'f16'} conv3x3={d.a_mode} act={d.act} res={int(bool(d.res))}" + (" ln_out" if d.ln_out else "")
        return ("gemm/mfma-bound" if fl / by >= RIDGE_FLOP_PER_BYTE else "gemm/hbm-bound"), fl, by, key
    if name == "lmx_k_attention":
        d = args[0]._obj
        fl = 4.0 * d.B * d.H * d.Tq * d.Tk * d.hd
        by = 2 * d.H * d.hd * d.B * (2 * d.Tq + 2 * d.Tk)
        key = f"attention B={d.B} H={d.H} Tq={d.Tq} Tk={d.Tk} hd={d.hd} mode={d.mode} ws={d.ws} qs={d.q_stride} rel={int(bool(d.rel))}"
        return ("attention/mfma-bound" if fl / by >= RIDGE_FLOP_PER_BYTE else "attention/hbm-bound"), fl, by, key
    if name == "lmx_k_layernorm":
        in_dt, out_dt, rows, D = args[1], args[6], args[8], args[9]
        return "layernorm", 0.0, rows * D * ((4 if in_dt == F32 else 2) + (4 if out_dt == F32 else 2)), f"layernorm rows={rows} D={D} in={in_dt} out={out_dt}"
    if name == "lmx_k_ln_mlp_img":
        rows, D = args[4], args[5]
        return "fused ln+mlp", 16.0 * D * D * rows, (8 + (2 if args[7] else 0) + (2 if args[8] else 0)) * D * rows, f"ln_mlp_img rows={rows} D={D}"
    if name == "lmx_k_ln_mlp":
        rows, D = args[8], args[9]
        return "fused ln+mlp", 16.0 * D * D * rows, (16 + (2 if args[12] else 0) + (2 if args[15] else 0)) * D * rows, f"ln_mlp rows={rows} D={D}"
    # the attention half of a Hiera block as one launch (csrc/hiera.hip): algorithmic flops of the unpadded products, bytes = the
    # f32 stream read + written (+ the f16 LayerNorm rows where they are an input)
    if name == "lmx_k_hiera_attn8":
        n_, Gh, Gw, D = args[10], args[11], args[12], args[13]
        rows = n_ * Gh * Gw
        return "fused attention half", rows * (8.0 * D * D + 256.0 * D), rows * D * (8 + (2 if args[0] else 0)), f"hiera_attn8 rows={rows} D={D} ln_inside={int(not args[0])}"
    if name == "lmx_k_hiera_attn4":
        n_, Gh, Gw, D = args[5], args[6], args[7], args[8]
        rows = n_ * Gh * Gw
        return "fused attention half", rows * (8.0 * D * D + 64.0 * D), rows * D * 10, f"hiera_attn4 rows={rows} D={D}"
    if name == "lmx_k_hiera_attn_pool":
        n_, Gh, Gw, Di, Do = args[4], args[5], args[6], args[7], args[8]
        rows = n_ * Gh * Gw
        keys = 64 if Di == 112 else 16  # tokens of a window
        return "fused attention half", rows * (8.0 * Di * Do + keys * Do + 0.5 * Do * Do), rows * (2 * Di + Do), f"hiera_attn_pool rows={rows} {Di}->{Do}"
    # streaming element-wise glue with a plain byte count: one HBM-bound class of its own (the rest — resizes, im2col, NMS,
    # mask_post, contour features, decode — stays "pre/post-processing and glue": time share only)
    if name == "lmx_k_cast_f32_f16":
        rows, cols = args[4], args[5]
        return "streaming glue", 0.0, 6 * rows * cols, f"cast_f32_f16 rows={rows} cols={cols}"
    if name == "lmx_k_maxpool2":
        dt, n_, H, W, C_ = args[4], args[5], args[6], args[7], args[8]
        esz = 4 if dt == F32 else 2
        return "streaming glue", 0.0, esz * n_ * H * W * C_ * 5 // 4, f"maxpool2 n={n_} H={H} W={W} C={C_} dtype={dt}"
    if name == "lmx_k_upsample2":
        n_, H, W, C_ = args[4], args[5], args[6], args[7]
        return "streaming glue", 0.0, 2 * n_ * H * W * C_ * 5, f"upsample2 n={n_} H={H} W={W} C={C_}"
    if name == "lmx_k_add_bcast":
        a_dt, o_dt, rows, D = args[1], args[7], args[9], args[10]
        return "streaming glue", 0.0, rows * D * ((4 if a_dt == F32 else 2) + (4 if o_dt == F32 else 2)), f"add_bcast rows={rows} D={D}"
    if name == "lmx_k_band_join":
        dt, n_, H, Hb, W, D = args[3:9]
        return "streaming glue", 0.0, 2 * (4 if dt == F32 else 2) * n_ * H * W * D, f"band_join n={n_} H={H} Hb={Hb} W={W} D={D} dtype={dt}"
    if name == "lmx_k_rope":
        B, T, H, hd = args[2], args[3], args[4], args[5]
        return "streaming glue", 0.0, 2 * 2 * 2 * B * T * H * hd, f"rope B={B} T={T} H={H} hd={hd}"  # q and k, read + written, f16
    return "pre/post-processing and glue", 0.0, None, name


def _install_trace():
    global _raw_lib
    if _raw_lib is not None:
        return
    lib = _raw_lib = _lib.load()

    def make(name, fn):
        def traced(*args):
            if LAUNCH_TRACE is None:
                return fn(*args)
            cls, fl, by, key = _work(name, args)
            st = torch.cuda.current_stream(_tls.dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = fn(*args)
            e1.record(st)
            LAUNCH_TRACE.append((cls, key, fl, by, e0, e1))
            return rc

        return traced

    class _Proxy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("lmx_k_"):
                fn = make(name, fn)
            setattr(self, name, fn)
            return fn

    _lib._lib = _Proxy()


def start_launch_trace():
    global LAUNCH_TRACE
    _install_trace()
    LAUNCH_TRACE = []


def stop_launch_trace(by_shape=False):
    """-> {class: dict(launches, seconds, flops, bytes)} over the traced launches (events read after a device sync);
    by_shape=True keys the table by (class, operand shape) instead."""
    global LAUNCH_TRACE
    tr, LAUNCH_TRACE = LAUNCH_TRACE or [], None
    torch.cuda.synchronize()
    out, shapes = {}, {}
    for cls, key, fl, by, e0, e1 in tr:
        dt = e0.elapsed_time(e1) * 1e-3
        for table, k in ((out, cls), (shapes, (cls, key))):
            r = table.setdefault(k, dict(launches=0, seconds=0.0, flops=0.0, bytes=0.0, modelled=by is not None))
            r["launches"] += 1
            r["seconds"] += dt
            r["flops"] += fl
            r["bytes"] += by or 0.0
    return (out, shapes) if by_shape else out
