"""Which kernel lmx_k_gemm, lmx_k_attention and lmx_k_layernorm pick, asked of the library's own selection without a GPU
(lmx_h_gemm_route / lmx_h_attn_route / lmx_h_layernorm_route through lmx.kernels.*_route).  The three choose from sizes that grow
with the batch, and a frame's bits must not depend on the batch (Reproducibility): the GPU tests that guard this cross the
thresholds by shape, and the tables of tests/test_gpu_dispatch.py and tests/test_gpu_attention.py say which kernel each shape
reaches.  Here every row of those tables is held to the selection, so a threshold that moves fails a test instead of leaving the GPU
tests on one side of it; the Python-side rules that must agree with the C rules (pooled_gemm_ok, split_k_for) are compared with
them, and the route functions must reject what the launchers reject."""
import pytest
import torch

import test_gpu_attention as GA
import test_gpu_dispatch as GD
from lmx import kernels as K
from lmx import yolo

F16, F32 = torch.float16, torch.float32
CU_COUNTS = (64, 104, 256, 304)  # for the table rows that are functions of the device's CU count


# ------------------------------------------------------------------------------------------------ GEMM and convolution tables
@pytest.mark.parametrize("N,K_,M,sizes,form", GD.CASES, ids=[f"N{c[0]}K{c[1]}-{c[4]}" for c in GD.CASES])
def test_gemm_table(N, K_, M, sizes, form):
    routes = GD.gemm_case_routes(N, K_, form)
    for rows in [M] + GD.gemm_case_sizes(M, sizes, form):
        assert K.gemm_route(rows, N, K_, **GD.FORM_ROUTE_ARGS[form]) == routes[rows], f"{rows} rows"


@pytest.mark.parametrize("label,n,sizes,H,W,cin,cout,stride,form,routes", GD.CONV_CASES, ids=[c[0] for c in GD.CONV_CASES])
def test_conv_table(label, n, sizes, H, W, cin, cout, stride, form, routes):
    for frames in [n] + sizes:
        got = K.conv3x3_route(frames, H, W, cin, cout, stride=stride, **GD.CONV_FORM_ROUTE_ARGS[form])
        assert got == routes[frames], f"{frames} frames"


def test_split_k_case():
    n, H, W, cin, cout, S, routes = GD.SPLIT_K_CASE
    for frames in (n, 1):
        assert K.conv3x3_route(frames, H, W, cin, cout, out_dtype=F32, act=K.ACT_NONE, scale=True, split_k=S) == routes[frames]


def test_gemm_tables_reach_every_route_they_claim():
    """What the comments of tests/test_gpu_dispatch.py claimed before they became tables: both register-staged tiles, the four
    dense tilings, both convolution tilings."""
    dense = set().union(*(r.values() for *_, r in GD.SHAPES), GD.AREP_ROUTES.values())
    assert dense == {GD.V1, GD.DMA_STAG, GD.DMA_Z, GD.DMA_C, GD.DMA_E}
    conv = set().union(*(c[-1].values() for c in GD.CONV_CASES), GD.SPLIT_K_CASE[-1].values())
    assert conv == {GD.V1, GD.V1_N64, GD.DMA_C, GD.DMA_Y}


# ------------------------------------------------------------------------------------------------ attention tables
@pytest.mark.parametrize("sid,fam,shape,rel_S,kinds,route", GA.SHAPES, ids=[s[0] for s in GA.SHAPES])
def test_attention_table(sid, fam, shape, rel_S, kinds, route):
    for cu in (CU_COUNTS if callable(shape) else (None,)):  # rows that grow with the CU count: the same route at every count
        assert GA.shape_route(shape, rel_S, cu) == route
    # the id and the family say what the route says
    word = {"small": "small", "sp": "sp_qb2_", "spp": "spp_", "gp": "gp4_", "kernel": "tiled_", "wide": "tiled_q1_dot2_hd96", "rel": "_rel_"}[fam]
    assert word in route
    for qb in (1, 2):
        assert f"kernel<{qb}>" not in sid or route.startswith(f"tiled_q{qb}_")
    for sums in ("ones", "dot2"):
        assert f" {sums} " not in sid or f"_{sums}" in route
    assert ("wide" in sid) == route.endswith("_hd96")


def test_many_item_rows_sample_a_whole_walk():
    """The rows that grow with the CU count: at every count each workgroup of the persistent kernel walks three or four items, and the
    row sample holds the items at positions 0, 1, 2 and last of one workgroup (GA.walked_sample asserts both)."""
    many = [s for s in GA.SHAPES if callable(s[2])]
    assert len(many) == 2
    for cu in CU_COUNTS:
        for sid, _, shape, *_ in many:
            geo = GA._geo(shape(cu))
            assert 3 * cu < geo.B * geo.H <= 3 * cu + 16, sid
            rows, _ = GA.walked_sample(geo, cu)
            assert len(rows) < geo.q_rows // 20


def test_attention_table_reaches_every_route_it_claims():
    got = {s[-1] for s in GA.SHAPES}
    assert got == {"small", "sp_qb2_ones", "sp_qb2_dot2", "spp_ones", "spp_dot2", "gp4_ones", "gp4_dot2", "tiled_q1_ones_hd64",
                   "tiled_q1_dot2_hd64", "tiled_q2_ones_hd64", "tiled_q2_dot2_hd64", "tiled_q1_dot2_hd96", "tiled_q1_dot2_rel_hd64",
                   "tiled_q2_dot2_rel_hd64", "tiled_q1_dot2_rel_hd96"}


@pytest.mark.parametrize("label,H,B,sizes,hd,window,routes", GD.ATTN_CASES, ids=[c[0] for c in GD.ATTN_CASES])
def test_batch_independence_attention_table(label, H, B, sizes, hd, window, routes):
    T = 201 if window is None else 196
    for cu in (CU_COUNTS if callable(B) else (None,)):
        batches = GD.attn_case_batches(B, sizes, window, cu)
        assert sum(batches[1:]) == batches[0]
        for i, b in enumerate(batches):
            assert K.attention_route(b, H, T, T, hd, window=window, pad=window is not None, ld=3 * H * hd) == routes[min(i, 1)], f"B = {b}"


def test_attention_edges():
    """Both sides of every threshold of attn_route."""
    r = K.attention_route
    assert (r(63, 1, 201, 201, 64), r(64, 1, 201, 201, 64)) == ("sp_qb2_dot2", "spp_dot2")            # items 63 / 64
    assert (r(9, 7, 201, 201, 64), r(8, 8, 201, 201, 64)) == ("sp_qb2_dot2", "spp_dot2")              # ... as B x H
    assert (r(2, 2, 256, 256, 64), r(2, 2, 257, 257, 64)) == ("gp4_dot2", "gp4_dot2")                 # T 256 / 257: both LDS-DMA
    assert (r(2, 2, 255, 255, 64), r(2, 2, 256, 256, 56)) == ("tiled_q2_dot2_hd64", "gp4_ones")       # Tk 255 / 256
    assert [r(2, 3, 208, tk, 64) for tk in (128, 129, 208, 209)] == ["tiled_q2_dot2_hd64", "sp_qb2_dot2", "sp_qb2_dot2", "tiled_q2_dot2_hd64"]
    assert [r(2, 3, tq, 208, 56) for tq in (64, 65, 208, 209)] == ["tiled_q1_ones_hd64", "sp_qb2_ones", "sp_qb2_ones", "tiled_q2_ones_hd64"]
    assert [r(2, 3, 201, 201, hd) for hd in (56, 64, 72)] == ["sp_qb2_ones", "sp_qb2_dot2", "tiled_q1_dot2_hd96"]
    assert [r(1, 2, 300, 300, hd) for hd in (56, 64, 72)] == ["gp4_ones", "gp4_dot2", "tiled_q1_dot2_hd96"]
    assert [r(2, 3, 17, 300, hd) for hd in (56, 64, 72)] == ["tiled_q1_ones_hd64", "tiled_q1_dot2_hd64", "tiled_q1_dot2_hd96"]
    assert (r(3, 5, 16, 16, 64), r(3, 5, 17, 16, 64), r(3, 5, 16, 17, 64), r(3, 5, 16, 16, 72)) == (
        "small", "tiled_q1_dot2_hd64", "tiled_q1_dot2_hd64", "tiled_q1_dot2_hd96")
    # windows reach the persistent kernel only with both pad vectors
    w = dict(Gh=20, Gw=20, ws=14, q_stride=1)
    assert (r(16, 4, 196, 196, 56, window=w, pad=True), r(16, 4, 196, 196, 56, window=w)) == ("spp_ones", "sp_qb2_ones")
    # K / V of one batch element beyond a 31-bit buffer: no LDS-DMA
    assert (r(1, 1, 4096, 4096, 64, ld=3072), r(1, 1, 4096, 262144, 64, ld=4096)) == ("gp4_dot2", "tiled_q2_dot2_hd64")


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_edges():
    r = K.layernorm_route
    assert (r(16383, 768), r(16384, 768)) == ("row_it4", "rows_it4")                       # rows 16383 / 16384
    assert (r(16383, 512), r(16384, 512)) == ("row_it2", "rows_it2")
    for rows in (7, 16384, 100000):
        assert (r(rows, 128), r(rows, 132)) == ("narrow", "rows_it2" if rows >= 16384 else "row_it2")   # D 128 / 132
    assert (r(100, 512), r(100, 516)) == ("row_it2", "row_it4")                            # D 512 / 516
    assert (r(100, 1024), r(100, 1028), r(100, 4096)) == ("row_it4", "row_it16", "row_it16")   # D 1024 / 1028
    assert (r(16384, 1024), r(16384, 1028)) == ("rows_it4", "row_it16")                    # the rows kernel ends at D = 1024
    # the dtype pairs and the activation that keep the rows kernel out
    for i, o in ((F32, F32), (F16, F16), (F16, F32)):
        assert (r(16384, 768, i, o), r(16384, 128, i, o)) == ("row_it4", "narrow")
    assert r(16384, 768, F32, F16, K.ACT_GELU) == "row_it4"
    assert r(16384, 768, F32, F16, K.ACT_NONE) == "rows_it4"


# ------------------------------------------------------------------------------------------------ Python rules against the C rules
def _validates(fn, *a, **kw):
    try:
        fn(*a, **kw)
        return True
    except K.LmxError:
        return False


@pytest.mark.parametrize("M", [256, 508, 512, 516])
@pytest.mark.parametrize("N", [88, 96, 100, 104])
def test_pooled_gemm_ok_is_the_c_rule(M, N):
    """pooled_gemm_ok(M, N) == "the a_mode-2 route validates", on an even token grid (2 x M/2 tokens)."""
    for out in (F16, F32):
        assert K.pooled_gemm_ok(M, N) == _validates(K.gemm_route, M, N, 112, out_dtype=out, pool_hw=(2, M // 2))
    if K.pooled_gemm_ok(M, N):
        assert K.gemm_route(M, N, 112, out_dtype=F32, pool_hw=(2, M // 2)) == "dma_256x256x64_s2"


def exact_conv3x3_layers(cfg, H, W):
    """(name, H, W, Cin, Cout, stride) of every 3 x 3 convolution the exact plan runs through lmx_k_gemm on an H x W letterboxed
    frame (everything but the stem), from lmx.yolo.layer_table / param_spec."""
    table, spec = yolo.layer_table(cfg), yolo.param_spec(cfg)
    hw, out = [], []

    def conv(name, h, w, stride=1):
        co, ci, k, _ = spec[name + ".conv.weight"][0]
        assert k == 3
        out.append((name, h, w, ci, co, stride))

    for i, m in enumerate(table):
        p = f"model.{i}"
        h, w = (H, W) if i == 0 else hw[i - 1]
        if m["kind"] == "conv":
            if i:
                conv(p, h, w, 2)
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        elif m["kind"] == "c2f":
            for j in range(m["n"]):
                conv(f"{p}.m.{j}.cv1", h, w)
                conv(f"{p}.m.{j}.cv2", h, w)
        elif m["kind"] == "up":
            h, w = 2 * h, 2 * w
        elif m["kind"] == "detect":
            for l, src in enumerate(m["src"]):
                for name in (f"{p}.cv2.{l}.0", f"{p}.cv2.{l}.1", f"{p}.cv3.{l}.0", f"{p}.cv3.{l}.1"):
                    conv(name, *hw[src])
        hw.append((h, w))
    assert len(out) == sum(1 for k, (s, _) in spec.items() if k.endswith(".conv.weight") and s[2] == 3) - 1
    return out


@pytest.mark.parametrize("H,W", [(384, 640), (1088, 1920)], ids=["640x384", "1920x1088"])
def test_split_k_for_is_valid_and_independent_of_the_batch(H, W):
    """YOLOv8-l's exact plan on 1080p frames letterboxed to 640 (384 rows) and to 1920 (1088 rows): wherever split_k_for splits a
    layer, lmx_k_gemm takes the split, and its kernel for 1 frame is its kernel for 32 unless the convolution t256 rule (N % 256 == 0,
    t256 >= 230, q256 >= 0.75; GD.SPLIT_K_CASE crosses it on the GPU) puts the 32 frames on 256 x 256 tiles."""
    split = 0
    for name, h, w, ci, co, stride in exact_conv3x3_layers(yolo.YoloConfig("l"), H, W):
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        s = K.split_k_for(ho * wo, co, 27 * ci, 3 * ci)  # the exact plan's x3 operands: 3 Cin channels, K = 27 Cin
        if s == 1:
            continue
        split += 1
        for n in (1, 32):  # one name for both, unless the t256 rule says otherwise
            t256 = -(-n * ho * wo // 256) * -(-co // 256)
            big = co % 256 == 0 and t256 >= 230 and t256 / (-(-t256 // 256) * 256) >= 0.75
            got = K.conv3x3_route(n, h, w, 3 * ci, co, stride=stride, out_dtype=F32, act=K.ACT_NONE, scale=True, split_k=s)
            assert got == (GD.DMA_Y if big else GD.DMA_C), (name, n)
    assert split > 0


def test_split_k_for_first_line_is_the_c_rule():
    """split_k_for returns 1 exactly where the LDS-DMA kernel's split_k shapes end: N >= 64, N % 8 == 0, Cin % 32 == 0."""
    for co in (56, 60, 64, 68, 72):
        for ci in (16, 32, 48, 64):
            ok = _validates(K.conv3x3_route, 1, 16, 16, ci, co, out_dtype=F32, act=K.ACT_NONE, split_k=2)
            assert ok == (co >= 64 and co % 8 == 0 and ci % 32 == 0), (co, ci)
            if not ok:
                assert K.split_k_for(256, co, 9 * ci, ci) == 1


# ------------------------------------------------------------------------------------------------ what the launchers reject
def _gemm_desc(**kw):
    d = K.GemmDesc()
    d.A = d.W = d.C = K._ROUTE_PTR
    d.M, d.N, d.K, d.lda, d.ldc = 1024, 256, 256, 256, 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _attn_desc(**kw):
    d = K.AttnDesc()
    d.Q = d.K = d.V = d.O = K._ROUTE_PTR
    d.B, d.H, d.Tq, d.Tk, d.hd = 2, 2, 64, 64, 64
    d.ldq = d.ldk = d.ldv = d.ldo = 128
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rejections():
    import ctypes as C

    lib = K._lib.load()
    name = C.create_string_buffer(64)
    null = C.c_void_p(0)

    def gemm(**kw):
        d = _gemm_desc(**kw)
        return lib.lmx_h_gemm_route(C.byref(d), name, 64), lambda: lib.lmx_k_gemm(C.byref(d), null)

    def attn(**kw):
        d = _attn_desc(**kw)
        return lib.lmx_h_attn_route(C.byref(d), name, 64), lambda: lib.lmx_k_attention(C.byref(d), null)

    def ln(D):
        p = C.c_void_p(K._ROUTE_PTR)
        return (lib.lmx_h_layernorm_route(K.F32, K.F16, 8, D, K.ACT_NONE, name, 64),
                lambda: lib.lmx_k_layernorm(p, K.F32, D, p, p, p, K.F16, D, 8, D, 1e-5, K.ACT_NONE, null))

    return [
        ("K % 8", lambda: gemm(K=252, lda=252), "K=252 must be a multiple of 8"),
        ("bad a_mode", lambda: gemm(a_mode=3), "bad a_mode 3"),
        ("SWIGLU with a residual", lambda: gemm(act=K.ACT_SWIGLU, res=K._ROUTE_PTR, ldr=256), "LMX_ACT_SWIGLU takes no residual"),
        ("pooled rows below the LDS-DMA shapes", lambda: gemm(a_mode=2, H=2, W_=128, M=256, out_dtype=K.F32), "pooled rows are built for"),
        ("split_k on 56 channels", lambda: gemm(split_k=2, N=56, ldc=56, out_dtype=K.F32, split_stride=1024 * 56), "split_k is built into"),
        ("a_rep below 512 rows", lambda: gemm(a_rep=2, M=256, out_dtype=K.F32), "a_rep is built into"),
        ("hd 100", lambda: attn(hd=100, ldq=200, ldk=200, ldv=200, ldo=200), "head dim 100"),
        ("rel_S mismatch", lambda: attn(rel=K._ROUTE_PTR, rel_S=7), "rel_S=7 does not match Tq=64 Tk=64"),
        ("window geometry", lambda: attn(mode=1, Gh=12, Gw=12, ws=8, q_stride=3), "q_stride 3"),
        ("LayerNorm D % 4", lambda: ln(130), "rows=8 D=130"),
    ]


@pytest.mark.parametrize("i", range(10), ids=lambda i: _rejections()[i][0])
def test_route_rejects_what_the_launcher_rejects(i):
    """One descriptor per group of requirements: the route function and the launcher return LMX_EINVAL with the same text.  (An
    invalid descriptor never reaches a launch, so the launcher may be called without a GPU, on the null stream.)"""
    lib = K._lib.load()
    _, make, text = _rejections()[i]
    rc_route, launch = make()
    msg_route = lib.lmx_last_error().decode()
    assert rc_route == -1 and text in msg_route, msg_route
    assert launch() == -1 and lib.lmx_last_error().decode() == msg_route


def test_route_functions_raise_lmx_error():
    with pytest.raises(K.LmxError, match="multiple of 8"):
        K.gemm_route(1024, 256, 252)
    with pytest.raises(K.LmxError, match="head dim 100"):
        K.attention_route(2, 2, 64, 64, 100)
    with pytest.raises(K.LmxError, match="rel_S"):
        K.attention_route(2, 2, 64, 64, 64, rel_S=7)
    with pytest.raises(K.LmxError, match="D=130"):
        K.layernorm_route(8, 130)


def test_name_buffer_too_short():
    import ctypes as C

    lib = K._lib.load()
    d = _gemm_desc()
    name = C.create_string_buffer(4)
    assert lib.lmx_h_gemm_route(C.byref(d), name, 4) == -1 and "too short" in lib.lmx_last_error().decode()
