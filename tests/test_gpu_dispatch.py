"""A frame's bits do not depend on the batch it rides in: lmx_k_gemm picks its kernel and tiling from M
(csrc/gemm.hip lmx_k_gemm: register-staged 128 x 64 / 128 x 128 below M = 512, or for 3 x 3 convolutions with N = 64 below
M = 65536; csrc/gemm2.hip lmx_gemm2_launch: four dense tilings keyed on tiles256 / q256 / tiles, two convolution tilings keyed on
t256 >= 230).  Every one of them must return the same bits for the same output rows: the same 16x16x32 MFMA in the same k order
and one rounding sequence in every epilogue.

GEMM level: one problem computed whole, then again in row chunks whose sizes land in the OTHER branches; the concatenation must
be torch.equal to the whole.  The branch of each chunk is a row of the route tables below: every case asserts, before it launches,
that the library's own selection (lmx.kernels.gemm_route / conv3x3_route / attention_route) names that kernel for it, and
tests/test_dispatch_routes_host.py holds the same tables to the selection without a GPU.  Model level: a frame / prompt alone against the same frame / prompt inside a batch that crosses the thresholds.
Branches are reached by shape only (the LMX_GEMM_* development switches are process-wide and would leak into later tests).

lmx_k_layernorm switches on rows = frames x tokens too (layernorm_rows_kernel from 16384 rows): that threshold is crossed by
tests/test_gpu_rowwise.py::test_layernorm_bits_do_not_depend_on_the_row_count, beside the float64 comparison of both kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _chunked(fn, M, sizes):
    """fn(r0, r1) -> rows [r0, r1) of the result; the chunks' results concatenated."""
    assert sum(sizes) == M
    out, r0 = [], 0
    for s in sizes:
        out.append(fn(r0, r0 + s))
        r0 += s
    return torch.cat(out, 0)


def _assert_equal(got, whole, what):
    if not torch.equal(got, whole):
        bad = (got != whole).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError(f"{what}: {len(bad)} rows differ from the whole problem's, first {bad[:8].tolist()}")


# the route names of lmx_h_gemm_route (include/lmx.h): register-staged 128 x BN, or LDS-DMA BM x BN x BK, ring slots, staggered
V1, V1_N64 = "v1_128x128", "v1_128x64"
DMA_STAG, DMA_Z, DMA_C = "dma_256x128x64_s3_stag", "dma_256x256x64_s2", "dma_256x128x32_s3"
DMA_E, DMA_Y = "dma_256x256x32_s3", "dma_256x256x32_s3_stag"

# N = 1792, K = 448 (the fc1 of Hiera stage 3).  Rows -> route:
#     500 (M < 512) | 4096 (tiles256 = 112, tiles = 224 <= 256) | 8192 (tiles256 = 224, q256 = 0.875) |
#     12000 (tiles256 = 329, q256 = 0.64; tiles = 658) | whole 24788 (tiles256 = 679, q256 = 0.88)
DENSE_SIZES = [500, 4096, 8192, 12000]
DENSE_ROUTES = {500: V1, 4096: DMA_STAG, 8192: DMA_Z, 12000: DMA_C, 24788: DMA_Z}
# the same shape with a_rep 2 (K = 896 in the descriptor; M >= 512 only): 20180 rows have tiles256 = 553, q256 = 0.72
AREP_ROUTES = {512: DMA_STAG, 4096: DMA_STAG, 20180: DMA_C, 24788: DMA_Z}
# short K (256 x 256 short-K rule: K < 448, N = 224 .. 1536 not a multiple of 256, tiles256 >= 200, q256 >= 0.75):
#     N = 672, K = 112: 17152 rows -> 64-deep short K (tiles256 201); 16896 (tiles256 198)
#     N = 1344, K = 224: 8704 rows -> 32-deep short K (tiles256 204); 8448 (198)
# (N, K, M, chunk sizes, {rows: route} for M and every chunk size)
SHAPES = [(1792, 448, 24788, DENSE_SIZES, DENSE_ROUTES),
          (672, 112, 17152, [16896, 256], {17152: DMA_Z, 16896: DMA_C, 256: V1}),
          (1344, 224, 8704, [8448, 256], {8704: DMA_E, 8448: DMA_C, 256: V1})]

FORMS = ["f16_silu_res", "f16_gelu_res", "f32_scale_res", "f32_res_rows", "a_rep2"]
# what gemm_route needs to know of a form (the activation does not enter the selection)
FORM_ROUTE_ARGS = {
    "f16_silu_res": dict(out_dtype=torch.float16, res=True),
    "f16_gelu_res": dict(out_dtype=torch.float16, scale=True, res=True),
    "f32_scale_res": dict(out_dtype=torch.float32, scale=True, res=True),
    "f32_res_rows": dict(out_dtype=torch.float32, scale=True, res=True, res_rows=4),
    "a_rep2": dict(out_dtype=torch.float32, scale=True, res=True, a_rep=2),
}
# (a_rep needs K % 64 == 0: the N = 1792 / K = 448 shape only)
CASES = [(N, K, M, sizes, f) for N, K, M, sizes, _ in SHAPES for f in FORMS if f != "a_rep2" or K % 64 == 0]


def gemm_case_sizes(M, sizes, form):
    """The chunk sizes a case of CASES runs (a_rep needs M >= 512: the LDS-DMA kernel only)."""
    if form == "a_rep2":
        return [4096, M - 4096 - 512, 512] if M > 9000 else [M - 512, 512]
    return sizes


def gemm_case_routes(N, K, form):
    """{rows: route} of a case of CASES: the whole problem and every chunk size."""
    return AREP_ROUTES if form == "a_rep2" else next(r for n, k, _, _, r in SHAPES if (n, k) == (N, K))


@pytest.mark.parametrize("N,K,M,sizes,form", CASES, ids=[f"N{c[0]}K{c[1]}-{c[4]}" for c in CASES])
def test_gemm_rows_are_independent_of_the_batch(cuda, N, K, M, sizes, form):
    """The forms the plans launch: f16 out with SiLU / GELU and an f16 residual (YOLO, ViT MLPs), f32 out with LayerScale and
    the residual stream (ViT blocks; the exact plan's scale), a res_rows-broadcast table (patch embed + position table), a_rep 2
    (the SAM ViT exact plan)."""
    from lmx import kernels as K_

    g = torch.Generator(device=cuda).manual_seed(N + K)
    a = torch.randn((M, K), device=cuda, generator=g).half()
    w = (torch.randn((N, 2 * K if form == "a_rep2" else K), device=cuda, generator=g) * K ** -0.5).half()
    b = torch.randn((N,), device=cuda, generator=g)
    s = torch.rand((N,), device=cuda, generator=g) + 0.5
    res_rows = 4
    if form == "f32_res_rows":
        res = torch.randn((res_rows, N), device=cuda, generator=g)
    else:
        res = torch.randn((M, N), device=cuda, generator=g)
        res = res.half() if form.startswith("f16") else res
    sizes = gemm_case_sizes(M, sizes, form)
    routes = gemm_case_routes(N, K, form)
    for rows in [M] + sizes:
        assert K_.gemm_route(rows, N, K, **FORM_ROUTE_ARGS[form]) == routes[rows], f"N={N} K={K} {form}: {rows} rows"

    def run(r0, r1):
        if form == "f16_silu_res":
            return K_.gemm(a[r0:r1], w, bias=b, act=K_.ACT_SILU, res=res[r0:r1])
        if form == "f16_gelu_res":
            return K_.gemm(a[r0:r1], w, bias=b, act=K_.ACT_GELU, scale=s, res=res[r0:r1])
        if form == "f32_scale_res":
            return K_.gemm(a[r0:r1], w, bias=b, scale=s, res=res[r0:r1], out_dtype=torch.float32)
        if form == "f32_res_rows":
            assert r0 % res_rows == 0
            return K_.gemm(a[r0:r1], w, bias=b, act=K_.ACT_RELU, scale=s, res=res, res_rows=res_rows, out_dtype=torch.float32)
        return K_.gemm(a[r0:r1], w, bias=b, a_rep=2, scale=s, res=res[r0:r1], out_dtype=torch.float32)

    whole = run(0, M)
    _assert_equal(_chunked(run, M, sizes), whole, f"N={N} K={K} {form} chunks {sizes}")
    # and in the other order of sizes: a chunk boundary inside another kernel's tile
    _assert_equal(_chunked(run, M, sizes[::-1]), whole, f"N={N} K={K} {form} chunks {sizes[::-1]}")


# (label, frames, frames per chunk, H, W, Cin (x3: 3 x logical), Cout, stride, form, {frames: route} for the whole and every chunk)
#   x3 Cin' = 192, Cout = 64 on 96 x 160: 5 frames are M = 76800 >= 65536, 4 frames and 1 stay on the register-staged kernel
#   Cout = 256 on 40 x 64: 24 frames have t256 = 240, 12 frames 120, 1 frame 10
#   16 x 16 output pixels, Cout = 128: 2 frames are M = 512, 1 frame M = 256
CONV_CASES = [
    ("x3 N=64 rule", 5, [4, 1], 96, 160, 192, 64, 1, "f32_scale", {5: DMA_C, 4: V1_N64, 1: V1_N64}),
    ("t256 rule", 24, [1] * 24, 40, 64, 96, 256, 1, "f32_scale", {24: DMA_Y, 1: DMA_C}),
    ("t256 rule f16", 24, [11, 1, 12], 40, 64, 96, 256, 1, "f16_silu_res", {24: DMA_Y, 12: DMA_C, 11: DMA_C, 1: DMA_C}),
    ("v1 / gemm2", 2, [1, 1], 16, 16, 64, 128, 1, "f16_silu_res", {2: DMA_C, 1: V1}),
    ("v1 / gemm2 stride 2", 2, [1, 1], 32, 32, 64, 128, 2, "f32_scale", {2: DMA_C, 1: V1}),
]
CONV_FORM_ROUTE_ARGS = {"f32_scale": dict(out_dtype=torch.float32, act=0, scale=True), "f16_silu_res": dict(out_dtype=torch.float16, res=True)}
# test_conv3x3_split_k_partials_are_independent_of_the_batch: (frames, H, W, Cin, Cout, split_k, {frames: route})
SPLIT_K_CASE = (24, 40, 64, 96, 256, 4, {24: DMA_Y, 1: DMA_C})


@pytest.mark.parametrize("label,n,sizes,H,W,cin,cout,stride,form,routes", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3x3_frames_are_independent_of_the_batch(cuda, label, n, sizes, H, W, cin, cout, stride, form, routes):
    from lmx import kernels as K_

    for frames in [n] + sizes:
        got = K_.conv3x3_route(frames, H, W, cin, cout, stride=stride, **CONV_FORM_ROUTE_ARGS[form])
        assert got == routes[frames], f"conv {label}: {frames} frames"

    g = torch.Generator(device=cuda).manual_seed(cin + cout + H)
    x = torch.randn((n, H, W, cin), device=cuda, generator=g).half()
    w = (torch.randn((cout, 9 * cin), device=cuda, generator=g) * (9 * cin) ** -0.5).half()
    b = torch.randn((cout,), device=cuda, generator=g)
    s = torch.rand((cout,), device=cuda, generator=g) + 0.5
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn((n, Ho, Wo, cout), device=cuda, generator=g).half()

    def run(f0, f1):
        if form == "f32_scale":
            return K_.conv3x3(x[f0:f1], w, b, act=K_.ACT_NONE, stride=stride, scale=s, out_dtype=torch.float32)
        return K_.conv3x3(x[f0:f1], w, b, act=K_.ACT_SILU, stride=stride, res=res[f0:f1])

    _assert_equal(_chunked(run, n, sizes), run(0, n), f"conv {label}")


def test_conv3x3_split_k_partials_are_independent_of_the_batch(cuda):
    """split_k partials (the exact plan's long-K convolutions) across the t256 crossing: 24 frames of 40 x 64 with Cout = 256 take
    the staggered 256x256x32 tiling, one frame 256x128x32; every partial of a frame is the same."""
    from lmx import kernels as K_

    g = torch.Generator(device=cuda).manual_seed(77)
    n, H, W, cin, cout, S, routes = SPLIT_K_CASE
    for frames in (n, 1):
        assert K_.conv3x3_route(frames, H, W, cin, cout, out_dtype=torch.float32, act=0, scale=True, split_k=S) == routes[frames]
    x = torch.randn((n, H, W, cin), device=cuda, generator=g).half()
    w = (torch.randn((cout, 9 * cin), device=cuda, generator=g) * (9 * cin) ** -0.5).half()
    b = torch.randn((cout,), device=cuda, generator=g)
    s = torch.rand((cout,), device=cuda, generator=g) + 0.5
    whole = K_.conv3x3(x, w, b, act=K_.ACT_NONE, scale=s, out_dtype=torch.float32, split_k=S)
    for f in (0, 13, 23):
        alone = K_.conv3x3(x[f:f + 1], w, b, act=K_.ACT_NONE, scale=s, out_dtype=torch.float32, split_k=S)
        _assert_equal(alone[:, 0], whole[:, f], f"split_k partials of frame {f}")


# ------------------------------------------------------------------------------------------------ model level
def test_yolo_exact_frame_alone_equals_frame_in_batch(cuda):
    """Exact YOLOv8-l on 1080p frames: model.2's 3 x 3 convolutions (96 x 160 per frame, N = 64) change kernel between 4 and 5
    frames (M >= 65536); a frame alone returns the bits it returns inside 5."""
    from lmx import synth, yolo

    cfg = yolo.YoloConfig("l")
    det = yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7, yolo.bn_stats_path("l")), cuda)
    assert det.precision == "exact"
    fr = torch.from_numpy(np.stack([synth.synth_frame(3, 40 + 7 * i) for i in range(5)], 0)).to(cuda)
    img, _ = det.preprocess(fr)
    print("yolov8l exact: letterboxed", tuple(img.shape))
    whole = det.forward_letterboxed(img)
    for j in (0, 4):
        _assert_equal(det.forward_letterboxed(img[j:j + 1]), whole[j:j + 1], f"yolov8l exact frame {j}")


@pytest.mark.parametrize("precision", ["exact", "f16"])
def test_sam_decoder_prompt_alone_equals_prompt_in_batch(cuda, precision):
    """MaskDecoder.predict: the 7-token Linears run on 7 n rows and change kernel between 73 and 74 prompts, the 4096-row image
    side changes tiling with n; prompt 0 and prompt 79 alone return the bits they return among 80."""
    from lmx import sam_decoder

    dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(41), cuda, precision=precision)
    n = 80
    g = torch.Generator(device=cuda).manual_seed(9)
    base = torch.nn.functional.interpolate(torch.randn((4, 256, 8, 8), device=cuda, generator=g), size=(64, 64), mode="bilinear")
    emb = base.permute(0, 2, 3, 1).reshape(4, 4096, 256)[torch.arange(n, device=cuda) % 4].reshape(n * 4096, 256).contiguous()
    emb = emb if precision == "exact" else emb.half()
    boxes = torch.rand((n, 4), device=cuda, generator=g) * torch.tensor([900.0, 500.0, 900.0, 500.0], device=cuda)
    boxes[:, 2:] += boxes[:, :2] + 50
    hw, rhw = (1080, 1920), (576, 1024)
    whole = {k: v.clone() for k, v in dec.predict(emb, boxes, hw, rhw).items()}
    for j in (0, n - 1):
        alone = dec.predict(emb[j * 4096:(j + 1) * 4096].contiguous(), boxes[j:j + 1].contiguous(), hw, rhw)
        for k in ("lowres", "iou", "mask", "stats"):
            _assert_equal(alone[k], whole[k][j:j + 1], f"{precision} decoder prompt {j}: {k}")


def test_dino_frame_alone_equals_frame_in_batch(cuda):
    """A small DINOv3 (201 tokens per frame): one frame runs every GEMM on 201 rows (register-staged kernel), three frames on
    603 (LDS-DMA kernel); the frame's hidden states and embedding are the same bits.  GEMM tilings only: 4 heads x 3 frames = 12
    attention items stay on attn_sp (the attn_spp switch at 64 items is test_dino_l_heads_frame_alone_equals_frame_in_batch)."""
    from lmx import dino, synth, weights

    cfg = dino.DinoConfig(hidden=256, layers=4, heads=4, mlp=1024, registers=4)
    assert cfg.tokens < 512 < 3 * cfg.tokens
    sd = weights.synth_state_dict(dino.param_spec(cfg), seed=21)
    m = dino.DinoEmbedder(cfg, sd, cuda)
    frames = torch.from_numpy(np.stack([synth.synth_frame(9, i) for i in (0, 40, 80)], 0)).to(cuda)
    patches = m.preprocess(frames)
    whole = m.hidden_states(patches, 3)
    np_ = cfg.grid * cfg.grid
    for j in (0, 2):
        alone = m.hidden_states(patches[j * np_:(j + 1) * np_].contiguous(), 1)
        _assert_equal(alone, whole[j * cfg.tokens:(j + 1) * cfg.tokens], f"dino frame {j} hidden states")
    _assert_equal(m.embed_frames(frames[2:3]), m.embed_frames(frames)[2:3], "dino embedding of frame 2")


# ------------------------------------------------------------------------------------------------ attention: attn_sp / attn_spp
# lmx_k_attention runs 128 < Tk <= 208 (64 < Tq <= 208, hd <= 64) on attn_sp below B * H = 64 items and on the persistent
# attn_spp from 64 (csrc/attn.hip lmx_k_attention; window geometry needs both pad vectors).  A frame's rows must be the same
# bits either way: the whole problem (>= 64 items, attn_spp) against batch chunks of < 64 items each (attn_sp).
# (label, items per batch element (H, or H x windows per image), B, chunk sizes in batch elements, hd, window,
#  (route of the whole, route of every chunk): lmx_h_attn_route's names)
ATTN_CASES = [
    ("flat T201 hd56 H16", 16, 8, [3, 1, 2, 2], 56, None, ("spp_ones", "sp_qb2_ones")),
    ("flat T201 hd64 H16", 16, 8, [3, 1, 2, 2], 64, None, ("spp_dot2", "sp_qb2_dot2")),
    ("win14 28x28 pad vectors hd56 H2", 2, 8 * 4, [3, 1, 4], 56, dict(Gh=28, Gw=28, ws=14, q_stride=1), ("spp_ones", "sp_qb2_ones")),
    ("win14 20x20 pad vectors hd64 H2", 2, 8 * 4, [7, 1], 64, dict(Gh=20, Gw=20, ws=14, q_stride=1), ("spp_dot2", "sp_qb2_dot2")),
    # more items than CUs (B and the chunk sizes are functions of the CU count): every workgroup of the persistent kernel walks three
    # or four items and hands its LDS image over between them — the geometries of the two many-items rows of tests/test_gpu_attention.py
    ("flat T201 hd64 H2 items 3CU+6", 2, lambda cu: -(-(3 * cu + 6) // 2), lambda cu: _cut(-(-(3 * cu + 6) // 2), (31, 17, 25, 9)), 64, None,
     ("spp_dot2", "sp_qb2_dot2")),
    ("win14 20x20 pad vectors hd56 H2 items 3CU+8", 2, lambda cu: 4 * -(-(3 * cu + 8) // 8), lambda cu: _cut(-(-(3 * cu + 8) // 8), (7, 3, 5, 1)), 56,
     dict(Gh=20, Gw=20, ws=14, q_stride=1), ("spp_ones", "sp_qb2_ones")),
]


def _cut(n, pattern):
    """n batch elements in chunks whose sizes cycle through `pattern`."""
    out = []
    while sum(out) < n:
        out.append(min(pattern[len(out) % len(pattern)], n - sum(out)))
    return out


def attn_case_batches(B, sizes, window, cu=None):
    """B of the whole problem, then of every chunk of a case of ATTN_CASES, as lmx_k_attention counts it (windows: 4 per image);
    cu: the CU count, for the cases whose B and sizes are functions of it."""
    B, sizes = (B(cu), sizes(cu)) if callable(B) else (B, sizes)
    return [B] + [s * (1 if window is None else 4) for s in sizes]


@pytest.mark.parametrize("label,H,B,sizes,hd,window,routes", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_rows_are_independent_of_the_batch(cuda, label, H, B, sizes, hd, window, routes):
    """sizes in batch elements (frames | windows); for windows a chunk is whole images (4 windows of 14 x 14 each)."""
    from lmx import kernels as K_

    if callable(B):
        cu = torch.cuda.get_device_properties(cuda).multi_processor_count
        B, sizes = B(cu), sizes(cu)
        assert B * H > 3 * cu, "every workgroup must walk at least three items"
    T = 201 if window is None else 196
    g = torch.Generator(device=cuda).manual_seed(hd + B)
    heads, per = H, (1 if window is None else 4)
    rows_per = T if window is None else window["Gh"] * window["Gw"]
    n_elem = B // per  # batch elements in token rows: frames, or images for windows
    D = heads * hd
    qkv = (torch.randn((n_elem * rows_per, 3 * D), device=cuda, generator=g) * 1.5).half()
    pad = torch.randn((3 * D,), device=cuda, generator=g).half()
    assert B * heads >= 64 and all(s * per * heads < 64 for s in sizes)
    for i, b in enumerate(attn_case_batches(B, sizes, window)):
        got = K_.attention_route(b, heads, T, T, hd, window=window, pad=window is not None, ld=3 * D)
        assert got == routes[min(i, 1)], f"attention {label}: B = {b}"

    def run(e0, e1):
        x = qkv[e0 * rows_per:e1 * rows_per]
        out = torch.empty((x.shape[0], D), dtype=torch.float16, device=cuda)
        K_.attention(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], out, (e1 - e0) * per, heads, T, T, hd, hd ** -0.5, window=window,
                     pad_k=pad[D:2 * D] if window else None, pad_v=pad[2 * D:] if window else None)
        return out

    whole = run(0, n_elem)
    _assert_equal(_chunked(run, n_elem, sizes), whole, f"attention {label} chunks {sizes}")


def test_dino_l_heads_frame_alone_equals_frame_in_batch(cuda):
    """DINOv3-L attention geometry (16 heads of 64, 201 tokens) on 2 layers: frame 0 alone is 16 attention items (attn_sp), the
    same frame among 4 is 64 (attn_spp); hidden states and embedding must be the same bits."""
    from lmx import dino, synth, weights

    cfg = dino.DinoConfig(hidden=1024, layers=2, heads=16, mlp=4096, registers=4)
    assert cfg.head_dim == 64 and cfg.tokens == 201 and cfg.heads < 64 <= 4 * cfg.heads
    sd = weights.synth_state_dict(dino.param_spec(cfg), seed=23)
    m = dino.DinoEmbedder(cfg, sd, cuda)
    frames = torch.from_numpy(np.stack([synth.synth_frame(5, i) for i in (0, 30, 60, 90)], 0)).to(cuda)
    patches = m.preprocess(frames)
    whole = m.hidden_states(patches, 4)
    np_ = cfg.grid * cfg.grid
    alone = m.hidden_states(patches[:np_].contiguous(), 1)
    _assert_equal(alone, whole[:cfg.tokens], "dino-L heads: frame 0 hidden states")
    _assert_equal(m.embed_frames(frames[:1]), m.embed_frames(frames)[:1], "dino-L heads: embedding of frame 0")
