"""The Hiera encoder on the band of token rows that depends on the frame (HieraEncoder(band=True), the default) against the same
encoder on the whole grid (band=False): bit for bit, on every stage output and every FPN level.  Nothing here has a tolerance: the
rows below the band are constants of the weights, and every kernel in front of the first global block computes a row from its own
window whatever the grid's height — a difference is a shape dependence of one of those kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _frames(cuda, n, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(cuda)


def _assert_same(got, ref, what):
    assert torch.equal(got["resized"], ref["resized"]), f"{what}: resized"
    for name in ("fpn", "stages"):
        assert len(got[name]) == len(ref[name])
        for lvl, (a, b) in enumerate(zip(got[name], ref[name])):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}: {name}[{lvl}] differs"


def _tiny(image):
    from lmx import sam

    return sam.HieraConfig(hidden=16, blocks=(1, 2, 3, 2), dims=(16, 32, 64, 128), heads=(1, 2, 4, 8), windows=(8, 4, 14, 7),
                           global_blocks=(4,), pos_bkg=(7, 7), fpn_dim=32, image=image)


@pytest.fixture(scope="module")
def bplus(cuda):
    """Hiera-B+ with one set of weights: the banded encoder, the whole-grid one, and what it takes to build a fresh one."""
    from lmx import sam, weights

    cfg = sam.hiera_b_plus()
    sd = weights.synth_state_dict(sam.param_spec(cfg), 5)
    return dict(cfg=cfg, sd=sd, on=sam.HieraEncoder(cfg, sd, cuda), off=sam.HieraEncoder(cfg, sd, cuda, band=False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [112, 8])
def test_band_join_against_indexing(cuda, dtype, D):
    from lmx import kernels as K

    n, H, Hb, W = 3, 5, 2, 3
    g = torch.Generator().manual_seed(D)
    band = torch.randn((n, Hb, W, D), generator=g).to(dtype).to(cuda)
    table = torch.randn(((H - Hb) * W, D), generator=g).to(dtype).to(cuda)
    want = torch.empty((n, H, W, D), dtype=dtype, device=cuda)
    want[:, :Hb] = band
    want[:, Hb:] = table.view(H - Hb, W, D)
    got = K.band_join(band, table, H)
    assert got.dtype == dtype and torch.equal(got, want)


def test_band_join_argument_errors(cuda):
    from lmx import kernels as K

    def join(n, H, Hb, W, D, dtype):
        return K.band_join(torch.zeros((n, Hb, W, D), dtype=dtype, device=cuda), torch.zeros((max(H - Hb, 0) * W, D), dtype=dtype, device=cuda), H)

    join(1, 5, 4, 3, 4, torch.float32)  # 16-byte rows, Hb = H - 1: the last shapes that pass
    join(1, 2, 1, 3, 8, torch.float16)
    for bad in ((1, 5, 2, 3, 4, torch.float16),   # rows of 8 bytes
                (1, 5, 2, 3, 6, torch.float32),   # rows of 24 bytes
                (1, 5, 2, 3, 12, torch.float16),  # rows of 24 bytes
                (1, 5, 5, 3, 8, torch.float32),   # Hb = H
                (1, 5, 0, 3, 8, torch.float32)):  # Hb = 0
        with pytest.raises(K.LmxError):
            join(*bad)
    # the library's own checks, behind the wrapper's
    lib, ptr = K._lib.load(), 4096
    for args in ((ptr, ptr, ptr, K.F32, 1, 5, 0, 3, 8), (ptr, ptr, ptr, K.F32, 1, 5, 5, 3, 8), (ptr, ptr, ptr, K.F32, 1, 5, 6, 3, 8),
                 (ptr, ptr, ptr, K.F16, 1, 5, 2, 3, 4), (ptr, ptr, ptr, K.F32, 1, 5, 2, 3, 6), (ptr, ptr + 8, ptr, K.F32, 1, 5, 2, 3, 8)):
        assert lib.lmx_k_band_join(*args, None) != 0, args


# (frame h, w, frames, the band the rule must return): 16:9; the last height of one 56-row piece and the first of two; 224 of 256
# rows; the first height whose pieces fill the grid (no band); portrait (no band)
CASES = [(1080, 1920, 2, 168), (221, 1024, 1, 56), (222, 1024, 1, 112), (800, 1024, 1, 224), (894, 1024, 1, 0), (1920, 1080, 1, 0)]


@pytest.mark.parametrize("h,w,n,band", CASES, ids=[f"{h}x{w}" for h, w, _, _ in CASES])
def test_hiera_b_plus_band_equals_whole_grid(cuda, bplus, h, w, n, band):
    from lmx import sam

    nh, nw = sam.resize_longest_side(h, w, bplus["cfg"].image)
    assert bplus["on"].band_rows(nh, nw) == band
    frames = _frames(cuda, n, h, w, seed=h)
    _assert_same(bplus["on"].encode(frames), bplus["off"].encode(frames), f"{h}x{w}")


@pytest.mark.parametrize("image,band", [(256, 40), (320, 48)])
def test_hiera_tiny_band_equals_whole_grid(cuda, image, band):
    """Grids of 64 / 80 rows with separate launches in every block (no fused kernel is built for these widths), windows of 14 on a
    padded grid in the block after the band."""
    from lmx import sam, weights

    cfg = _tiny(image)
    sd = weights.synth_state_dict(sam.param_spec(cfg), 31)
    on, off = sam.HieraEncoder(cfg, sd, cuda), sam.HieraEncoder(cfg, sd, cuda, band=False)
    assert on.band_rows(*sam.resize_longest_side(1080, 1920, image)) == band
    frames = _frames(cuda, 2, 1080, 1920, seed=image)
    _assert_same(on.encode(frames), off.encode(frames), f"tiny {image}")


def test_embedding_outputs(cuda, bplus):
    frames = _frames(cuda, 2, 1080, 1920, seed=11)
    ref = bplus["off"].encode(frames)
    for enc in (bplus["on"], bplus["off"]):
        got = enc.encode(frames, outputs="embedding")
        assert got["fpn"][0] is None and got["fpn"][1] is None and got["stages"][0] is None and got["stages"][1] is None
        assert torch.equal(got["fpn"][2], ref["fpn"][2]) and torch.equal(got["resized"], ref["resized"])
        assert torch.equal(got["stages"][2], ref["stages"][2]) and torch.equal(got["stages"][3], ref["stages"][3])
    with pytest.raises(ValueError):
        bplus["on"].encode(frames, outputs="fpn")


def test_table_follows_the_kernel_selection(cuda, bplus, monkeypatch):
    """The constant rows come from the kernels that were selected when they were built.  With the fused attention halves switched off
    after a first call, the same encoder must build them again from the separate launches, not reuse the fused kernels' rows."""
    frames = _frames(cuda, 1, 1080, 1920, seed=12)
    on, off = bplus["on"], bplus["off"]
    _assert_same(on.encode(frames), off.encode(frames), "fused")
    tables = len(on._band_tabs)
    for v in ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL"):
        monkeypatch.setenv(v, "0")
    plain = off.encode(frames)
    _assert_same(on.encode(frames), plain, "separate launches")
    assert len(on._band_tabs) == tables + 1
    monkeypatch.setenv("LMX_MLP_IMG", "0")
    _assert_same(on.encode(frames), off.encode(frames), "separate launches, csrc/mlp.hip's fused MLP")
    assert len(on._band_tabs) == tables + 2


def test_first_calls_on_two_streams(cuda, bplus):
    """A fresh encoder builds its table in the first call and synchronises the building stream; the second call, issued at once on
    another stream, reads the table without an event."""
    from lmx import sam

    frames = _frames(cuda, 2, 1080, 1920, seed=13)
    ref = bplus["off"].encode(frames)
    torch.cuda.synchronize()
    enc = sam.HieraEncoder(bplus["cfg"], bplus["sd"], cuda)
    s1, s2 = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    with torch.cuda.stream(s1):
        a = enc.encode(frames[:1])
    with torch.cuda.stream(s2):
        b = enc.encode(frames[1:])
    torch.cuda.synchronize()
    for name in ("fpn", "stages"):
        for lvl, r in enumerate(ref[name]):
            assert torch.equal(a[name][lvl][0], r[0]) and torch.equal(b[name][lvl][0], r[1]), f"{name}[{lvl}]"


def test_table_is_not_built_under_capture(cuda, bplus, monkeypatch):
    """Building the table ends in a synchronisation, which a stream capture must never meet: a capture that finds no table is an
    error (lmx.graphs.GraphedFn runs its warm-up calls first, and those build it)."""
    from lmx import kernels as K
    from lmx import sam

    enc = sam.HieraEncoder(bplus["cfg"], bplus["sd"], cuda)
    frames = _frames(cuda, 1, 1080, 1920, seed=14)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(K.LmxError, match="capture"):
            enc.encode(frames)
        assert not enc._band_tabs
    _assert_same(enc.encode(frames), bplus["off"].encode(frames), "after the refused capture")
    with monkeypatch.context() as m:  # with the table in place the same call goes through
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        enc.encode(frames)


def test_fused_step_with_and_without_band(cuda, bplus):
    """FusedExtractor.step on 3 frames: every returned field is the same with the SAM encoder's band on and off."""
    from lmx import dino, pipeline, sam_decoder, synth, weights, yolo

    ycfg = yolo.YoloConfig("n")
    dcfg = dino.DinoConfig(hidden=256, layers=2, heads=4, mlp=1024, registers=4)
    fx = pipeline.FusedExtractor.from_models(yolo.YoloDetector(ycfg, yolo.synthetic_state_dict(ycfg, 7, yolo.bn_stats_path("n")), cuda), bplus["off"],
                                             sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(105), cuda),
                                             dino.DinoEmbedder(dcfg, weights.synth_state_dict(dino.param_spec(dcfg), 3), cuda))
    frames = torch.from_numpy(np.stack([synth.synth_frame(3, 40 + i) for i in range(3)], 0)).to(cuda)
    out = {}
    for mode in ("off", "on"):
        fx.sam = bplus[mode]
        out[mode] = {k: v.clone() for k, v in fx.step(frames, sam_chunk=2, keep_byte_masks=True).items()}
        torch.cuda.synchronize()
    assert out["on"].keys() == out["off"].keys()
    for k, v in out["off"].items():
        assert torch.equal(out["on"][k], v), k
    assert {"mask", "mask_bits", "mask_stats", "mask_contour", "mask_iou"} <= out["off"].keys()
