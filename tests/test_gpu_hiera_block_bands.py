"""The Hiera encoder on a band of token rows sized block by block (HieraEncoder(band="blocks"), lmx_h_hiera_bands) against the same
encoder on the whole grid (band=False): bit for bit, on every stage output and every FPN level.  Nothing here has a tolerance: the
rows a join adds are constants of the weights, and every kernel in front of the first global block computes a row from its own
window whatever the grid's height — a difference is a shape dependence of one of those kernels, or a join at the wrong rows."""
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


def _assert_embedding(got, ref, what):
    assert got["fpn"][0] is None and got["fpn"][1] is None and got["stages"][0] is None and got["stages"][1] is None
    assert torch.equal(got["fpn"][2], ref["fpn"][2]) and torch.equal(got["resized"], ref["resized"]), what
    assert torch.equal(got["stages"][2], ref["stages"][2]) and torch.equal(got["stages"][3], ref["stages"][3]), what


def _pair(cuda, image):
    from lmx import sam, weights

    cfg = sam.HieraConfig(image=image)
    sd = weights.synth_state_dict(sam.param_spec(cfg), 5)
    return dict(cfg=cfg, sd=sd, on=sam.HieraEncoder(cfg, sd, cuda, band="blocks"), off=sam.HieraEncoder(cfg, sd, cuda, band=False))


@pytest.fixture(scope="module")
def small(cuda):
    """Hiera-B+ widths on canvases of 256 and 320 pixels (grids of 64 and 80 rows: every fused kernel's divisibility holds)."""
    return {256: _pair(cuda, 256), 320: _pair(cuda, 320)}


@pytest.fixture(scope="module")
def bplus(cuda):
    return _pair(cuda, 1024)


def _joins(enc, nh, nw, n):
    rows = enc.block_rows(nh, nw, n)
    return (rows[0], rows[3], rows[6]), [(i, p.join, p.H) for i, p in enumerate(enc.plan(n, rows)) if p.join]


# (canvas, frame h, w, frames, rows of blocks 0 - 2 / 3 - 5 / 6 - 11, joins): the smallest shape with both joins, one and two frames; a
# band that ends in front of block 6 (the join there reaches the whole grid, none at the global block); the smallest band with a
# partial join
SMALL = [(256, 1080, 1920, 1, (40, 20, 14), [(6, 10, 14), (12, 14, 16)]), (256, 1080, 1920, 2, (40, 20, 14), [(6, 10, 14), (12, 14, 16)]),
         (320, 460, 640, 2, (64, 32, 20), [(6, 16, 20)]), (256, 200, 512, 2, (32, 16, 14), [(6, 8, 14), (12, 14, 16)])]


@pytest.mark.parametrize("image,h,w,n,rows,joins", SMALL, ids=[f"{c[0]}-{c[1]}x{c[2]}-n{c[3]}" for c in SMALL])
def test_small_canvas_bands_equal_whole_grid(cuda, small, image, h, w, n, rows, joins):
    from lmx import sam

    on, off = small[image]["on"], small[image]["off"]
    nh, nw = sam.resize_longest_side(h, w, image)
    assert (nh, nw) == {(256, 1080): (144, 256), (320, 460): (230, 320), (256, 200): (100, 256)}[(image, h)]
    assert _joins(on, nh, nw, n) == (rows, joins)
    frames = _frames(cuda, n, h, w, seed=h + n)
    ref = off.encode(frames)
    _assert_same(on.encode(frames), ref, f"{image}: {h}x{w}")
    _assert_embedding(on.encode(frames, outputs="embedding"), ref, f"{image}: {h}x{w} embedding")


# (frame h, w, rows, joins) on the 1024 canvas, one frame each: 16:9; a frame that had no band under the one-number rule; portrait
REAL = [(1080, 1920, (152, 76, 42), [(6, 38, 42), (12, 42, 64)]), (894, 1024, (232, 116, 64), [(6, 58, 64)]), (1920, 1080, (256, 128, 64), [])]


@pytest.mark.parametrize("h,w,rows,joins", REAL, ids=[f"{h}x{w}" for h, w, _, _ in REAL])
def test_hiera_b_plus_bands_equal_whole_grid(cuda, bplus, h, w, rows, joins):
    from lmx import sam

    on, off = bplus["on"], bplus["off"]
    nh, nw = sam.resize_longest_side(h, w, 1024)
    assert _joins(on, nh, nw, 1) == (rows, joins)
    frames = _frames(cuda, 1, h, w, seed=h)
    ref = off.encode(frames)
    _assert_same(on.encode(frames), ref, f"{h}x{w}")
    _assert_embedding(on.encode(frames, outputs="embedding"), ref, f"{h}x{w} embedding")


def test_launches_of_a_1080p_frame(cuda, bplus):
    """The mode is on: the first fused attention half runs on n * 152 * 256 rows, and one encode(outputs="embedding") joins the f32
    stream exactly twice — 38 -> 42 stage-3 rows in front of block 6, 42 -> 64 in front of block 12 — and nothing else."""
    from lmx import kernels as K

    n = 2
    frames = _frames(cuda, n, 1080, 1920, seed=21)
    bplus["on"].encode(frames, outputs="embedding")  # builds the table of constant rows, outside the trace
    K.start_launch_trace()
    try:
        bplus["on"].encode(frames, outputs="embedding")
        keys = [key for _, key, *_ in K.LAUNCH_TRACE]
    finally:
        K.stop_launch_trace()
    attn8 = [k for k in keys if k.startswith("hiera_attn8 ")]
    assert attn8[0] == f"hiera_attn8 rows={n * 152 * 256} D=112 ln_inside=1" and len(attn8) == 2
    assert [k for k in keys if k.startswith("band_join")] == [f"band_join n={n} H=42 Hb=38 W=64 D=448 dtype={K.F32}",
                                                              f"band_join n={n} H=64 Hb=42 W=64 D=448 dtype={K.F32}"]


def test_table_bookkeeping(cuda, small, monkeypatch):
    """One table per frame geometry, built by the first call; under a stream capture a missing table is an error."""
    from lmx import kernels as K
    from lmx import sam

    s = small[256]
    enc = sam.HieraEncoder(s["cfg"], s["sd"], cuda, band="blocks")
    wide, flat = _frames(cuda, 1, 1080, 1920, seed=31), _frames(cuda, 1, 200, 512, seed=32)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(K.LmxError, match="capture"):
            enc.encode(wide)
        assert not enc._band_tabs
    _assert_same(enc.encode(wide), s["off"].encode(wide), "first geometry")
    assert len(enc._band_tabs) == 1
    tab = next(iter(enc._band_tabs.values()))
    assert sorted(tab["x"]) == [6, 12] and [tuple(t.shape) for t in tab["x"].values()] == [(4 * 16, 448), (2 * 16, 448)]
    assert [tuple(t.shape) for t in tab["stages"]] == [(24 * 64, 112), (12 * 32, 224)] and [t.dtype for t in tab["stages16"]] == [torch.float16] * 2
    enc.encode(wide, outputs="embedding")
    enc.encode(_frames(cuda, 2, 1080, 1920, seed=33))
    assert len(enc._band_tabs) == 1  # a repeated geometry adds none, whatever the batch and the outputs
    _assert_same(enc.encode(flat), s["off"].encode(flat), "second geometry")
    assert len(enc._band_tabs) == 2
    with monkeypatch.context() as m:  # with the tables in place the same calls go through
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        enc.encode(wide)
        enc.encode(flat)
        with pytest.raises(K.LmxError, match="capture"):
            enc.encode(_frames(cuda, 1, 400, 512, seed=34))  # a third geometry

