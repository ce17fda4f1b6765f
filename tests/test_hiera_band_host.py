"""The band rule of the Hiera encoder (lmx_h_hiera_band) and the premise it rests on, without a GPU.

A frame resized to nh x nw sits at the top-left of the zero canvas.  Until the first global-attention block, tokens mix only inside
windows and 2 x 2 pools, so the token rows below a band never see a pixel and hold the same values for every frame.  The rule is
checked against a brute-force propagation of a boolean "touched a pixel" grid through the block plan; the premise on the fp32 oracle."""
import math

import numpy as np
import pytest
import torch

from lmx import kernels as K
from lmx import sam, weights


def _tiny(image=256):  # the configuration of tests/test_gpu_sam.py
    return sam.HieraConfig(hidden=16, blocks=(1, 2, 3, 2), dims=(16, 32, 64, 128), heads=(1, 2, 4, 8), windows=(8, 4, 14, 7),
                           global_blocks=(4,), pos_bkg=(7, 7), fpn_dim=32, image=image)


def _rule(cfg, nh, nw):
    plan = cfg.block_plan()
    return K.hiera_band([p[3] for p in plan], [p[4] for p in plan], cfg.image // 4, nh, nw)


def _touched0(g, nh, nw):
    """[g, g] bool: the 7 x 7 / stride 4 / pad 3 patch of token (r, c) holds a pixel of the nh x nw frame."""
    rows = np.array([any(0 <= y < nh for y in range(4 * r - 3, 4 * r + 4)) for r in range(g)])
    cols = np.array([any(0 <= x < nw for x in range(4 * c - 3, 4 * c + 4)) for c in range(g)])
    return rows[:, None] & cols[None, :]


def _close_windows(t, win):
    """A token of a window that holds a touched token is touched (attention inside the window; the grid is padded to whole windows)."""
    H, W = t.shape
    Hp, Wp = -(-H // win) * win, -(-W // win) * win
    p = np.zeros((Hp, Wp), bool)
    p[:H, :W] = t
    w = p.reshape(Hp // win, win, Wp // win, win)
    w = np.broadcast_to(w.any(axis=(1, 3), keepdims=True), w.shape)
    return w.reshape(Hp, Wp)[:H, :W].copy()


def _brute_force(cfg, nh, nw):
    """Stage-1 token rows that a pixel reaches in front of the first global block (0 if block 0 is global), the rows of the smallest
    piece that is whole windows and whole pooled pairs at every one of those blocks, and the index of the first global block."""
    t = _touched0(cfg.image // 4, nh, nw)
    scale, unit, reach = 1, 1, 0
    for i, (_, _, _, win, qs) in enumerate(cfg.block_plan()):
        if win == 0:
            return reach, unit, i
        t = _close_windows(t, win)
        unit = math.lcm(unit, win * scale)
        if qs:
            H, W = t.shape
            t = t.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))
            unit = math.lcm(unit, 2 * scale)
            scale *= 2
        rows = np.flatnonzero(t.any(axis=1))
        reach = max(reach, (int(rows[-1]) + 1) * scale if rows.size else 0)
    return reach, unit, None


@pytest.mark.parametrize("cfg", [sam.hiera_b_plus(), _tiny(256), _tiny(320)], ids=["hiera_b_plus", "tiny256", "tiny320"])
def test_band_rule_against_brute_force(cfg):
    g, S = cfg.image // 4, cfg.image
    first_off = None
    for nh in range(1, S + 1):
        band = _rule(cfg, nh, S)
        reach, unit, first_global = _brute_force(cfg, nh, S)
        assert first_global and first_global > 0
        d1 = (nh + 2) // 4 + 1
        assert min(d1, g) == int(_touched0(g, nh, S).any(axis=1).sum())  # the formula for the rows whose patch touches a pixel
        want = -(-d1 // unit) * unit  # the smallest whole number of pieces that covers them
        assert want >= reach  # ... and nothing a pixel reaches lies below it
        if want < g:
            assert band == want, (nh, band, want)
        else:
            assert band == 0, (nh, band)
            first_off = first_off or nh
    # the first height without a band: the first whose pieces fill the grid
    assert first_off is not None and _rule(cfg, first_off - 1, S) > 0 and _rule(cfg, first_off, S) == 0


def test_band_rule_edges_of_hiera_b_plus():
    cfg = sam.hiera_b_plus()
    assert _brute_force(cfg, 576, 1024)[1:] == (56, 12)  # pieces of 56 stage-1 rows (the 14 x 14 windows of stage 3), block 12 is global
    assert _rule(cfg, 221, 1024) == 56 and _rule(cfg, 222, 1024) == 112
    assert _rule(cfg, 576, 1024) == 168  # 1080 x 1920: 42 of the 64 stage-3 rows
    assert _rule(cfg, 893, 1024) == 224 and _rule(cfg, 894, 1024) == 0  # 225 rows touch a pixel: the next piece ends past the grid
    assert _rule(cfg, 1024, 1024) == 0
    assert _rule(cfg, 1024, 576) == 0 and _rule(cfg, 576, 1023) == 0  # portrait, or any padding on the right: no band
    nh, nw = sam.resize_longest_side(1920, 1080)
    assert _rule(cfg, nh, nw) == 0


def test_band_rule_without_a_place_to_end():
    first = sam.HieraConfig(global_blocks=(0, 12))  # block 0 is global
    none = sam.HieraConfig(global_blocks=())  # no block is
    assert _rule(first, 576, 1024) == 0 and _rule(none, 576, 1024) == 0
    with pytest.raises(K.LmxError):
        K.hiera_band([8, 0], [0, 0], 256, 0, 1024)
    with pytest.raises(K.LmxError):
        K.hiera_band([8, 0], [0, 0], 256, 1025, 1024)


def test_rows_below_the_band_do_not_depend_on_the_frame():
    """The premise, on the fp32 oracle with the tiny configuration: after every block in front of the first global one the rows below
    the band are equal for two random frames (and the rows of the band are not); after the global block every row differs."""
    from oracle import hiera as OH

    cfg = _tiny(256)
    sd = weights.synth_state_dict(sam.param_spec(cfg), seed=31)
    nh, nw = sam.resize_longest_side(1080, 1920, cfg.image)
    band = _rule(cfg, nh, nw)
    assert (nh, nw, band) == (144, 256, 40)
    rng = np.random.default_rng(7)
    per_block = []
    for _ in range(2):  # one call per frame: the same shapes, so equal inputs give equal bits
        u8 = rng.integers(0, 256, (nh, nw, 3), dtype=np.uint8)
        pv = np.zeros((cfg.image, cfg.image, 3), np.float32)
        pv[:nh, :nw] = (u8.astype(np.float32) - np.array(sam.SAM_PIXEL_MEAN, np.float32)) / np.array(sam.SAM_PIXEL_STD, np.float32)
        with torch.no_grad():
            per_block.append(OH.trunk_forward(cfg, sd, torch.from_numpy(pv.transpose(2, 0, 1)[None].copy()), return_blocks=True)[1])
    g = cfg.image // 4
    first_global = cfg.global_blocks[0]
    for i, (a, b) in enumerate(zip(*per_block)):
        bs = band * a.shape[1] // g
        if i < first_global:
            assert torch.equal(a[:, bs:], b[:, bs:]), f"block {i}: rows below the band differ between the frames"
            assert not torch.equal(a[:, :bs], b[:, :bs])
        elif i == first_global:
            differs = (a != b).any(dim=3)[0]  # [H, W]
            assert bool(differs.any(dim=1).all()), f"block {i}: a row is still equal after global attention"
