"""The band of the Hiera encoder sized block by block (lmx_h_hiera_bands, HieraEncoder(band="blocks")) without a GPU: the rule against
a brute-force propagation of a boolean "touched a pixel" grid through the block plan, its pinned values for Hiera-B+, and the plan
that lmx.sam.hiera_plan makes of the rows per block — where its joins sit and that it runs the whole grid's kernels."""
import math

import numpy as np
import pytest

from lmx import kernels as K
from lmx import sam

SWITCHES = ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL", "LMX_HIERA_ATTN_POOL3", "LMX_MLP_IMG", "LMX_NO_FUSED_MLP")


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _tiny(image=256):  # the configuration of tests/test_gpu_sam.py
    return sam.HieraConfig(hidden=16, blocks=(1, 2, 3, 2), dims=(16, 32, 64, 128), heads=(1, 2, 4, 8), windows=(8, 4, 14, 7),
                           global_blocks=(4,), pos_bkg=(7, 7), fpn_dim=32, image=image)


def _rule(cfg, nh, nw):
    plan = cfg.block_plan()
    return K.hiera_bands([p[3] for p in plan], [p[4] for p in plan], cfg.image // 4, nh, nw)


def _whole(cfg):
    """The whole grid's rows at the resolution each block reads."""
    rows, g = [], cfg.image // 4
    for _, _, _, _, qs in cfg.block_plan():
        rows.append(g)
        g = g // 2 if qs else g
    return tuple(rows)


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


def _reach_per_block(cfg, nh, nw):
    """[(rows a pixel reaches going INTO block i, rows of the grid block i reads)] for the blocks in front of the first global one,
    and that block's index."""
    t = _touched0(cfg.image // 4, nh, nw)
    out = []
    for i, (_, _, _, win, qs) in enumerate(cfg.block_plan()):
        if win == 0:
            return out, i
        rows = np.flatnonzero(t.any(axis=1))
        out.append((int(rows[-1]) + 1 if rows.size else 0, t.shape[0]))
        t = _close_windows(t, win)
        if qs:
            H, W = t.shape
            t = t.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))
    return out, None


@pytest.mark.parametrize("cfg", [sam.hiera_b_plus(), _tiny(256), _tiny(320)], ids=["hiera_b_plus", "tiny256", "tiny320"])
def test_rule_against_brute_force(cfg):
    S, blocks, whole = cfg.image, cfg.block_plan(), _whole(cfg)
    seen = set()
    for nh in range(1, S + 1):
        rows = _rule(cfg, nh, S)
        seen.add(rows)
        reach, first_global = _reach_per_block(cfg, nh, S)
        assert first_global and first_global > 0 and len(rows) == len(blocks)
        for i, (r, g) in enumerate(reach):
            win, qs = blocks[i][3], blocks[i][4]
            assert g == whole[i]
            assert r <= rows[i] <= g, (nh, i)  # everything a pixel reaches going into the block, never more than the grid
            piece = math.lcm(win, 2 if qs else 1)
            assert rows[i] == min(-(-r // piece) * piece, g), (nh, i, rows[i], r)  # the smallest count of whole windows and pairs
        assert rows[first_global:] == whole[first_global:]
    assert _rule(cfg, S, S) == whole and len(seen) > 2


def test_rule_is_monotonic_for_every_height():
    """Every nh from 1 to the canvas: a block never has fewer rows than the block before it left, whole windows everywhere."""
    for cfg in (sam.hiera_b_plus(), _tiny(256), _tiny(320)):
        blocks, whole, last = cfg.block_plan(), _whole(cfg), None
        first_global = next(i for i, b in enumerate(blocks) if b[3] == 0)
        for nh in range(1, cfg.image + 1):
            rows = _rule(cfg, nh, cfg.image)
            assert rows[0] >= min((nh + 2) // 4 + 1, whole[0])
            left = rows[0]
            for i in range(first_global):
                assert left <= rows[i] <= whole[i] and (rows[i] % blocks[i][3] == 0 or rows[i] == whole[i]), (nh, i)
                assert not blocks[i][4] or rows[i] % 2 == 0
                left = rows[i] // 2 if blocks[i][4] else rows[i]
            assert last is None or all(a <= b for a, b in zip(last, rows))  # a taller frame never needs fewer rows
            last = rows


def _stages(rows):
    assert len(set(rows[0:3])) == len(set(rows[3:6])) == len(set(rows[6:12])) == 1
    return rows[0], rows[3], rows[6]


def test_pinned_values_of_hiera_b_plus():
    cfg = sam.hiera_b_plus()
    whole = _whole(cfg)
    assert whole == (256,) * 3 + (128,) * 3 + (64,) * 16 + (32,) * 2
    for nh, want in ((576, (152, 76, 42)), (221, (56, 28, 14)), (222, (64, 32, 28)), (800, (208, 104, 56)), (894, (232, 116, 64))):
        rows = _rule(cfg, nh, 1024)
        assert _stages(rows) == want and rows[12:] == whole[12:], nh
    assert _rule(cfg, 1024, 1024) == whole
    assert _rule(cfg, 1024, 576) == whole and _rule(cfg, 576, 1023) == whole  # portrait, or any padding on the right
    assert _rule(cfg, *sam.resize_longest_side(1920, 1080)) == whole
    assert _stages(_rule(cfg, *sam.resize_longest_side(1080, 1920))) == (152, 76, 42)
    # the one-number rule stays what it is
    plan = cfg.block_plan()
    assert K.hiera_band([p[3] for p in plan], [p[4] for p in plan], 256, 576, 1024) == 168


def test_rule_without_a_place_to_end_and_argument_errors():
    first = sam.HieraConfig(global_blocks=(0, 12))  # block 0 is global
    none = sam.HieraConfig(global_blocks=())  # no block is
    assert _rule(first, 576, 1024) == _whole(first) and _rule(none, 576, 1024) == _whole(none)
    assert K.hiera_bands([8, 8, 0], [0, 2, 0], 256, 576, 1024) == (152, 152, 128)
    assert K.hiera_bands([7, 0], [2, 0], 256, 576, 1024) == (154, 128)  # an odd window that pools: whole windows, an even count
    for bad in (([8, 0], [0, 0], 256, 0, 1024), ([8, 0], [0, 0], 256, 1025, 1024), ([8, 0], [0, 0], 0, 576, 1024),
                ([8, 0], [0, 3], 256, 576, 1024), ([-1, 0], [0, 0], 256, 576, 1024), ([8, 0], [0], 256, 576, 1024)):
        with pytest.raises(K.LmxError):
            K.hiera_bands(*bad)


def _plan(nh, n=1, **kw):
    cfg = sam.hiera_b_plus()
    return sam.hiera_plan(cfg, n, _rule(cfg, nh, 1024), **kw), sam.hiera_plan(cfg, n, 256, **kw)


def test_plan_of_a_1080p_frame():
    band, whole = _plan(576, n=2)
    assert [(i, p.join, p.H) for i, p in enumerate(band) if p.join] == [(6, 38, 42), (12, 42, 64)]
    assert [(p.H, p.Hf, p.Ho, p.Hfo) for p in band[:6]] == [(152, 256, 152, 256)] * 2 + [(152, 256, 76, 128)] + [(76, 128, 76, 128)] * 2 + [(76, 128, 38, 64)]
    assert [(p.H, p.W, p.Hf) for p in band[6:12]] == [(42, 64, 64)] * 6
    assert band[12]._replace(join=0) == whole[12] and band[13:] == whole[13:]
    assert band[6].ln1 == band[12].ln1 == "launch"  # layer_norm1 behind any join is a launch of its own
    assert [i for i, p in enumerate(band) if p.join_out] == [1, 4] and not any(p.clone for p in band)
    for a, b in zip(band[:12], whole[:12]):  # the band runs the whole grid's kernels: what the table's bits rest on
        assert a.choices() == b.choices()
    low = sam.hiera_plan(sam.hiera_b_plus(), 2, _rule(sam.hiera_b_plus(), 576, 1024), lowest=2)
    assert not any(p.join_out or p.x16 for p in low[:12]) and [p.join for p in low] == [p.join for p in band]


def test_plan_of_a_frame_whose_band_ends_early():
    band, whole = _plan(894)
    assert [(i, p.join, p.H) for i, p in enumerate(band) if p.join] == [(6, 58, 64)]
    assert [(p.H, p.Ho) for p in band[:6]] == [(232, 232)] * 2 + [(232, 116)] + [(116, 116)] * 2 + [(116, 58)]
    assert band[6]._replace(join=0, ln1=whole[6].ln1) == whole[6] and band[7:] == whole[7:]
    for a, b in zip(band[:12], whole[:12]):
        assert a.choices() == b.choices()
    nb, nw_ = _plan(1024)
    assert nb == nw_  # no band: the whole grid's plan, no join


def test_one_number_is_its_rows_per_block():
    cfg = sam.hiera_b_plus()
    per = (168,) * 3 + (84,) * 3 + (42,) * 6 + _whole(cfg)[12:]
    for lowest in (0, 2):
        assert sam.hiera_plan(cfg, 2, per, lowest=lowest) == sam.hiera_plan(cfg, 2, 168, lowest=lowest)
    assert sam.hiera_plan(cfg, 1, _whole(cfg)) == sam.hiera_plan(cfg, 1, 256)
    with pytest.raises(ValueError):
        sam.hiera_plan(cfg, 1, per[:-1])
    with pytest.raises(ValueError):
        sam.hiera_plan(cfg, 1, (168,) * 3 + (76,) * 3 + per[6:])  # fewer rows than block 2 left
    with pytest.raises(ValueError):
        sam.hiera_plan(cfg, 1, (168,) * 3 + (84,) * 3 + (70,) * 6 + per[12:])  # more than the grid


def test_small_canvases_of_the_gpu_tests():
    for image, (h, w), rows, joins in ((256, (1080, 1920), (40, 20, 14), [(6, 10, 14), (12, 14, 16)]),
                                       (320, (230, 320), (64, 32, 20), [(6, 16, 20)]),
                                       (256, (100, 256), (32, 16, 14), [(6, 8, 14), (12, 14, 16)])):
        cfg = sam.HieraConfig(image=image)
        nh, nw = sam.resize_longest_side(h, w, image)
        r = _rule(cfg, nh, nw)
        assert _stages(r) == rows, image
        band, whole = sam.hiera_plan(cfg, 2, r), sam.hiera_plan(cfg, 2, image // 4)
        assert [(i, p.join, p.H) for i, p in enumerate(band) if p.join] == joins
        assert all(a.choices() == b.choices() for a, b in zip(band[:12], whole[:12]))


def test_encoder_settles_rows_on_the_whole_grids_kernels(monkeypatch):
    """An encoder built on the CPU (the constructor launches nothing).  The rule's rows pass every shape check, so block_rows is the
    rule; a block whose check fails on them runs on the next count of whole windows that passes, with the whole grid's kernel."""
    from lmx import weights

    cfg = sam.HieraConfig(image=256)
    sd = weights.synth_state_dict(sam.param_spec(cfg), 5)
    enc = sam.HieraEncoder(cfg, sd, "cpu", band="blocks")
    nh, nw = sam.resize_longest_side(1080, 1920, 256)
    rule = _rule(cfg, nh, nw)
    assert enc.block_rows(nh, nw) == enc.block_rows(nh, nw, 2) == rule and enc.band_rows(nh, nw) == 56
    rows, plan, whole = enc._settle(nh, nw, 2, lowest=2)
    assert rows == rule and plan == enc.plan(2, rule, lowest=2) and whole == enc.plan(1, 64)
    assert enc._table_key(nh, nw, rule, whole) == enc._table_key(nh, nw, rule) == (nh, nw, rule, tuple(p.choices() for p in whole[:12]))
    assert enc._table_key(nh, nw, rule) != enc._table_key(nh, nw, 56)
    assert enc._settle(*sam.resize_longest_side(1920, 1080, 256), 1) == (_whole(cfg), None, None)
    ok8, ok4 = K.hiera_attn8_ok, K.hiera_attn4_ok
    with monkeypatch.context() as m:
        m.setattr(K, "hiera_attn8_ok", lambda D, heads, win, Gh, Gw, qs: Gh != 40 and ok8(D, heads, win, Gh, Gw, qs))
        assert sam.hiera_plan(cfg, 1, rule)[0].attn == "launches"  # what the rule's rows alone would run
        rows = enc.block_rows(nh, nw)
        assert (rows[:3], rows[3:6], rows[6:]) == ((48,) * 3, (24,) * 3, rule[6:])  # the next whole windows, and what they leave
        plan = enc.plan(1, rows)
        assert [(i, p.join, p.H) for i, p in enumerate(plan) if p.join] == [(6, 12, 14), (12, 14, 16)]
        assert all(a.choices() == b.choices() for a, b in zip(plan[:12], enc.plan(1, 64)[:12]))
    # blocks 3 and 4 cannot run on 20 rows.  On 24 a join would sit in front of block 3 and its layer_norm1 would be a launch of its
    # own, where the whole grid's comes from block 2's MLP kernel: another choice, so the band ends there
    monkeypatch.setattr(K, "hiera_attn4_ok", lambda D, heads, win, Gh, Gw, qs: Gh != 20 and ok4(D, heads, win, Gh, Gw, qs))
    rows = enc.block_rows(nh, nw)
    assert (rows[:3], rows[3:12]) == (rule[:3], (32,) * 3 + (16,) * 6)
    plan = enc.plan(1, rows)
    assert [(i, p.join, p.H) for i, p in enumerate(plan) if p.join] == [(3, 20, 32)] and plan[4:] == enc.plan(1, 64)[4:]
    with pytest.raises(ValueError):
        sam.HieraEncoder(cfg, sd, "cpu", band="rows")
