"""The Hiera encoder's block plan computed in C (lmx_h_hiera_plan, lmx_h_hiera_plan_rows: csrc/host_hiera_plan.cpp) against the Python
plan it restates, without a GPU: every field of every BlockPlan equals lmx.sam.hiera_plan's, and the rows per block equal
HieraEncoder(band="blocks").block_rows — the settling loop included.  The encoders are built on "cpu": their constructors launch no
kernel.

R8 is Hiera-B+ cut to eight blocks, one of every kind Hiera-B+ has: attn8_ln, attn8, attn_pool 112 -> 224, attn4, attn_pool
224 -> 448, windowed-14 launches, global launches, and the stage-4 opener on pooled GEMMs.

FRAMES: the band's cases at image 1024, each asserted below as a property and not only as numbers
  (90, 160)  -> 576 x 1024   a join sits inside the band, in front of the first 14-window block
  (139, 160) -> 890 x 1024   224 / 112 / 56 = 4 * 14 rows: no join before the one in front of the global block
  (150, 100)                 portrait, nw < 1024: no band
  (64, 64)                   no padding: no band"""
import dataclasses

import pytest

from lmx import kernels as K
from lmx import sam, weights

SWITCHES = ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL", "LMX_HIERA_ATTN_POOL3", "LMX_MLP_IMG", "LMX_NO_FUSED_MLP")
R8 = sam.HieraConfig(blocks=(2, 2, 3, 1), global_blocks=(6,))
# R8 with 6 x 6 windows in stage 2: the rule's rows put a join in front of block 3, whose layer_norm1 rows the whole grid takes from
# block 2's MLP kernel — another choice than the whole grid's, so the settling loop has to add rows (with the windows of Hiera-B+
# the rule's rows pass every check and the loop never turns)
R8W6 = dataclasses.replace(R8, windows=(8, 6, 14, 7))
CONFIGS = {"R8": R8, "B+": sam.hiera_b_plus(), "R8w6": R8W6}
IMAGES = (256, 512, 1024)
BATCHES = (1, 2, 3, 16)
FRAMES = [(90, 160), (139, 160), (150, 100), (64, 64), (1080, 1920), (720, 1280)]


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def encoders():
    """{(name, image): HieraEncoder(band="blocks") on the CPU}; the weights do not enter the plan."""
    out = {}
    for name, base in CONFIGS.items():
        sd = weights.synth_state_dict(sam.param_spec(base), seed=5)  # (no parameter's shape depends on `image`)
        for image in IMAGES:
            out[name, image] = sam.HieraEncoder(dataclasses.replace(base, image=image), sd, "cpu", band="blocks")
    return out


def _python(enc, nh, nw, n, lowest):
    """(rows per block, plan) as HieraEncoder.encode runs them: the band's, or the whole grid's where there is none."""
    rows, plan, _ = enc._settle(nh, nw, n, lowest)
    return tuple(rows), plan if plan is not None else enc.plan(n, enc.grid0, lowest)


def _heights(image):
    """Every height whose (nh + 2) // 4 + 1 rows differ from the one before: each count of token rows once, so every multiple of
    every window (8, 4, 14 at their resolutions) is crossed."""
    return [1] + list(range(2, image + 1, 4)) + [image]


@pytest.mark.parametrize("image", IMAGES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_plan_equals_pythons(encoders, name, image):
    enc = encoders[name, image]
    cfg = enc.cfg
    sizes = [sam.resize_longest_side(h, w, image) for h, w in FRAMES] + [(nh, image) for nh in _heights(image)]
    seen, banded = set(), 0
    for nh, nw in sizes:
        for n in BATCHES:
            for lowest in (0, 2):
                rows, plan = _python(enc, nh, nw, n, lowest)
                got_rows, got = sam.native_plan(cfg, n, nh, nw, lowest)
                assert got_rows == rows == enc.block_rows(nh, nw, n), (nh, nw, n, lowest)
                assert len(got) == len(plan)
                for i, (a, b) in enumerate(zip(got, plan)):
                    assert a == b, (nh, nw, n, lowest, i, [f for f in a._fields if getattr(a, f) != getattr(b, f)])
                    for f in ("ln_out", "emit_ln1", "stage_end", "keep", "x16", "join_out", "clone"):
                        assert type(getattr(a, f)) is type(getattr(b, f)) is bool
                seen |= {(P.attn, P.shortcut, P.query, P.mlp, P.ln1) for P in got}
                banded += rows[0] < enc.grid0
    assert banded > len(sizes)  # (the sweep is not all whole grids)
    attn = {s[0] for s in seen}
    assert attn == {"attn8_ln", "attn8", "attn_pool", "attn4", "launches"} - ({"attn4"} if name == "R8w6" else set())
    assert {s[4] for s in seen} == {"kernel", "prev", "launch"} and {s[3] for s in seen} == {"img", "launches"}
    if image == 256:  # the stage-4 opener on 16 x 16 tokens: 256 rows a frame, the pooled GEMM only from two frames on
        assert {"gemm+maxpool", "pooled_gemm"} <= {s[1] for s in seen} and {"qkv+maxpool", "pooled_q+kv", "qkv"} <= {s[2] for s in seen}


def test_r8_has_every_form_of_hiera_b_plus(encoders):
    for n in (1, 3):
        rows, plan = sam.native_plan(R8, n, 1024, 1024, 2)
        assert rows == (256, 256, 256, 128, 128, 64, 64, 64)
        assert [(P.attn, P.mlp) for P in plan] == [("attn8_ln", "img"), ("attn8", "img"), ("attn_pool", "img"), ("attn4", "img"),
                                                   ("attn_pool", "launches"), ("launches", "launches"), ("launches", "launches"),
                                                   ("launches", "launches")]
        assert [P.ln1 for P in plan] == ["kernel", "prev", "prev", "prev", "prev", "launch", "launch", "launch"]
        assert [P.ln_out for P in plan] == [False] * 5 + [True, True, False] and [P.window for P in plan] == [8, 8, 8, 4, 4, 14, 0, 14]
        assert (plan[7].shortcut, plan[7].query) == ("pooled_gemm", "pooled_q+kv")
        assert [P.keep for P in plan] == [False] * 6 + [True, True] and [P.stage_end for P in plan] == [False, True, False, True, False, False, True, True]
    # every attention form, every MLP form and every layer_norm1 source of the full model (its 896-wide blocks behind the stage-4
    # opener run the plain launches without ln_out, which R8's single stage-4 block does not have: the same launches as a global block's)
    full = sam.native_plan(sam.hiera_b_plus(), 1, 1024, 1024, 2)[1]
    for key in (lambda P: (P.attn, P.mlp), lambda P: P.ln1, lambda P: P.shortcut, lambda P: P.query):
        assert {key(P) for P in plan} == {key(P) for P in full}


def test_frames_of_the_band(encoders):
    """The properties the GPU tests of the C encoder rely on, for R8 at image 1024."""
    enc = encoders["R8", 1024]
    first_global = enc.first_global
    # a join inside the band: the 14-window block needs 42 rows, the pooling block in front of it left 38
    nh, nw = sam.resize_longest_side(90, 160)
    rows, plan = sam.native_plan(R8, 3, nh, nw, 2)
    assert (nh, nw) == (576, 1024) and rows == (152, 152, 152, 76, 76, 42, 64, 64)
    joins = [i for i, P in enumerate(plan) if P.join]
    assert joins == [5, first_global] and plan[5].join == 38 and plan[5].H == 42 < plan[5].Hf and plan[first_global].H == plan[first_global].Hf == 64
    # no join before the global block's: every block takes the rows the one before left
    nh, nw = sam.resize_longest_side(139, 160)
    rows, plan = sam.native_plan(R8, 3, nh, nw, 2)
    assert (nh, nw) == (890, 1024) and rows == (224, 224, 224, 112, 112, 56, 64, 64) and 56 == 4 * 14
    assert [i for i, P in enumerate(plan) if P.join] == [first_global] and plan[first_global].join == 56
    # portrait and square: the whole grid, no join, nothing joined at a stage end
    for h, w in ((150, 100), (64, 64)):
        nh, nw = sam.resize_longest_side(h, w)
        rows, plan = sam.native_plan(R8, 3, nh, nw, 2)
        assert (nw < 1024 or nh == 1024) and rows == (256, 256, 256, 128, 128, 64, 64, 64)
        assert not any(P.join or P.join_out for P in plan)
    assert sam.resize_longest_side(150, 100) == (1024, 683) and sam.resize_longest_side(64, 64) == (1024, 1024)


def test_settling_moves_rows_and_never_kernels(encoders):
    """Where the band's plan on the rule's rows would make another choice than the whole grid's (R8w6: a join in front of a block
    whose layer_norm1 rows the whole grid takes from the MLP kernel before it), the C plan adds rows as Python does — the sweep above
    compares them; here: it happens at all, only there, rows are only ever added, and the band's kernel choices are the whole grid's."""
    moved = {name: 0 for name in CONFIGS}
    for (name, image), enc in encoders.items():
        blocks = enc.cfg.block_plan()
        whole = sam.native_plan(enc.cfg, 1, image, image)[1]
        for nh in _heights(image):
            rule = K.hiera_bands([b[3] for b in blocks], [b[4] for b in blocks], image // 4, nh, image)
            rows, plan = sam.native_plan(enc.cfg, 1, nh, image)
            assert all(r >= q for r, q in zip(rows, rule))
            moved[name] += rows != rule
            assert all(P.choices() == Q.choices() for P, Q in list(zip(plan, whole))[:enc.first_global] if P.H < P.Hf)
    assert moved["R8w6"] > 0 and moved["R8"] == moved["B+"] == 0, moved


def test_plan_rows_equals_hiera_plan(encoders):
    """lmx_h_hiera_plan_rows on rows of the caller's: the rule's rows unsettled, one number as its rows per block (lmx_h_hiera_band),
    the whole grid — and what hiera_plan refuses."""
    for (name, image), enc in encoders.items():
        cfg, blocks = enc.cfg, enc.cfg.block_plan()
        wins, qss = [b[3] for b in blocks], [b[4] for b in blocks]
        whole, g = [], image // 4
        for b in blocks:
            whole.append(g)
            g = g // 2 if b[4] else g
        for nh in (1, image // 3, image // 2 + 2, image * 9 // 16, image - 40, image):
            one = K.hiera_band(wins, qss, image // 4, nh, image)
            per_one, d = [], one
            for i, b in enumerate(blocks):
                per_one.append(d if one and i < enc.first_global else whole[i])
                d = d // 2 if b[4] else d
            for rows in (K.hiera_bands(wins, qss, image // 4, nh, image), tuple(per_one), tuple(whole)):
                for n in (1, 16):
                    for lowest in (0, 2):
                        assert sam.native_plan_rows(cfg, n, rows, lowest) == sam.hiera_plan(cfg, n, rows, True, lowest, True), (name, image, nh, rows)
            assert sam.native_plan_rows(cfg, 2, tuple(per_one), 2) == sam.hiera_plan(cfg, 2, one or image // 4, True, 2, True)
    cfg = encoders["R8", 1024].cfg
    for rows in ((152, 144, 152, 76, 76, 42, 64, 64), (152, 152, 152, 76, 76, 70, 64, 64), (264, 256, 256, 128, 128, 64, 64, 64)):
        with pytest.raises(ValueError):
            sam.hiera_plan(cfg, 1, rows)
        with pytest.raises(K.LmxError, match="lmx_h_hiera_plan_rows: block"):
            sam.native_plan_rows(cfg, 1, rows)
    with pytest.raises(K.LmxError, match="row counts for 8 blocks"):
        sam.native_plan_rows(cfg, 1, (256,) * 7)


def test_the_c_plan_reads_no_switch(monkeypatch):
    want = sam.native_plan(R8, 2, 576, 1024, 2)
    for v in SWITCHES:
        monkeypatch.setenv(v, "0")
    monkeypatch.setenv("LMX_MLP448", "1")
    assert sam.native_plan(R8, 2, 576, 1024, 2) == want


def test_argument_errors():
    bad = [(dict(blocks=(2, 2, 3, 0)), "blocks\\[3\\] = 0"), (dict(global_blocks=(8,)), "global_blocks\\[0\\] = 8 is not a block of 0 .. 7"),
           (dict(image=1022), "image 1022"), (dict(windows=(8, 4, 0, 7)), "stage 2: dims 448 heads 8 windows 0")]
    for change, msg in bad:
        with pytest.raises(K.LmxError, match=msg):
            sam.native_plan(dataclasses.replace(R8, **change), 1, 576, 1024)
    for args, msg in (((0, 576, 1024), "n=0"), ((1, 0, 1024), "nh=0"), ((1, 576, 1028), "nw=1028"), ((70000, 576, 1024), "n=70000")):
        with pytest.raises(K.LmxError, match=msg):
            sam.native_plan(R8, *args)
    with pytest.raises(K.LmxError, match="lowest=-1"):
        sam.native_plan(R8, 1, 576, 1024, -1)
    with pytest.raises(K.LmxError, match="does not fit"):
        sam.native_plan(dataclasses.replace(R8, global_blocks=tuple(range(33))), 1, 576, 1024)
    assert sam.native_plan(R8, 1, 576, 1024)[0] == (152, 152, 152, 76, 76, 42, 64, 64)  # (and the intact one still plans)
