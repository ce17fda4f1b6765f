"""lmx.sam.hiera_plan on the host: the record of every Hiera-B+ block, what each environment switch changes in it, the band's join
and the key of the band's table.  No GPU; only the cases that ask K.hiera_band for a band need the shared library (kept apart at
the end of the file)."""
import pytest

from lmx import sam

SWITCHES = ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL", "LMX_HIERA_ATTN_POOL3", "LMX_MLP_IMG", "LMX_NO_FUSED_MLP")
STAGE_ENDS = (1, 4, 20, 23)


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _plan(n=1, rows=256, image=1024, **kw):
    return sam.hiera_plan(sam.HieraConfig(image=image), n, rows, **kw)


def _changed(a, b):
    """{block: {field: (a's, b's)}} over the records that differ."""
    return {i: {f: (getattr(p, f), getattr(q, f)) for f in p._fields if getattr(p, f) != getattr(q, f)}
            for i, (p, q) in enumerate(zip(a, b)) if p != q}


def _launches(p):
    return (p.attn, p.shortcut, p.query, p.ln_out)


def test_hiera_b_plus_whole_grid_block_by_block():
    plan = _plan()
    assert len(plan) == 24
    grids = [(p.H, p.W, p.Hf, p.Ho, p.Wo, p.Hfo) for p in plan]
    assert grids[:2] == [(256,) * 6] * 2 and grids[2] == (256, 256, 256, 128, 128, 128) and grids[3:5] == [(128,) * 6] * 2
    assert grids[5] == (128, 128, 128, 64, 64, 64) and grids[6:21] == [(64,) * 6] * 15
    assert grids[21] == (64, 64, 64, 32, 32, 32) and grids[22:] == [(32,) * 6] * 2
    assert not any(p.join or p.join_out for p in plan)
    # the attention halves and where layer_norm1 comes from
    assert (plan[0].attn, plan[0].ln1) == ("attn8_ln", "kernel")
    assert (plan[1].attn, plan[1].ln1) == ("attn8", "prev")
    assert (plan[2].attn, plan[2].ln1) == ("attn_pool", "prev")
    assert [(p.attn, p.ln1) for p in plan[3:5]] == [("attn4", "prev")] * 2
    assert (plan[5].attn, plan[5].ln1, plan[5].mlp) == ("attn_pool", "prev", "launches")
    for p in plan[:6]:
        assert (p.shortcut, p.query, p.ln_out) == (None, None, False)
    for i in range(6, 21):
        assert _launches(plan[i]) == ("launches", None, "qkv", True) and plan[i].ln1 == "launch", i
        assert plan[i].window == (0 if i in (12, 16, 20) else 14), i
    assert _launches(plan[21]) == ("launches", "pooled_gemm", "pooled_q+kv", False) and plan[21].window == 14
    for i in (22, 23):
        assert _launches(plan[i]) == ("launches", None, "qkv", False) and plan[i].window == 7 and plan[i].ln1 == "launch"
    assert [p.window for p in plan[:6]] == [8, 8, 8, 4, 4, 4]
    # the MLP halves: streamed images on blocks 0 - 4, each emitting the next layer_norm1 (no next block normalises itself here)
    assert [p.mlp for p in plan] == ["img"] * 5 + ["launches"] * 19
    assert [p.emit_ln1 for p in plan] == [True] * 5 + [False] * 19
    # stage ends
    assert tuple(i for i, p in enumerate(plan) if p.stage_end) == STAGE_ENDS
    assert all(plan[i].keep for i in STAGE_ENDS) and not any(p.keep for i, p in enumerate(plan) if i not in STAGE_ENDS)
    assert tuple(i for i, p in enumerate(plan) if p.x16) == (1, 4)
    assert not any(p.clone for p in plan)  # (every block behind a stage end changes the width: it writes a new stream)
    same = sam.hiera_plan(sam.HieraConfig(dims=(112, 112, 448, 896), heads=(2, 2, 8, 16)), 1, 256)
    assert [i for i, p in enumerate(same) if p.clone] == [1]  # a same-width block 2 would update the kept output in place


def test_each_switch_changes_exactly_its_records(monkeypatch):
    base = _plan()
    with monkeypatch.context() as m:
        m.setenv("LMX_HIERA_ATTN8", "0")
        assert _changed(base, _plan()) == {
            0: dict(attn=("attn8_ln", "launches"), ln1=("kernel", "launch"), query=(None, "qkv")),
            1: dict(attn=("attn8", "launches"), query=(None, "qkv"))}
    with monkeypatch.context() as m:
        m.setenv("LMX_HIERA_ATTN4", "0")
        assert _changed(base, _plan()) == {i: dict(attn=("attn4", "launches"), query=(None, "qkv")) for i in (3, 4)}
    pool = dict(attn=("attn_pool", "launches"), shortcut=(None, "pooled_gemm"), query=(None, "pooled_q+kv"))
    with monkeypatch.context() as m:
        m.setenv("LMX_HIERA_ATTN_POOL", "0")
        assert _changed(base, _plan()) == {2: pool, 5: pool}
    with monkeypatch.context() as m:
        m.setenv("LMX_HIERA_ATTN_POOL3", "0")
        assert _changed(base, _plan()) == {5: pool}
    with monkeypatch.context() as m:
        m.setenv("LMX_MLP_IMG", "0")
        assert _changed(base, _plan()) == {i: dict(mlp=("img", "fused")) for i in range(5)}
    assert _changed(base, _plan(proj_ln=False)) == {i: dict(ln_out=(True, False)) for i in range(6, 21)}


def test_without_fused_mlp_every_attn8_block_normalises_itself():
    base, plan = _plan(), _plan(fused_mlp=False)
    assert [(p.attn, p.ln1) for p in plan[:2]] == [("attn8_ln", "kernel")] * 2
    assert all(p.mlp == "launches" and not p.emit_ln1 and not p.x16 for p in plan)
    assert [p.ln1 for p in plan[2:]] == ["launch"] * 22
    assert [p.ln_out for p in plan] == [p.ln_out for p in base]  # (448 is no fused-MLP width either way)
    assert sam.attn8_ln_inside(0, True) and not sam.attn8_ln_inside(1, True) and sam.attn8_ln_inside(1, False)


def test_layer_norm1_rows_with_three_stage1_blocks():
    """The last block emits nothing; with three stage-1 blocks only the first normalises in its kernel."""
    assert not _plan()[-1].emit_ln1
    cfg = sam.HieraConfig(blocks=(3, 3, 16, 3))
    plan = sam.hiera_plan(cfg, 1, 256)
    assert [(p.attn, p.ln1, p.emit_ln1) for p in plan[:3]] == [("attn8_ln", "kernel", True), ("attn8", "prev", True), ("attn8", "prev", True)]


def test_band_of_168_rows():
    whole, band = _plan(n=2), _plan(n=2, rows=168)
    assert [i for i, p in enumerate(band) if p.join] == [12] and band[12].join == 42 and band[12].H == 64
    assert [(p.H, p.Hf) for p in band[:2]] == [(168, 256)] * 2 and (band[2].Ho, band[2].Hfo) == (84, 128) and (band[5].Ho, band[5].Hfo) == (42, 64)
    assert [(p.H, p.W, p.Hf) for p in band[6:12]] == [(42, 64, 64)] * 6
    assert band[12]._replace(join=0) == whole[12] and band[13:] == whole[13:]
    assert band[12].ln1 == "launch"  # the joined grid's layer_norm1 is a launch of its own
    assert [i for i, p in enumerate(band) if p.join_out] == [1, 4] and not any(p.clone for p in band)
    for a, b in zip(band[:12], whole[:12]):  # the band runs the whole grid's kernels: what the table's bits rest on
        assert a.choices() == b.choices()
    low = _plan(n=2, rows=168, lowest=2)
    assert _changed(band, low) == {1: dict(keep=(True, False), x16=(True, False), join_out=(True, False)),
                                   4: dict(keep=(True, False), x16=(True, False), join_out=(True, False))}
    assert [i for i, p in enumerate(low) if p.stage_end] == list(STAGE_ENDS)


def test_batch_size_changes_only_the_pooled_gemm_choices():
    one, two = _plan(n=1, rows=64, image=256), _plan(n=2, rows=64, image=256)
    assert _launches(one[21]) == ("launches", "gemm+maxpool", "qkv+maxpool", False)  # 16 x 16 = 256 rows < 512
    assert _changed(one, two) == {21: dict(shortcut=("gemm+maxpool", "pooled_gemm"), query=("qkv+maxpool", "pooled_q+kv"))}
    assert [p._replace(shortcut=None, query=None) for p in one] == [p._replace(shortcut=None, query=None) for p in two]


def test_plan_is_read_per_call(monkeypatch):
    a = _plan()
    monkeypatch.setenv("LMX_HIERA_ATTN4", "0")
    b = _plan()
    monkeypatch.delenv("LMX_HIERA_ATTN4")
    assert a != b and a == _plan()


def test_records_are_hashable_choices():
    plan = _plan()
    assert len({p.choices() for p in plan}) > 1 and hash(tuple(p.choices() for p in plan)) is not None
    with pytest.raises(AttributeError):
        plan[0].attn = "attn4"


def test_encoder_packs_by_shape_class_and_keys_its_table_by_the_building_pass(monkeypatch):
    """An encoder built on the CPU (the constructor launches nothing): operands for every block of a fused class, whatever the
    switches say, and the table key — which takes no batch size: it is the plan of the pass that builds the table, one frame on the
    whole grid in front of the first global block."""
    from lmx import weights

    monkeypatch.setenv("LMX_HIERA_ATTN8", "0")
    cfg = sam.HieraConfig(image=256)
    enc = sam.HieraEncoder(cfg, weights.synth_state_dict(sam.param_spec(cfg), 5), "cpu")
    monkeypatch.delenv("LMX_HIERA_ATTN8")
    assert [i for i, b in enumerate(enc.blocks) if "attn" in b] == [0, 1, 2, 3, 4, 5]
    assert [tuple(b["attn"][0].shape) for b in enc.blocks[:6]] == [(384, 128), (384, 128), (14, 16384), (16, 16384), (16, 16384), (47, 16384)]
    assert [i for i, b in enumerate(enc.blocks) if "mlp_img" in b] == [0, 1, 2, 3, 4]
    assert enc.first_global == 12 and enc.plan(2, 56, lowest=2) == sam.hiera_plan(cfg, 2, 56, True, 2, True)
    key = enc._table_key(144, 256, 56)
    assert key == (144, 256, 56, tuple(p.choices() for p in sam.hiera_plan(cfg, 1, 64)[:12]))
    assert key[3] == tuple(p.choices() for p in sam.hiera_plan(cfg, 2, 64)[:12])  # (block 21's pooled GEMMs lie behind the band)
    keys = {key}
    for v in ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL"):
        monkeypatch.setenv(v, "0")
    keys.add(enc._table_key(144, 256, 56))
    monkeypatch.setenv("LMX_MLP_IMG", "0")
    keys.add(enc._table_key(144, 256, 56))
    assert len(keys) == 3
    enc.proj_ln = False
    assert not any(p.ln_out for p in enc.plan(1, 64))


# ---- with the shared library (K.hiera_band) -------------------------------------------------------------------------------------------
def test_band_rule_on_the_256_canvas():
    from lmx import kernels as K

    blocks = sam.HieraConfig(image=256).block_plan()
    band = K.hiera_band([b[3] for b in blocks], [b[4] for b in blocks], 64, *sam.resize_longest_side(1080, 1920, 256))
    assert band == 56
    plan = sam.hiera_plan(sam.HieraConfig(image=256), 2, band)
    assert [(i, p.join, p.H) for i, p in enumerate(plan) if p.join] == [(12, 14, 16)]
