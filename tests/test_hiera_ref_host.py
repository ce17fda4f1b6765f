"""tests/hieraref.py checked on the CPU: its per-window float64 operations equal the whole-grid definitions tests/test_gpu_kernels.py
spells out (evaluated in float64), walk() gives the hand-checked passes and start slots, and the defect models miss C_FUSED by TEETH."""
import pytest
import torch
import torch.nn.functional as F

import hieraref as R
import test_gpu_persistent as GP


def _case(kernel, n, Gh, Gw, seed=1):
    gen = torch.Generator().manual_seed(seed)
    p = R.f64(R.make_params(kernel, gen))
    x, h = R.make_acts(kernel, n * Gh * Gw, gen)
    return p, (x.double() if x is not None else None), (h.double() if h is not None else None)


def _grid_attn(x, h, p, n, Gh, Gw, ws, heads):
    """test_hiera_attn8_fused_block / test_hiera_attn4_fused_block's definition (a), in float64."""
    D = x.shape[1]
    hd, T = D // heads, ws * ws
    qkv = h @ p["wqkv"].t() + p["bqkv"]
    t = qkv.view(n, Gh // ws, ws, Gw // ws, ws, 3, heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, -1, heads, T, hd)
    att = torch.softmax(t[0] @ t[1].transpose(-1, -2) * hd ** -0.5, -1) @ t[2]
    att = att.view(n, Gh // ws, Gw // ws, heads, ws, ws, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(-1, D)
    return x + att @ p["wo"].t() + p["bo"]


def _grid_attn_pool(h, p, n, Gh, Gw, ws, heads):
    """test_hiera_attn_pool_fused_block's definition, in float64."""
    D = p["wo"].shape[0]
    hd, wq = D // heads, ws // 2

    def pool(t):
        return F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)

    sc = pool((h @ p["wsc"].t() + p["bsc"]).view(n, Gh, Gw, D))
    qkv = (h @ p["wqkv"].t() + p["bqkv"]).view(n, Gh, Gw, 3, D)
    q = pool(qkv[..., 0, :])
    q = q.reshape(n, Gh // ws, wq, Gw // ws, wq, heads, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, heads, wq * wq, hd)
    kk, vv = (qkv[..., j, :].reshape(n, Gh // ws, ws, Gw // ws, ws, heads, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, heads, ws * ws, hd)
              for j in (1, 2))
    att = torch.softmax(q @ kk.transpose(-1, -2) * hd ** -0.5, -1) @ vv
    att = att.view(n, Gh // ws, Gw // ws, heads, wq, wq, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, Gh // 2, Gw // 2, D)
    return (sc + att @ p["wo"].t() + p["bo"]).reshape(-1, D)


@pytest.mark.parametrize("kernel,form,n,Gh,Gw", [("attn8", "ln", 2, 16, 24), ("attn8", "h", 2, 24, 16), ("attn4", "h", 3, 8, 12),
                                                 ("attnp", "h", 2, 16, 24), ("attnq", "h", 3, 12, 8)])
def test_windows_equal_the_grid_definition(kernel, form, n, Gh, Gw):
    g = R.GEOM[kernel]
    ws, heads = g["ws"], g["heads"]
    p, x, h = _case(kernel, n, Gh, Gw)
    nwin = n * (Gh // ws) * (Gw // ws)
    rows = R.window_rows(range(nwin), Gh, Gw, ws)
    if g["pool"]:
        want = _grid_attn_pool(h, p, n, Gh, Gw, ws, heads)
        got = R.reference(kernel, None, h[rows], p)
        out_rows = R.window_rows(range(nwin), Gh // 2, Gw // 2, ws // 2)
    else:
        hh = F.layer_norm(x, (g["D"],), p["gam"], p["bet"], R.EPS) if form == "ln" else h
        want = _grid_attn(x, hh, p, n, Gh, Gw, ws, heads)
        got = R.reference(kernel, x[rows], None if form == "ln" else h[rows], p, form=form)
        out_rows = rows
    assert sorted(out_rows.flatten().tolist()) == list(range(want.shape[0]))  # the windows tile the grid
    assert float((got - want[out_rows]).abs().max()) <= 1e-12


@pytest.mark.parametrize("kernel", ["mlp112", "mlp224"])
def test_mlp_rows_equal_the_definition(kernel):
    """test_ln_mlp_img's definition, in float64."""
    D = R.GEOM[kernel]["D"]
    p, x, _ = _case(kernel, 1, 1, 300)
    hh = F.layer_norm(x, (D,), p["g2"], p["e2"], R.EPS)
    want = x + F.gelu(hh @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"]
    wantn = F.layer_norm(want, (D,), p["gn"], p["en"], R.EPS)
    got = R.reference(kernel, x, None, p)
    assert float((got[:, :D] - want).abs().max()) <= 1e-12 and float((got[:, D:] - wantn).abs().max()) <= 1e-12
    # in blocks of rows
    parts = torch.cat([R.reference(kernel, x[a:b], None, p) for a, b in ((0, 7), (7, 200), (200, 300))])
    assert float((parts - got).abs().max()) <= 1e-12


def test_images_per_group_come_from_the_packers():
    assert [R.images_per_group(k) for k in ("attn4", "attnp", "attnq", "mlp112", "mlp224")] == [16, 14, 47, 7, 28]


def test_walk_of_streamed_kernels():
    # 3 workgroups, 11 groups of 47 images: passes 0 0 0 1 1 1 2 2 2 3 3, start slots 0, 47 % 4 = 3, 94 % 4 = 2, 141 % 4 = 1
    w = R.walk("attnq", 11, 3)
    assert [u[0] for u in w] == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    assert [u[1] for u in w] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3]
    assert [u[2] for u in w] == [0, 0, 0, 3, 3, 3, 2, 2, 2, 1, 1]
    assert sorted({(u[1], u[2]) for u in R.walk("attnp", 2 * 5 + 3, 5)}) == [(0, 0), (1, 2), (2, 0)]        # 14 images
    assert sorted({(u[1], u[2]) for u in R.walk("mlp112", 4 * 5 + 3, 5)}) == [(0, 0), (1, 3), (2, 2), (3, 1), (4, 0)]  # 7 images
    assert {u[2] for u in R.walk("attn4", 40, 5)} == {0} and {u[2] for u in R.walk("mlp224", 40, 5)} == {0}  # 16, 28 images
    # fewer groups than CUs: one pass, one workgroup each
    assert R.walk("attn4", 3, 8) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]


def test_walk_of_attn8():
    # 2 CUs, 19 windows: 5 wave quadruples on 2 workgroups; windows 16..18 are workgroup 0's third pass
    w = R.walk("attn8", 19, 2)
    assert [u[0] for u in w] == [0] * 4 + [1] * 4 + [0] * 4 + [1] * 4 + [0] * 3
    assert [u[1] for u in w] == [0] * 8 + [1] * 8 + [2] * 3
    assert R.walk("attn8", 6, 8) == [(0, 0, 0)] * 4 + [(1, 0, 0)] * 2


def test_walk_of_attn_spp():
    # 16 workgroups (2 per XCD), 37 items: iq 4, ir 5 -> XCDs 0..4 own 5 items, 5..7 own 4.  XCD 0 = workgroups 0 and 8 over items
    # 0..4: workgroup 0 walks 0, 2, 4 and workgroup 8 walks 1, 3; XCD 5 starts at item 25: workgroup 5 walks 25, 27, workgroup 13 26, 28
    w = R.walk("attn_spp", 37, 16)
    assert w[:5] == [(0, 0, 0), (8, 0, 0), (0, 1, 1), (8, 1, 1), (0, 2, 0)]
    assert w[25:29] == [(5, 0, 0), (13, 0, 0), (5, 1, 1), (13, 1, 1)]
    assert w[36] == (15, 1, 1)
    # fewer items than CUs: one item per workgroup, XCD x owns its contiguous share
    assert sorted(u[0] for u in R.walk("attn_spp", 20, 64)) == list(range(20)) and {u[1] for u in R.walk("attn_spp", 20, 64)} == {0}
    # 12 workgroups: XCDs 0..3 have two, 4..7 one
    w = R.walk("attn_spp", 64, 12)
    assert [u[1] for u in w[:8]] == [0, 0, 1, 1, 2, 2, 3, 3] and [u[1] for u in w[32:40]] == list(range(8))


def test_gpu_plans_reach_every_slot_at_any_cu_count():
    """The coverage assertions of tests/test_gpu_persistent.py hold whatever the CU count: every start slot, a partial last group on
    pass >= 2, single-pass chunks."""
    for cu in (32, 64, 104, 256, 304):
        for kernel, slots in GP.EXPECTED_SLOTS.items():
            pl = GP.Plan(kernel, cu)
            pl.check_coverage(slots)
            pl.chunks()


def test_round_up_partial():
    assert R.round_up_partial(2054, 6, 4) == 2058 and R.round_up_partial(8229, 4, 16) == 8232
    assert R.round_up_partial(4115, 4, 8) == 4116 and R.round_up_partial(16421, 4, 16) == 16424
    assert R.round_up_partial(32, 4, 16) == 36


TEETH_CASES = [(k, f, d) for k, f in (("attn8", "ln"), ("attn8", "h"), ("attn4", "h"), ("attnp", "h"), ("attnq", "h"))
               for d in ("stale_matrix", "drop_key")] + [("mlp112", "h", "stale_matrix"), ("mlp224", "h", "stale_matrix")]


@pytest.mark.parametrize("kernel,form,defect", TEETH_CASES, ids=[f"{k}-{f}-{d}" for k, f, d in TEETH_CASES])
def test_bound_catches_the_defect_models(kernel, form, defect):
    """A stale ring slot (the last head's v matrix is the previous head's; the MLP's last fc1 step is the previous one) and a missing
    last key, on the inputs of tests/test_gpu_persistent.py (make_params / make_acts, the same small images), must miss C_FUSED by
    TEETH x under ratio()."""
    g = R.GEOM[kernel]
    gen = torch.Generator().manual_seed(7)
    p = R.f64(R.make_params(kernel, gen))
    if kernel.startswith("mlp"):
        x, _ = R.make_acts(kernel, 2 * g["per_group"], gen)
        args = (x, None)
        arg = dict(stale_matrix=4 * g["D"] // 64 - 1)
    else:
        Gh, Gw = g["img"]
        n = 4
        x, h = R.make_acts(kernel, n * Gh * Gw, gen)
        rows = R.window_rows(range(n * (Gh // g["ws"]) * (Gw // g["ws"])), Gh, Gw, g["ws"])
        args = (x[rows] if x is not None else None, h[rows] if form == "h" else None)
        arg = dict(stale_matrix=g["heads"] - 1) if defect == "stale_matrix" else dict(drop_key=True)
    ref = R.reference(kernel, *args, p, form=form)
    bad = R.reference(kernel, *args, p, form=form, **arg)
    t = R.ratio(bad, ref)
    print(f"teeth {kernel} {form} {defect}: {R.lg(t)} = {t / R.C_FUSED:.0f} x C_FUSED")
    assert t >= R.TEETH * R.C_FUSED
