"""Every branch of lmx_k_attention (csrc/attn.hip) against the float64 reference of tests/attnref.py, under the bound

    |got - ref| <= C_ATTN * ( |ref| + sum_j p_j |v_jd| (1 + E_j) + 2^-14 * sum_j |v_jd| / L )

on the stress inputs of attnref.make_inputs (benign, large logits, a late maximum, f16-subnormal probability mass, dominant
padded keys).  Branches are reached by shape only (the LMX_ATTN_* switches are process-wide statics); each case id names the
kernel the dispatch picks for it and each row of SHAPES ends with that kernel's route name (lmx_h_attn_route, include/lmx.h), which
the test asserts of the library's own selection before it launches (tests/test_dispatch_routes_host.py does so without a GPU).
q / k / v are views with ld > H * hd inside NaN-filled buffers (gap columns and the rows after
the last described row), `out` a strided view of a sentinel-filled buffer: every result must be finite and every cell outside
the described output must keep the sentinel.  The tests print each case's ratio as a power of two.

Two spp rows hold more items than the device has CUs (3 CU + 6 / 3 CU + 8: a function of the CU count, resolved in the test), so that a
workgroup of the persistent kernel walks three or four items and hands its double-buffered LDS image over between them; the test
asserts through hieraref.walk that the sampled rows hold the items at positions 0, 1, 2 and last of one workgroup's walk."""
import math

import pytest
import torch

import attnref as A
import hieraref

pytestmark = pytest.mark.gpu

C_ATTN, TEETH = A.C_ATTN, A.TEETH
SENT = -1234.0        # exactly representable in f16
F32_EXP_MAX = 88.73   # exp(s) overflows f32 above this (f16 above 11.09)

ALL = ("benign", "large", "late_max", "subnormal_mass")
WIN = ALL + ("pad_heavy",)
BL = ("benign", "late_max")


def _win(Gh, ws, qs=1):
    return dict(Gh=Gh, Gw=Gh, ws=ws, q_stride=qs)


def _multi_flat(cu):
    """B x H = 3 CU + 6 items of T 201 (B rounded up to whole batch elements of 2 heads)."""
    return (-(-(3 * cu + 6) // 2), 2, 201, 201, 64, None)


def _multi_win(cu):
    """images x 4 windows x 2 heads = 3 CU + 8 items (rounded up to whole images): the four 14 x 14 windows of a 20 x 20 image have
    four different padding patterns, so consecutive items of a workgroup alternate edge and interior DMA plans over one LDS image."""
    return (4 * -(-(3 * cu + 8) // 8), 2, 196, 196, 56, _win(20, 14))


def resolve(shape, cu):
    """A row's shape: a tuple, or a function of the device's CU count."""
    return shape(cu) if callable(shape) else shape


# (id naming the branch, family, (B, H, Tq, Tk, hd, window) or a function of the CU count giving it, rel_S, stresses, route)
SHAPES = [
    ("small 7x7 hd32 items15", "small", (3, 5, 7, 7, 32, None), None, ALL, "small"),
    ("small Tq16 Tk1 hd64", "small", (2, 3, 16, 1, 64, None), None, ("benign", "late_max"), "small"),
    ("small Tq1 Tk16 hd16", "small", (24, 1, 1, 16, 16, None), None, ALL, "small"),
    ("small win4 qs2 12x12", "small", (2 * 9, 3, 4, 16, 32, _win(12, 4, 2)), None, ALL, "small"),
    ("small win4 padded 10x10", "small", (2 * 9, 3, 16, 16, 48, _win(10, 4)), None, WIN, "small"),
    ("kernel<1> ones Tq7 Tk4096 hd16", "kernel", (2, 8, 7, 4096, 16, None), None, ALL, "tiled_q1_ones_hd64"),
    ("kernel<1> dot2 Tq17 Tk300 hd64", "kernel", (2, 3, 17, 300, 64, None), None, ALL, "tiled_q1_dot2_hd64"),
    ("kernel<1> ones Tq33 Tk100 hd8", "kernel", (2, 2, 33, 100, 8, None), None, ALL, "tiled_q1_ones_hd64"),
    ("kernel<1> ones Tq64 Tk130 hd24", "kernel", (1, 3, 64, 130, 24, None), None, ALL, "tiled_q1_ones_hd64"),
    ("kernel<2> ones Tq4096 Tk7 hd16", "kernel", (2, 8, 4096, 7, 16, None), None, ALL, "tiled_q2_ones_hd64"),
    ("kernel<2> dot2 T209 hd64", "kernel", (2, 3, 209, 209, 64, None), None, ALL, "tiled_q2_dot2_hd64"),
    ("kernel<2> dot2 Tq500 Tk100 hd64", "kernel", (1, 2, 500, 100, 64, None), None, ALL, "tiled_q2_dot2_hd64"),
    ("kernel<2> ones win16 padded 20x20 hd48", "kernel", (4, 2, 256, 256, 48, _win(20, 16)), None, WIN, "tiled_q2_ones_hd64"),
    ("wide hd72 Tq30 Tk100", "wide", (2, 2, 30, 100, 72, None), None, ALL, "tiled_q1_dot2_hd96"),
    ("wide hd80 Tq300 Tk150", "wide", (1, 2, 300, 150, 80, None), None, ALL, "tiled_q1_dot2_hd96"),
    ("wide hd96 Tq100 Tk600", "wide", (1, 2, 100, 600, 96, None), None, ALL, "tiled_q1_dot2_hd96"),
    ("wide hd80 win14 padded 20x20", "wide", (4, 2, 196, 196, 80, _win(20, 14)), None, WIN, "tiled_q1_dot2_hd96"),
    ("sp ones T201 hd56", "sp", (2, 4, 201, 201, 56, None), None, ALL, "sp_qb2_ones"),
    ("spp ones T201 hd56", "spp", (4, 16, 201, 201, 56, None), None, ALL, "spp_ones"),
    ("sp dot2 T201 hd64", "sp", (2, 4, 201, 201, 64, None), None, ALL, "sp_qb2_dot2"),
    ("spp dot2 T201 hd64", "spp", (4, 16, 201, 201, 64, None), None, ALL, "spp_dot2"),
    ("sp ones Tq65 Tk208 hd56", "sp", (2, 3, 65, 208, 56, None), None, BL, "sp_qb2_ones"),
    ("spp ones Tq65 Tk208 hd56", "spp", (8, 8, 65, 208, 56, None), None, BL, "spp_ones"),
    ("sp dot2 Tq65 Tk208 hd64", "sp", (2, 3, 65, 208, 64, None), None, BL, "sp_qb2_dot2"),
    ("spp dot2 Tq65 Tk208 hd64", "spp", (8, 8, 65, 208, 64, None), None, BL, "spp_dot2"),
    ("sp ones Tq208 Tk129 hd56", "sp", (2, 3, 208, 129, 56, None), None, BL, "sp_qb2_ones"),
    ("spp ones Tq208 Tk129 hd56", "spp", (8, 8, 208, 129, 56, None), None, BL, "spp_ones"),
    ("sp dot2 Tq208 Tk129 hd64", "sp", (2, 3, 208, 129, 64, None), None, BL, "sp_qb2_dot2"),
    ("spp dot2 Tq208 Tk129 hd64", "spp", (8, 8, 208, 129, 64, None), None, BL, "spp_dot2"),
    ("sp ones win14 padded 20x20 hd56", "sp", (4, 4, 196, 196, 56, _win(20, 14)), None, WIN, "sp_qb2_ones"),
    ("spp ones win14 padded 20x20 hd56", "spp", (16, 4, 196, 196, 56, _win(20, 14)), None, WIN, "spp_ones"),
    ("sp dot2 win14 padded 20x20 hd64", "sp", (4, 4, 196, 196, 64, _win(20, 14)), None, WIN, "sp_qb2_dot2"),
    ("spp dot2 win14 padded 20x20 hd64", "spp", (16, 4, 196, 196, 64, _win(20, 14)), None, WIN, "spp_dot2"),
    ("sp dot2 items63 T201", "sp", (63, 1, 201, 201, 64, None), None, BL, "sp_qb2_dot2"),
    ("spp dot2 items64 T201", "spp", (64, 1, 201, 201, 64, None), None, BL, "spp_dot2"),
    ("spp dot2 T201 hd64 items 3CU+6", "spp", _multi_flat, None, ("benign", "large"), "spp_dot2"),
    ("spp ones win14 padded 20x20 hd56 items 3CU+8", "spp", _multi_win, None, ("late_max", "pad_heavy"), "spp_ones"),
    ("gp ones T256 hd56", "gp", (1, 2, 256, 256, 56, None), None, ALL, "gp4_ones"),
    ("gp dot2 T256 hd64", "gp", (1, 2, 256, 256, 64, None), None, ALL, "gp4_dot2"),
    ("gp ones T257 hd56", "gp", (2, 2, 257, 257, 56, None), None, ALL, "gp4_ones"),
    ("gp dot2 T257 hd64", "gp", (2, 2, 257, 257, 64, None), None, ALL, "gp4_dot2"),
    ("gp ones T4096 hd56", "gp", (1, 2, 4096, 4096, 56, None), None, ALL, "gp4_ones"),
    ("gp dot2 T4096 hd64", "gp", (1, 2, 4096, 4096, 64, None), None, ALL, "gp4_dot2"),
    ("gp ones Tq65 Tk300 hd56", "gp", (2, 2, 65, 300, 56, None), None, ALL, "gp4_ones"),
    ("gp dot2 Tq65 Tk300 hd64", "gp", (2, 2, 65, 300, 64, None), None, ALL, "gp4_dot2"),
    ("gp ones Tq1024 Tk4096 hd56", "gp", (1, 2, 1024, 4096, 56, None), None, BL, "gp4_ones"),
    ("gp dot2 Tq1024 Tk4096 hd64", "gp", (1, 2, 1024, 4096, 64, None), None, BL, "gp4_dot2"),
    ("rel kernel<2> S64 hd64", "rel", (1, 2, 4096, 4096, 64, None), 64, ("benign", "large", "late_max"), "tiled_q2_dot2_rel_hd64"),
    ("rel wide S64 hd80", "rel", (1, 2, 4096, 4096, 80, None), 64, ("benign", "large", "late_max"), "tiled_q1_dot2_rel_hd96"),
    ("rel kernel<1> win8 padded 12x12 hd64", "rel", (4, 2, 64, 64, 64, _win(12, 8)), 8, ("benign", "late_max", "pad_heavy"), "tiled_q1_dot2_rel_hd64"),
    ("rel kernel<2> win16 padded 20x20 hd64", "rel", (4, 2, 256, 256, 64, _win(20, 16)), 16, ("benign", "late_max", "pad_heavy"), "tiled_q2_dot2_rel_hd64"),
    ("rel wide win16 padded 20x20 hd80", "rel", (4, 2, 256, 256, 80, _win(20, 16)), 16, ("benign", "late_max", "pad_heavy"), "tiled_q1_dot2_rel_hd96"),
    ("rel kernel<2> win14 padded 20x20 hd64", "rel", (4, 2, 196, 196, 64, _win(20, 14)), 14, ("benign", "large", "pad_heavy"), "tiled_q2_dot2_rel_hd64"),
    ("rel wide win14 padded 20x20 hd80", "rel", (4, 2, 196, 196, 80, _win(20, 14)), 14, ("benign", "large", "pad_heavy"), "tiled_q1_dot2_rel_hd96"),
]
CASES = [(sid, fam, shape, rel_S, kind, route) for sid, fam, shape, rel_S, kinds, route in SHAPES for kind in kinds]
VIEW_COL0, VIEW_GAP = 8, 16  # _view: q / k / v / out are views with ld = 8 + H * hd + 16


def shape_route(shape, rel_S, cu=None):
    """The route lmx_k_attention takes for a row of SHAPES as run_attention launches it (windows with both pad vectors); cu: the
    CU count for the rows that depend on it."""
    from lmx import kernels as K_

    B, H, Tq, Tk, hd, win = resolve(shape, cu)
    return K_.attention_route(B, H, Tq, Tk, hd, window=win, pad=win is not None, rel_S=rel_S or 0, ld=VIEW_COL0 + H * hd + VIEW_GAP)


def _geo(shape):
    B, H, Tq, Tk, hd, win = shape
    return A.Geo(B, H, Tq, Tk, hd, win)


def _view(x, cuda, fill=math.nan, col0=VIEW_COL0, gap=VIEW_GAP, extra_rows=5):
    """x [rows, D] -> (buffer, view): the view starts at column col0 of a buffer with ld = col0 + D + gap and extra_rows more
    rows, everything outside the view filled with `fill`."""
    rows, D = x.shape
    buf = torch.full((rows + extra_rows, col0 + D + gap), fill, dtype=torch.float16, device=cuda)
    view = buf[:rows, col0:col0 + D]
    if x.numel():
        view.copy_(x.to(cuda))
    return buf, view


def run_attention(inp, geo, cuda, pads=True, Tk=None):
    """Launch lmx_k_attention on sentinel-guarded device copies of `inp`; -> the f16 output [q_rows, H*hd] on the CPU.
    Asserts that every output is finite and that nothing outside the output view was written."""
    from lmx import kernels as K_

    D = geo.H * geo.hd
    q, k, v = (_view(inp[n], cuda)[1] for n in ("q", "k", "v"))
    obuf, out = _view(torch.full((geo.q_rows, D), SENT), cuda, fill=SENT)
    obuf_ref = obuf.clone()
    pk = inp["pad_k"].to(cuda) if pads and inp["pad_k"] is not None else None
    pv = inp["pad_v"].to(cuda) if pads and inp["pad_v"] is not None else None
    rel = tuple(r.to(cuda) for r in inp["rel"]) if inp["rel"] is not None else None
    K_.attention(q, k, v, out, geo.B, geo.H, geo.Tq, Tk or geo.Tk, geo.hd, geo.scale, window=geo.window, pad_k=pk, pad_v=pv,
                 rel_pos=rel)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "non-finite output"
    obuf_ref[:geo.q_rows, 8:8 + D] = out
    assert torch.equal(obuf, obuf_ref), "cells outside the output view were written"
    return out.cpu()


def walked_sample(geo, cu):
    """The row sample of a many-items spp case: rows_sample plus the first and last two query rows of every item the first
    longest-walking workgroup of the persistent kernel visits (item = b * H + h; an output row holds every head of its batch
    element | window).  Asserts that the sample holds that workgroup's items at positions 0, 1, 2 and last -> (rows, a line)."""
    items = geo.B * geo.H
    assert items > 3 * cu, "every workgroup must walk at least three items"
    by_wg = {}
    for item, (wg, p, _) in enumerate(hieraref.walk("attn_spp", items, cu)):
        by_wg.setdefault(wg, {})[p] = item
    lens = sorted({len(v) for v in by_wg.values()})
    assert lens[0] >= 3 and lens[-1] >= 4, lens
    wg, its = next((w, v) for w, v in sorted(by_wg.items()) if len(v) == lens[-1])
    of_b = {}
    for r in range(geo.q_rows):
        of_b.setdefault(geo.locate(r)[0], []).append(r)
    extra = [r for it in its.values() for r in of_b[it // geo.H][:2] + of_b[it // geo.H][-2:]]
    rows = torch.tensor(sorted(set(A.rows_sample(geo.q_rows).tolist()) | set(extra)), dtype=torch.long)
    sampled = {geo.locate(r)[0] * geo.H + h for r in rows.tolist() for h in range(geo.H)}
    last = len(its) - 1
    assert last >= 3 and all(its[p] in sampled for p in (0, 1, 2, last))
    return rows, f"workgroups walk {lens} items; workgroup {wg} walks items {[its[p] for p in range(last + 1)]}, all sampled"


def _check_stress(kind, ref, geo):
    s, p = ref[3]["s"], ref[1]
    if kind == "large":
        assert float(s.max()) > F32_EXP_MAX, "large: exp without the max subtraction must overflow f32 somewhere"
    if kind == "subnormal_mass":
        rel = p / p.max(-1, keepdim=True).values
        mass = float((p * ((rel >= 2.0 ** -17) & (rel < 2.0 ** -14))).sum(-1).min())
        assert mass > 0
        if geo.Tk >= 4096:
            assert mass >= 0.10, f"subnormal_mass: only {mass:.3f} of a row's mass in the f16 subnormal range"
        return f" (subnormal-range mass >= {mass:.3f})"
    return ""


@pytest.mark.parametrize("sid,fam,shape,rel_S,kind,route", CASES, ids=[f"{c[0]}-{c[4]}" for c in CASES])
def test_attention_matches_float64(cuda, sid, fam, shape, rel_S, kind, route):
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    multi = callable(shape)
    shape = resolve(shape, cu)
    assert shape_route(shape, rel_S) == route, sid
    geo = _geo(shape)
    rows = A.rows_sample(geo.q_rows)
    if multi:
        rows, line = walked_sample(geo, cu)
        print(f"attention [{fam}] {sid}: {cu} CUs, {line}")
    inp = A.make_inputs(kind, geo, seed=sum(shape[:5]) + A.STRESSES.index(kind), rel_S=rel_S)
    got = run_attention(inp, geo, cuda)
    r, ref = A.evaluate(inp, geo, got[rows], rows=rows)
    extra = _check_stress(kind, ref, geo)
    print(f"attention [{fam}] {sid} {kind}: max ratio {A.lg(r)} (bound {A.lg(C_ATTN)}){extra}")
    assert r <= C_ATTN, f"{sid} {kind}: {A.lg(r)} > {A.lg(C_ATTN)}"


# ------------------------------------------------------------------------------------------------ teeth on the GPU
# the kernel's own output for a neighbouring problem must miss the bound of the original one by >= TEETH x:
# one key fewer on late_max (B = 1: the key rows of the single item do not move), no pad vectors on pad_heavy
TEETH_TK = [("small", (1, 3, 16, 16, 32, None)), ("kernel<1>", (1, 3, 17, 300, 64, None)), ("kernel<2>", (1, 3, 209, 209, 64, None)),
            ("wide", (1, 2, 100, 150, 80, None)), ("sp", (1, 4, 201, 201, 56, None)), ("spp", (1, 64, 201, 201, 64, None)),
            ("gp", (1, 2, 257, 257, 64, None))]
TEETH_PAD = [("small", (2 * 9, 3, 16, 16, 48, _win(10, 4))), ("kernel<2>", (4, 2, 256, 256, 48, _win(20, 16))),
             ("sp", (4, 4, 196, 196, 64, _win(20, 14))), ("spp", (16, 4, 196, 196, 56, _win(20, 14)))]


@pytest.mark.parametrize("name,shape", TEETH_TK, ids=[t[0] for t in TEETH_TK])
def test_attention_bound_catches_a_missing_last_key(cuda, name, shape):
    geo = _geo(shape)
    inp = A.make_inputs("late_max", geo, seed=5)
    rows = A.rows_sample(geo.q_rows)
    t, _ = A.evaluate(inp, geo, run_attention(inp, geo, cuda, Tk=geo.Tk - 1)[rows], rows=rows)
    print(f"teeth {name}: Tk - 1 on late_max misses the bound by {t / C_ATTN:.0f} x")
    assert t >= TEETH * C_ATTN, f"{name}: Tk - 1 stays within {t / C_ATTN:.1f} x the bound"


@pytest.mark.parametrize("name,shape", TEETH_PAD, ids=[t[0] for t in TEETH_PAD])
def test_attention_bound_catches_missing_pad_vectors(cuda, name, shape):
    geo = _geo(shape)
    inp = A.make_inputs("pad_heavy", geo, seed=6)
    rows = A.rows_sample(geo.q_rows)
    t, _ = A.evaluate(inp, geo, run_attention(inp, geo, cuda, pads=False)[rows], rows=rows)
    print(f"teeth {name}: pad_k / pad_v = None on pad_heavy misses the bound by {t / C_ATTN:.0f} x")
    assert t >= TEETH * C_ATTN, f"{name}: no pad vectors stays within {t / C_ATTN:.1f} x the bound"


# ------------------------------------------------------------------------------------------------ offsets beyond 2^31 bytes
@pytest.mark.parametrize("form", ["gp flat T4096", "spp win14 padded 20x20"])
def test_attention_last_item_beyond_2gb(cuda, form):
    """One qkv buffer (ld = 3072 halfs) of ~2.2 GB whose last batch element's rows start beyond 2^31 bytes, and an output of the
    same row stride: only the last element's sampled queries are checked against float64."""
    from lmx import kernels as K_

    ld, H, hd = 3072, 1, 64
    if form.startswith("gp"):
        last = A.Geo(1, H, 4096, 4096, hd)
        n = 87                                  # element 86 starts at 86 * 4096 * 6144 bytes = 2.16e9
        geo = A.Geo(n, H, 4096, 4096, hd)
    else:
        w = _win(20, 14)
        last = A.Geo(4, H, 196, 196, hd, w)
        n = 880                                 # image 879 starts at 879 * 400 * 6144 bytes = 2.16e9
        geo = A.Geo(4 * n, H, 196, 196, hd, w)
    per = last.k_rows
    r0 = geo.k_rows - per
    assert r0 * ld * 2 > 2 ** 31 and geo.q_rows == geo.k_rows
    inp = A.make_inputs("late_max", last, seed=9)
    qkv = torch.empty((geo.k_rows, ld), dtype=torch.float16, device=cuda)
    qkv.normal_()
    for i, name in enumerate("qkv"):
        qkv[r0:, i * 1024:i * 1024 + hd].copy_(inp[name].to(cuda))
    out = torch.full((geo.q_rows, ld), SENT, dtype=torch.float16, device=cuda)
    pk = inp["pad_k"].to(cuda) if inp["pad_k"] is not None else None
    pv = inp["pad_v"].to(cuda) if inp["pad_v"] is not None else None
    K_.attention(qkv[:, :hd], qkv[:, 1024:1024 + hd], qkv[:, 2048:2048 + hd], out[:, 8:8 + hd], geo.B, H, geo.Tq, geo.Tk, hd,
                 geo.scale, window=geo.window, pad_k=pk, pad_v=pv)
    torch.cuda.synchronize()
    assert bool((out[:, :8] == SENT).all()) and bool((out[:, 8 + hd:] == SENT).all()), "cells outside the output view were written"
    got = out[r0:, 8:8 + hd]
    assert bool(torch.isfinite(got).all())
    rows = A.rows_sample(last.q_rows)
    r, _ = A.evaluate(inp, last, got.cpu()[rows], rows=rows)
    print(f"attention {form}, last element beyond 2^31 bytes: max ratio {A.lg(r)} (bound {A.lg(C_ATTN)})")
    assert r <= C_ATTN
    del qkv, out
    torch.cuda.empty_cache()
