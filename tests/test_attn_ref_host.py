"""The attention bound of tests/attnref.py has teeth (CPU only): the f16 model of the kernels' arithmetic stays within
C_ATTN * bound on every stress input, and each modelled kernel defect misses it by at least TEETH x on the input built to
expose it.  tests/test_gpu_attention.py holds the kernels themselves to the same bound."""
import pytest

import attnref as A

# (id, (B, H, Tq, Tk, hd, window), rel_S): small shapes of every geometry the kernels take
SHAPES = [
    ("flat multi-tile", (2, 2, 70, 300, 64, None), None),
    ("flat one tile, hd 16", (3, 2, 7, 40, 16, None), None),
    ("window 4 q_stride 2", (18, 2, 4, 16, 32, dict(Gh=12, Gw=12, ws=4, q_stride=2)), None),
    ("window 4 padded 10x10", (18, 2, 16, 16, 48, dict(Gh=10, Gw=10, ws=4, q_stride=1)), None),
    ("window 14 padded 20x20", (4, 2, 196, 196, 56, dict(Gh=20, Gw=20, ws=14, q_stride=1)), None),
    ("rel-pos flat S16", (1, 2, 256, 256, 64, None), 16),
    ("rel-pos window 14 padded", (4, 2, 196, 196, 64, dict(Gh=20, Gw=20, ws=14, q_stride=1)), 14),
]
CASES = [(sid, shape, rel_S, kind) for sid, shape, rel_S in SHAPES for kind in A.STRESSES
         if kind != "pad_heavy" or shape[5] is not None]

# defect -> (stress that exposes it, shapes it applies to)
DEFECT_CASES = [
    ("mask_last", "late_max", "flat multi-tile"),
    ("mask_last", "late_max", "window 4 padded 10x10"),
    ("mask_last", "late_max", "window 14 padded 20x20"),
    ("pad_zero", "pad_heavy", "window 4 padded 10x10"),
    ("pad_zero", "pad_heavy", "window 14 padded 20x20"),
    ("no_rescale", "late_max", "flat multi-tile"),
    ("no_rescale", "late_max", "window 14 padded 20x20"),
    ("flush", "subnormal_mass", "flat multi-tile"),
    ("flush", "subnormal_mass", "flat one tile, hd 16"),
    ("flush", "subnormal_mass", "window 14 padded 20x20"),
    ("swap_rel", "benign", "rel-pos flat S16"),
    ("swap_rel", "benign", "rel-pos window 14 padded"),
]


def _geo(shape):
    B, H, Tq, Tk, hd, win = shape
    return A.Geo(B, H, Tq, Tk, hd, win)


@pytest.mark.parametrize("sid,shape,rel_S,kind", CASES, ids=[f"{c[0]}-{c[3]}" for c in CASES])
def test_f16_model_within_bound(sid, shape, rel_S, kind):
    geo = _geo(shape)
    inp = A.make_inputs(kind, geo, seed=11, rel_S=rel_S)
    r, _ = A.evaluate(inp, geo)
    print(f"f16 model {sid} {kind}: {A.lg(r)} (bound {A.lg(A.C_ATTN)})")
    assert r <= A.C_ATTN, f"{sid} {kind}: the f16 model is {A.lg(r)} > {A.lg(A.C_ATTN)}"


@pytest.mark.parametrize("defect,kind,sid", DEFECT_CASES, ids=[f"{c[0]}-{c[2]}" for c in DEFECT_CASES])
def test_defect_misses_bound(defect, kind, sid):
    shape, rel_S = next((s, r) for i, s, r in SHAPES if i == sid)
    geo = _geo(shape)
    inp = A.make_inputs(kind, geo, seed=12, rel_S=rel_S)
    t, _ = A.evaluate(inp, geo, defect=defect)
    print(f"defect {defect} on {sid} {kind}: {t / A.C_ATTN:.0f} x the bound")
    assert t >= A.TEETH * A.C_ATTN, f"{defect} on {sid}: within {t / A.C_ATTN:.1f} x the bound: the bound has no teeth"


def test_stress_inputs_do_what_they_say():
    """large overflows exp without the max subtraction; late_max puts every row's maximum on the last valid key, several units
    above the rest; subnormal_mass at Tk = 4096 carries >= 10 % of a row's mass in the f16 subnormal range."""
    geo = A.Geo(1, 2, 70, 300, 64)
    _, ref = A.evaluate(A.make_inputs("large", geo, 1), geo)
    assert float(ref[3]["s"].max()) > 88.73
    _, ref = A.evaluate(A.make_inputs("late_max", geo, 1), geo)
    s = ref[3]["s"]
    assert bool((s.argmax(-1) == geo.Tk - 1).all()) and float((s[..., -1] - s[..., :-1].max(-1).values).min()) > 3
    geo = A.Geo(1, 1, 8, 4096, 64)
    _, ref = A.evaluate(A.make_inputs("subnormal_mass", geo, 1), geo)
    p = ref[1]
    rel = p / p.max(-1, keepdim=True).values
    sub = (rel >= 2.0 ** -17) & (rel < 2.0 ** -14)
    assert int(sub.sum(-1).min()) == geo.Tk - 1 and float((p * sub).sum(-1).min()) >= 0.10
