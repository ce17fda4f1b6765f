"""The constants of tests/maskref.py, established on the CPU without the code under test: per geometry the error of torch's own
f32 resize against float64 (e_ref), from which the device's bound against float64 follows; the share of fixture pixels whose
sign that bound leaves open; and that the reference says what include/lmx.h says.  tests/test_gpu_mask_output.py holds
lmx_k_hyper_mask / _multi, lmx_k_mask_post, lmx_k_mask_logits and lmx_k_mask_score to these numbers."""
import numpy as np
import pytest
import torch

import maskref as M

_CACHE = {}


def _measured(geo):
    if geo not in _CACHE:
        _CACHE[geo] = M.e_ref(geo)
    return _CACHE[geo]


def _lg(r):
    return f"2^{np.log2(max(r, 1e-300)):.2f}"


def test_every_geometry_has_its_constants():
    from lmx import sam

    assert set(M.LOG2_BOUND64) == set(M.SEEDS) == set(M.GEOMETRIES) and len(set(M.GEOMETRIES)) == len(M.GEOMETRIES) == 11
    for h, w, L, T in M.GEOMETRIES:
        assert M.resized(h, w, T) == sam.resize_longest_side(h, w, T)


@pytest.mark.parametrize("geo", M.GEOMETRIES, ids=M.geo_id)
def test_resize_bound_comes_from_the_reference_alone(geo):
    """A geometry keeps the existing 2^-18 max|low| where torch's CPU f32 path stays within half of it; one that does not has
    4 x e_ref rounded up to a power of two, so e_ref <= bound / 4 there (and the bound is the smallest such power of two)."""
    e, _, _ = _measured(geo)
    lb = M.LOG2_BOUND64[geo]
    print(f"resize {M.geo_id(geo)}: e_ref {_lg(e)} of max|low|, device bound against float64 2^{lb}")
    if lb == M.LOG2_KEPT:
        assert e <= 2.0 ** lb / 2, f"e_ref {_lg(e)} is above half of 2^{lb}: this geometry needs its own bound"
    else:
        assert lb > M.LOG2_KEPT and 2.0 ** lb / 8 < e <= 2.0 ** lb / 4, f"e_ref {_lg(e)}: 2^{lb} is not 4 x e_ref rounded up"
    assert M.LOG2_BOUND32 == -20


@pytest.mark.parametrize("geo", M.GEOMETRIES, ids=M.geo_id)
def test_fixture_masks_are_decided_and_mixed(geo):
    """At most 1 pixel per 10 000 of every mask lies within the bound of 0, and no fixture mask is empty or full."""
    h, w = geo[:2]
    _, ref64, top = _measured(geo)
    assert ref64.shape == (M.N_MASKS, h, w)
    amb = M.ambiguous(ref64, M.bound64(geo, top))
    for i in range(M.N_MASKS):
        k, area = int(amb[i].sum()), int((ref64[i] > 0).sum())
        print(f"fixture {M.geo_id(geo)} mask {i}: {k} ambiguous = {k / (h * w) * 1e4:.3f} per 10 000, coverage {area / (h * w):.3f}")
        assert k <= M.AMBIGUOUS_CAP * h * w, (i, k)
        assert 0 < area < h * w, (i, area)


@pytest.mark.parametrize("hw", [(333, 517), (97, 130)], ids=["333x517", "97x130"])
def test_made_masks_are_what_they_are_made_to_be(hw):
    h, w = hw
    rhw = M.resized(h, w, 1024)
    got = {k: M.postprocess(M.made_low(k).double(), 1024, rhw, hw)[0] for k in ("empty", "full", "border")}
    assert float(got["empty"].max()) == -10.0 and float(got["full"].min()) == 10.0
    assert M.stats(got["empty"] > 0) == [0, 0, 0, None, None, None, None]
    assert M.stats(got["full"] > 0) == M.full_stats(h, w)
    b = got["border"]
    st = M.stats(b > 0)
    assert st[3:] == [0, 0, w - 1, h - 1] and 0 < st[0] < h * w
    # the two bars across the longer side decide the box, far from the threshold: rounding cannot move it
    assert bool((b[0] > 1).all() and (b[:, 0] > 1).all() and (b[:, -1] > 1).all()) and float(b[-1, :1]) > 1 and float(b[-1, -1:]) > 1


def test_stats_are_plain_sums():
    m = np.zeros((5, 7), np.uint8)
    m[1, 2] = m[1, 6] = m[4, 3] = 1
    assert M.stats(m) == [3, 11, 6, 2, 1, 6, 4]
    sx, sy = int(np.arange(3840, dtype=np.int64).sum()) * 2160, int(np.arange(2160, dtype=np.int64).sum()) * 3840
    assert M.full_stats(2160, 3840) == [2160 * 3840, sx, sy, 0, 0, 3839, 2159] and sx == 15921100800 > 2 ** 32
    assert M.stats(np.ones((4, 6), bool)) == M.full_stats(4, 6)


def test_hyper_mask_is_the_sentence_in_lmx_h():
    """Cell by cell on a small launch: logits[b, 4y + 2dy1 + dy2, 4x + 2dx1 + dx2] = sum_c up[b, y, x, dy1, dx1, dy2, dx2, c] *
    hyper[b, c]; an f32 fma chain stays within the bound; the reference with the two quadrant levels exchanged misses it."""
    n, G, C = 2, 3, 8
    g = torch.Generator().manual_seed(5)
    up = torch.randn(n, G, G, 2, 2, 2, 2, C, generator=g).half()
    hy = torch.randn(n, C, generator=g)
    ref, mag = M.hyper_mask(up, hy)
    assert ref.shape == mag.shape == (n, 4 * G, 4 * G)
    u, h = up.double().numpy(), hy.double().numpy()
    for b in range(n):
        for y in range(G):
            for x in range(G):
                for dy1, dx1, dy2, dx2 in np.ndindex(2, 2, 2, 2):
                    want = float((u[b, y, x, dy1, dx1, dy2, dx2] * h[b]).sum())
                    assert abs(float(ref[b, 4 * y + 2 * dy1 + dy2, 4 * x + 2 * dx1 + dx2]) - want) <= 1e-12
    chain = torch.zeros(n, G, G, 2, 2, 2, 2)
    for c in range(C):  # f32 products are not exact here as they are inside an fma, which only loosens this check
        chain = (chain.double() + up[..., c].double() * hy[:, c].double().view(n, 1, 1, 1, 1, 1, 1)).float()
    got = chain.permute(0, 1, 3, 5, 2, 4, 6).reshape(n, 4 * G, 4 * G).double()
    bound = M.hyper_mask_bound(mag, C)
    assert float(((got - ref).abs() / bound).max()) <= 1.0
    swapped, _ = M.hyper_mask(up.permute(0, 1, 2, 5, 6, 3, 4, 7), hy)
    assert float(((got - swapped).abs() / bound).max()) >= 100
    multi, mmag = M.hyper_mask(up, torch.stack([hy, -2 * hy], 1))
    assert torch.equal(multi[:, 0], ref) and torch.equal(multi[:, 1], -2 * ref) and torch.equal(mmag[:, 1], 2 * mag)
