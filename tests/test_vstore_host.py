"""The vector store's host twin (csrc/host_vstore.cpp) without a GPU: the pinned dot product against float64, the order of
(score, slot) pairs on planted cases, `limits` against the search-then-append loop it stands for, and the unit rows."""
import numpy as np
import pytest

import vstoreref as V


def _f64(G, Q):
    return G.astype(np.float64) @ Q.astype(np.float64).T  # [N, Q]


@pytest.mark.parametrize("D", [4, 260, 384, 1024])
@pytest.mark.parametrize("N", [37, 3000])
def test_twin_against_float64(D, N):
    """Scores within bound(D) of the float64 dot of the same f32 unit rows; slots equal rank by rank wherever float64 separates a rank
    from both neighbours by more than 2 bound(D), which it must do for at least 95 % of the (query, rank) pairs."""
    rng = np.random.default_rng(0)
    k, nq = 32, 9
    G, Q = V.unit_gauss(rng, N, D), V.unit_gauss(rng, nq, D)
    ref = _f64(G, Q)
    b = V.bound(D)
    order = np.argsort(-ref, axis=0, kind="stable")[: k + 1].T  # [nq, k + 1]
    sorted_ref = np.take_along_axis(ref.T, order, axis=1)
    gaps = -np.diff(sorted_ref, axis=1)  # gaps[q, j]: rank j to rank j + 1
    clear = np.ones((nq, k), bool)
    clear[:, 1:] &= gaps[:, : k - 1] > 2 * b
    clear &= gaps[:, :k] > 2 * b
    print(f"D {D} N {N}: bound {b:.2e}, tightest top-{k + 1} gap {gaps.min():.2e}, unclear pairs {int((~clear).sum())} of {clear.size}")
    assert (~clear).mean() <= 0.05
    scores, slots = V.h_topk(G, Q, k)
    assert (slots >= 0).all() and (slots < N).all()
    err = np.abs(scores.astype(np.float64) - np.take_along_axis(ref.T, slots.astype(np.int64), axis=1))
    print(f"  worst score error {err.max():.2e}")
    assert err.max() <= b
    assert np.array_equal(slots[clear], order[:, :k][clear])
    assert (np.diff(scores, axis=1) <= 0).all()


def test_duplicates_give_the_lower_slot_first():
    rng = np.random.default_rng(1)
    G, Q = V.unit_gauss(rng, 40, 260), V.unit_gauss(rng, 2, 260)
    for s in (31, 7, 19):
        G[s] = Q[0]
    G[5] = G[2]
    scores, slots = V.h_topk(G, Q, 5)
    assert slots[0, :3].tolist() == [7, 19, 31] and scores[0, 0] == scores[0, 1] == scores[0, 2]
    full_s, full_i = V.h_topk(G, Q, 32)
    at = full_i[1].tolist().index(2)
    assert full_i[1, at + 1] == 5 and full_s[1, at] == full_s[1, at + 1]


def test_all_negative_scores():
    """a top-k that starts from score 0 returns nothing here"""
    rng = np.random.default_rng(2)
    q = V.unit_gauss(rng, 1, 384)
    G = V.ladder(rng, q[0], 12, 0.15, 0.9, sign=-1.0)
    scores, slots = V.h_topk(G, q, 5)
    assert slots[0].tolist() == [0, 1, 2, 3, 4]
    assert (scores < 0).all() and np.allclose(scores[0], -np.linspace(0.15, 0.9, 12)[:5], atol=1e-5)


def test_empty_gallery_and_fewer_rows_than_k():
    rng = np.random.default_rng(3)
    Q = V.unit_gauss(rng, 3, 8)
    scores, slots = V.h_topk(np.zeros((0, 8), np.float32), Q, 5)
    assert (slots == -1).all() and (scores == 0).all()
    G = V.unit_gauss(rng, 3, 8)
    scores, slots = V.h_topk(G, Q, 5)
    assert (slots[:, 3:] == -1).all() and (scores[:, 3:] == 0).all()
    assert all(sorted(r[:3].tolist()) == [0, 1, 2] for r in slots)


def test_limits_are_a_shorter_gallery():
    rng = np.random.default_rng(4)
    N, k = 50, 5
    G, Q = V.unit_gauss(rng, N, 260), V.unit_gauss(rng, 4, 260)
    limits = [0, 1, 23, N]
    scores, slots = V.h_topk(G, Q, k, limits)
    for j, lim in enumerate(limits):
        s1, i1 = V.h_topk(G[:lim], Q[j : j + 1], k)
        assert np.array_equal(scores[j : j + 1], s1) and np.array_equal(slots[j : j + 1], i1)
    assert (slots[0] == -1).all() and slots[1].tolist() == [0, -1, -1, -1, -1]
    # beyond the ends: clamped
    s2, i2 = V.h_topk(G, Q, k, [-3, 1, 23, N + 9])
    assert np.array_equal(s2, scores) and np.array_equal(i2, slots)


def test_limits_stand_for_search_then_append():
    """a backlog of B new rows in one call = B search-then-append steps, equal bytes"""
    rng = np.random.default_rng(5)
    n0, B, D, k = 20, 11, 384, 5
    G = V.unit_gauss(rng, n0 + B, D)
    G[n0 + 4] = G[n0 + 1]  # a later clip that repeats an earlier one of the backlog finds it
    new = np.ascontiguousarray(G[n0:])
    scores, slots = V.h_topk(G, new, k, n0 + np.arange(B))
    for j in range(B):
        s1, i1 = V.h_topk(np.ascontiguousarray(G[: n0 + j]), new[j : j + 1], k)
        assert np.array_equal(scores[j : j + 1], s1) and np.array_equal(slots[j : j + 1], i1)
    assert slots[4, 0] == n0 + 1


def test_row_stride():
    rng = np.random.default_rng(6)
    G = V.unit_gauss(rng, 30, 260)
    wide = np.full((30, 272), np.float32(7.0))
    wide[:, :260] = G
    Q = V.unit_gauss(rng, 2, 260)
    a, b = V.h_topk(G, Q, 5), V.h_topk(wide[:, :260], Q, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [4, 260, 1024])
def test_unit_rows(dtype, D):
    """the float64 expression to one f32 rounding; a zero row gives zeros"""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((6, D)) * np.array([1e-3, 1, 1, 50, 1e4, 1])[:, None]).astype(dtype)
    x[2] = 0
    out = V.h_unit(x)
    x64 = x.astype(np.float64)
    ref = x64 / (np.sqrt((x64 * x64).sum(1, keepdims=True)) + 1e-8)
    half_ulp = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.isfinite(out).all() and (out[2] == 0).all()
    assert (np.abs(out.astype(np.float64) - ref) <= half_ulp * (1 + 1e-6)).all()
    assert np.allclose(np.linalg.norm(out[[0, 1, 3, 4, 5]].astype(np.float64), axis=1), 1, atol=1e-6)


@pytest.mark.parametrize("D,k", [(6, 5), (0, 5), (4100, 5), (8, 0), (8, 33)])
def test_refusals(D, k):
    G, Q = np.zeros((3, max(D, 4)), np.float32), np.zeros((1, max(D, 4)), np.float32)
    rc, scores, slots = V.h_topk_rc(G, Q, k, D=D)
    assert rc == V.EINVAL and "lmx_h_cosine_topk" in V.last_error()
    assert (slots == -7).all()  # nothing written
    if k == 5:
        rc, _ = V.h_unit_rc(np.zeros((1, max(D, 4)), np.float32), D=D)
        assert rc == V.EINVAL and "lmx_h_unit_rows" in V.last_error()


def test_workspace_and_geometry():
    from lmx import vstore

    lib = V._lib.load()
    R, T, per_cu = vstore.geometry(1024)
    assert R >= 1 and T >= 1 and per_cu >= 1
    assert vstore.geometry(4096)[1] >= 1
    assert lib.lmx_h_cosine_topk_workspace(0, 4, 5) == 0
    assert lib.lmx_h_cosine_topk_workspace(R + 1, 3, 5) == 2 * 3 * 5 * 8
    assert lib.lmx_h_cosine_topk_workspace(10 ** 6, 64, 32) <= 64 << 20
