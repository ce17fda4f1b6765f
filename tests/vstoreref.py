"""What the vector-store tests share: the host twin (lmx_h_cosine_topk, lmx_h_unit_rows) through ctypes on numpy arrays, the error
bound of the pinned dot product, and seeded unit rows.  No GPU."""
import ctypes as C
import math

import numpy as np

from lmx import _lib

EINVAL = -1


def bound(D):
    """|pinned dot - exact| for unit rows: ceil(D / 256) + 8 roundings on the longest path (the fmaf chain of a partial, then eight
    halving adds), each relative to at most sum |q g| <= 1; 1 % for the rows' own distance from unit length."""
    return 1.01 * (math.ceil(D / 256) + 8) * 2.0 ** -24


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def h_unit_rc(raw, D=None):
    raw = np.ascontiguousarray(raw)
    n, D = raw.shape[0], (raw.shape[1] if D is None else D)
    out = np.full((n, max(D, 1)), np.float32(np.nan))
    rc = _lib.load().lmx_h_unit_rows(_p(raw), {np.dtype(np.float32): 1, np.dtype(np.float64): 2}[raw.dtype], n, D, _p(out), D)
    return rc, out


def h_unit(raw):
    rc, out = h_unit_rc(raw)
    _lib.check(rc, "lmx_h_unit_rows")
    return out


def h_topk_rc(G, Q, k, limits=None, D=None):
    """G [N, ldg >= D] f32 (a view with a row stride is passed as it stands), Q [Q, D] f32"""
    assert G.dtype == np.float32 and Q.dtype == np.float32 and (G.shape[0] == 0 or G.strides[1] == 4) and Q.flags.c_contiguous
    D = Q.shape[1] if D is None else D
    ldg = G.strides[0] // 4 if G.shape[0] > 1 else max(G.shape[1], D)
    lim = None if limits is None else np.ascontiguousarray(limits, np.int32)
    kk = max(k, 1)
    scores, slots = np.full((Q.shape[0], kk), np.float32(np.nan)), np.full((Q.shape[0], kk), -7, np.int32)
    rc = _lib.load().lmx_h_cosine_topk(_p(G), G.shape[0], D, ldg, _p(Q), Q.shape[0], _p(lim), k, _p(scores), _p(slots))
    return rc, scores, slots


def h_topk(G, Q, k, limits=None):
    rc, scores, slots = h_topk_rc(G, Q, k, limits)
    _lib.check(rc, "lmx_h_cosine_topk")
    return scores, slots


def last_error():
    return _lib.load().lmx_last_error().decode()


def unit_gauss(rng, n, D):
    return h_unit(rng.standard_normal((n, D)).astype(np.float32))


def ladder(rng, q, n, lo, hi, sign=1.0):
    """n unit rows whose cosines to the unit row q are sign * (lo .. hi), evenly spaced, row i the i-th: far apart next to `bound`"""
    D = q.shape[0]
    cos = np.linspace(lo, hi, n)
    rows = np.empty((n, D), np.float64)
    q64 = q.astype(np.float64)
    for i, c in enumerate(cos):
        o = rng.standard_normal(D)
        o -= (o @ q64) * q64 / (q64 @ q64)
        o /= np.linalg.norm(o)
        rows[i] = sign * c * q64 + math.sqrt(1 - c * c) * o
    return h_unit(rows)
