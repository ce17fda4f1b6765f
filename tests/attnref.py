"""Float64 reference, f16 rounding model and error bound of lmx_k_attention (include/lmx.h lmx_attn_desc, lmx/kernels.py
attention), written from the documented semantics and shared by tests/test_attn_ref_host.py (CPU) and
tests/test_gpu_attention.py (GPU).

    O[b, t, h, :] = softmax_j(scale * Q[b, t, h, :] . K[b, j, h, :] + bias[t, j]) V[b, j, h, :]

Geometry: flat (row = b * T + t) or windows of ws x ws keys on a [Gh][Gw] grid per image (padded keys take pad_k / pad_v, zeros
when None; queries on the grid subsampled by q_stride; queries in the padding produce no output row).  bias is SAM's decomposed
relative position term rel[t][ky] + rel[t][S + kx] with rel = q . R[q_pos - k_pos + S - 1] (lmx_k_relpos_tables).

The bound every kernel is held to, per output element (query i, feature d), with p_j the float64 probabilities and
L = sum_j exp(s_j - max s) >= 1:

    |got - ref| <= C * ( |ref| + sum_j p_j |v_jd| (1 + E_j) + 2^-14 * sum_j |v_jd| / L )

sum p|v| covers the 2^-11 rounding of every f16 P, the last term the f16 subnormal spacing of small P, and E_j is the logit
error in units of 2^-11: 2^-10 * scale * sum_d |q_d k_jd| for the f32 score and exp2 argument, plus for rel-pos
|bias_h| + |bias_w| + sum_d |q_d| (|Rh_d| + |Rw_d|) for the f16 tables.

Only a sample of query rows is computed (rows_sample), so that 4096-token problems stay cheap on the CPU."""
import math

import numpy as np
import torch

C_ATTN = 2.0 ** -10.5  # 1.85x the largest ratio measured on MI355X (2^-11.39, attn_sp on padded 14x14 windows; the printed ratios)
TEETH = 30.0         # a defect must miss the bound by at least this factor
TILE = 64  # keys per online-softmax tile of attn_kernel / attn_gp_kernel
DEFECTS = ("mask_last", "pad_zero", "no_rescale", "flush", "swap_rel")
STRESSES = ("benign", "large", "late_max", "subnormal_mass", "pad_heavy")


def lg(r):
    return f"2^{math.log2(r):.2f}" if r > 0 else "0"


class Geo:
    """One lmx_attn_desc problem: B items (batch elements | windows), H heads, Tq queries and Tk keys per item, head dim hd.
    window = None (flat) or dict(Gh, Gw, ws, q_stride)."""

    def __init__(self, B, H, Tq, Tk, hd, window=None):
        self.B, self.H, self.Tq, self.Tk, self.hd = B, H, Tq, Tk, hd
        self.scale = hd ** -0.5
        self.window = window
        if window is not None:
            self.Gh, self.Gw, self.ws = window["Gh"], window["Gw"], window["ws"]
            self.qs = window.get("q_stride", 1)
            self.nWy, self.nWx = -(-self.Gh // self.ws), -(-self.Gw // self.ws)
            self.wsq = self.ws // self.qs
            self.Gqh, self.Gqw = self.Gh // self.qs, self.Gw // self.qs
            self.n = B // (self.nWy * self.nWx)
            assert self.n * self.nWy * self.nWx == B and Tk == self.ws ** 2 and Tq == self.wsq ** 2

    @property
    def q_rows(self):
        return self.B * self.Tq if self.window is None else self.n * self.Gqh * self.Gqw

    @property
    def k_rows(self):
        return self.B * self.Tk if self.window is None else self.n * self.Gh * self.Gw

    def locate(self, r):
        """Output (= query) row -> (item b, query t)."""
        if self.window is None:
            return r // self.Tq, r % self.Tq
        img, rem = divmod(r, self.Gqh * self.Gqw)
        y, x = divmod(rem, self.Gqw)
        b = (img * self.nWy + y // self.wsq) * self.nWx + x // self.wsq
        return b, (y % self.wsq) * self.wsq + x % self.wsq

    def key_rows(self, b):
        """Token rows of item b's keys, -1 for keys in the padding."""
        t = torch.arange(self.Tk)
        if self.window is None:
            return b * self.Tk + t
        nW = self.nWy * self.nWx
        img, w = divmod(b, nW)
        wy, wx = divmod(w, self.nWx)
        y, x = wy * self.ws + t // self.ws, wx * self.ws + t % self.ws
        ok = (y < self.Gh) & (x < self.Gw)
        return torch.where(ok, (img * self.Gh + y) * self.Gw + x, torch.full_like(t, -1))


def rows_sample(M, step=97, edge=64):
    """Every row in the first and last `edge`, plus every `step`-th."""
    idx = set(range(0, M, step)) | set(range(min(edge, M))) | set(range(max(0, M - edge), M))
    return torch.tensor(sorted(idx), dtype=torch.long)


def _f16(x):
    return x.float().half().double()


def _items(geo, rows):
    """Sampled output rows grouped by item: [(b, positions in `rows`, query indices t)]."""
    groups = {}
    for i, r in enumerate(rows.tolist()):
        b, t = geo.locate(r)
        groups.setdefault(b, ([], []))
        groups[b][0].append(i)
        groups[b][1].append(t)
    return [(b, torch.tensor(p), torch.tensor(t)) for b, (p, t) in sorted(groups.items())]


def _operands(geo, q, k, v, pad_k, pad_v, b, rows, ts):
    """float64 Q [m, H, hd] of the item's sampled queries, K / V [Tk, H, hd] with padded keys replaced."""
    H, hd = geo.H, geo.hd
    kr = geo.key_rows(b)
    pad = kr < 0
    K = q.new_zeros((geo.Tk, H * hd), dtype=torch.float64)
    V = K.clone()
    K[~pad] = k[kr[~pad]].double()
    V[~pad] = v[kr[~pad]].double()
    if pad.any():
        K[pad] = pad_k.double() if pad_k is not None else 0.0
        V[pad] = pad_v.double() if pad_v is not None else 0.0
    Q = q[rows].double()
    return Q.view(-1, H, hd), K.view(-1, H, hd), V.view(-1, H, hd)


def _rel_tables(geo, Q, ts, rel, f16, swap=False):
    """Per-query decomposed bias [m, H, Tk] and its |table| / sum |q||R| terms: rel[t][j] = q . Rh[ty - j + S - 1] (rows) and
    q . Rw[tx - j + S - 1] (columns).  f16: R and the tables rounded to f16 as lmx_k_relpos_tables does."""
    Rh, Rw = (torch.as_tensor(r).double() for r in rel)
    if f16:
        Rh, Rw = _f16(Rh), _f16(Rw)
    S = (Rh.shape[0] + 1) // 2
    ty, tx = ts // S, ts % S
    j = torch.arange(S)
    Gh_ = Rh[ty[:, None] - j[None, :] + S - 1]  # [m, S, hd]
    Gw_ = Rw[tx[:, None] - j[None, :] + S - 1]
    th = torch.einsum("mhc,mjc->mhj", Q, Gh_)
    tw = torch.einsum("mhc,mjc->mhj", Q, Gw_)
    ah = torch.einsum("mhc,mjc->mhj", Q.abs(), Gh_.abs())
    aw = torch.einsum("mhc,mjc->mhj", Q.abs(), Gw_.abs())
    if f16:
        th, tw = _f16(th), _f16(tw)
    if swap:
        th, tw = tw, th
    t = torch.arange(geo.Tk)
    ky, kx = t // S, t % S
    bias = th[:, :, ky] + tw[:, :, kx]
    err = th.abs()[:, :, ky] + tw.abs()[:, :, kx] + ah[:, :, ky] + aw[:, :, kx]
    return bias, err


def reference(q, k, v, geo, pad_k=None, pad_v=None, rel=None, rows=None):
    """float64 attention on the sampled output rows -> (ref [n, H*hd], p [n, H, Tk], L [n, H], aux) with aux['den'] the bound's
    parenthesis [n, H*hd] (multiply by C) and aux['s'] the scores [n, H, Tk] in natural units.
    q / k / v: the f16 values as CPU tensors [rows, H*hd]; pad_k / pad_v [H*hd] or None; rel = (Rh, Rw) [2S-1, hd] or None."""
    rows = rows_sample(geo.q_rows) if rows is None else rows
    n, H, hd, Tk = len(rows), geo.H, geo.hd, geo.Tk
    ref = torch.empty((n, H, hd), dtype=torch.float64)
    den = torch.empty_like(ref)
    P = torch.empty((n, H, Tk), dtype=torch.float64)
    S_ = torch.empty_like(P)
    Ls = torch.empty((n, H), dtype=torch.float64)
    for b, pos, ts in _items(geo, rows):
        Q, K, V = _operands(geo, q, k, v, pad_k, pad_v, b, rows[pos], ts)
        s = geo.scale * torch.einsum("mhd,khd->mhk", Q, K)
        E = 2.0 ** -10 * geo.scale * torch.einsum("mhd,khd->mhk", Q.abs(), K.abs())
        if rel is not None:
            bias, berr = _rel_tables(geo, Q, ts, rel, f16=False)
            s = s + bias
            E = E + berr
        mx = s.max(-1, keepdim=True).values
        e = torch.exp(s - mx)
        L = e.sum(-1)
        p = e / L[..., None]
        Va = V.abs()
        ref[pos] = torch.einsum("mhk,khd->mhd", p, V)
        den[pos] = (ref[pos].abs() + torch.einsum("mhk,khd->mhd", p * (1 + E), Va)
                    + 2.0 ** -14 * Va.sum(0)[None] / L[..., None])
        P[pos], S_[pos], Ls[pos] = p, s, L
    return ref.view(n, H * hd), P, Ls, dict(den=den.view(n, H * hd), s=S_, rows=rows)


def f16_model(q, k, v, geo, pad_k=None, pad_v=None, rel=None, rows=None, defect=None):
    """The kernels' arithmetic in float64 with their f16 rounding points: 64-key tiles with a running maximum, P = exp(s - m)
    rounded to f16 (subnormals included), the normaliser the sum of the rounded P (ones column / fdot2), O and L rescaled when
    the maximum grows, the output O / L rounded to f16; rel-pos tables from f16 R, rounded to f16.
    defect: None or one of DEFECTS — a model of a kernel bug the bound must catch:
      mask_last   the last valid key masked (>= Tk - 1)          pad_zero  padded window keys read as zeros
      no_rescale  O and L not rescaled when the maximum grows    flush     f16-subnormal P flushed to zero
      swap_rel    rel-pos bias_h / bias_w swapped"""
    assert defect is None or defect in DEFECTS, defect
    rows = rows_sample(geo.q_rows) if rows is None else rows
    n, H, hd, Tk = len(rows), geo.H, geo.hd, geo.Tk
    out = torch.empty((n, H, hd), dtype=torch.float64)
    for b, pos, ts in _items(geo, rows):
        if defect == "pad_zero":
            Q, K, V = _operands(geo, q, k, v, None, None, b, rows[pos], ts)
        else:
            Q, K, V = _operands(geo, q, k, v, pad_k, pad_v, b, rows[pos], ts)
        s = geo.scale * torch.einsum("mhd,khd->mhk", Q, K)
        if rel is not None:
            s = s + _rel_tables(geo, Q, ts, rel, f16=True, swap=defect == "swap_rel")[0]
        if defect == "mask_last":
            s[..., Tk - 1] = -math.inf
        m = torch.full(s.shape[:2], -math.inf, dtype=torch.float64)
        L = torch.zeros_like(m)
        O = torch.zeros((len(pos), H, hd), dtype=torch.float64)
        for t0 in range(0, Tk, TILE):
            st = s[..., t0:t0 + TILE]
            m_new = torch.maximum(m, st.max(-1).values)
            alpha = torch.exp(m - m_new)
            if defect == "no_rescale":
                alpha = torch.ones_like(alpha)
            Pt = _f16(torch.exp(st - m_new[..., None]))
            if defect == "flush":
                Pt = torch.where(Pt < 2.0 ** -14, torch.zeros_like(Pt), Pt)
            L = L * alpha + Pt.sum(-1)
            O = O * alpha[..., None] + torch.einsum("mhk,khd->mhd", Pt, V[t0:t0 + TILE])
            m = m_new
        out[pos] = _f16(O / L[..., None])
    return out.view(n, H * hd)


def ratio(got, ref, den):
    """max |got - ref| / den over the sampled elements (the bound holds for C >= this)."""
    err = (torch.as_tensor(got).double().cpu() - ref).abs()
    return float((err / den).max())


# ------------------------------------------------------------------------------------------------ stress inputs
def _last_valid(geo, b):
    kr = geo.key_rows(b)
    return int(kr[(kr >= 0).nonzero().max()])


def make_inputs(kind, geo, seed, rel_S=None):
    """f16 q [q_rows, H*hd], k / v [k_rows, H*hd], pad_k / pad_v [H*hd] (window geometry) and rel = (Rh, Rw) f32 [2S-1, hd]
    (rel_S given) for one stress pattern (STRESSES):
      benign          q, k, v ~ N(0, 1.5^2): scores within about +-9
      large           scores with a standard deviation of 40 natural units: exp without the max subtraction overflows
      late_max        the last valid key of every item scores ~12, several units above every earlier key (lazy rescale,
                      ragged-tile mask)
      subnormal_mass  one dominant key (the item's first, V = 0) and every other key at p / p_max in [2^-16, 2^-14.2), the f16
                      subnormal range, with V ~ 1
      pad_heavy       (windows) pad_k aligned with the queries: padded keys dominate the padded windows"""
    assert kind in STRESSES, kind
    g = np.random.default_rng(seed)
    H, hd = geo.H, geo.hd
    D = H * hd
    win = geo.window is not None
    assert kind != "pad_heavy" or win

    def rn(*shape):
        return torch.from_numpy(g.standard_normal(shape))

    e = rn(H, hd)
    e = e / e.norm(dim=1, keepdim=True)  # one unit direction per head
    E = e.reshape(D)
    q, k, v = rn(geo.q_rows, D), rn(geo.k_rows, D), rn(geo.k_rows, D)
    pk, pv = rn(D), rn(D)
    if kind == "benign":
        q, k, v = q * 1.5, k * 1.5, v * 1.5
    elif kind == "large":
        a = 40.0 ** 0.5
        q, k, pk = q * a, k * a, pk * a
    elif kind in ("late_max", "pad_heavy"):
        # q = 0.7 N(0, 1) (orthogonal to e_h) + (3 + 0.3 N(0, 1)) e_h: a key c e_h scores 3 c scale +- 10 %
        along = 3 + 0.3 * rn(geo.q_rows, H, 1)
        qn = q.view(geo.q_rows, H, hd)
        qn = qn - (qn * e[None]).sum(-1, keepdim=True) * e[None]  # the noise orthogonal to e_h
        q = (0.7 * qn + along * e[None]).reshape(geo.q_rows, D)
        if kind == "late_max":
            c = 4.0 / geo.scale
            for b in range(geo.B):
                k[_last_valid(geo, b)] = c * E
        else:
            pk = (3.0 / geo.scale) * E
            pv = 2 + 0.5 * pv
    elif kind == "subnormal_mass":
        a = 2.0 * hd ** 0.5  # q = a e_h (+ noise): score of k = (t / 2) e_h is t
        q = a * (e[None].expand(geo.q_rows, H, hd)).reshape(geo.q_rows, D) + 0.01 * q
        t = math.log(2) * torch.from_numpy(g.uniform(-16.0, -14.2, (geo.k_rows, H, 1)))
        k = (t / 2 * e[None]).reshape(geo.k_rows, D) + 0.01 * k
        v = 1 + 0.5 * v
        for b in range(geo.B):
            kr = geo.key_rows(b)
            first = int(kr[(kr >= 0).nonzero().min()])
            k[first] = 0.01 * rn(D)
            v[first] = 0
        pk = (math.log(2) * -15.0 / 2) * E + 0.01 * pk
        pv = 1 + 0.5 * pv
    out = dict(q=q.half(), k=k.half(), v=v.half(), pad_k=pk.half() if win else None, pad_v=pv.half() if win else None, rel=None)
    if rel_S:
        out["rel"] = tuple((torch.from_numpy(g.standard_normal((2 * rel_S - 1, hd))) * 0.3).float() for _ in range(2))
    return out


def evaluate(inp, geo, got=None, defect=None, rows=None, pads=True):
    """ratio of `got` (the kernel's output at the sampled rows) or of the f16 model (with `defect`) against the reference of
    `inp`; -> (ratio, reference tuple)."""
    pk, pv = (inp["pad_k"], inp["pad_v"]) if pads else (None, None)
    r = reference(inp["q"], inp["k"], inp["v"], geo, pk, pv, inp["rel"], rows)
    if got is None:
        got = f16_model(inp["q"], inp["k"], inp["v"], geo, inp["pad_k"], inp["pad_v"], inp["rel"], r[3]["rows"], defect)
    return ratio(got, r[0], r[3]["den"]), r
