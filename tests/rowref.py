"""Float64 references, per-element error bounds, stress inputs and modelled defects of the HBM-bound kernels: csrc/norm.hip
(layernorm, assemble_tokens, token_mean, rope) and the YOLO glue of csrc/yolo.hip (stem_conv, maxpool5, upsample2,
detect_decode, scale_boxes).  Written from the documented semantics (include/lmx.h, the kernel comments) and shared by
tests/test_row_ref_host.py (CPU) and tests/test_gpu_rowwise.py (GPU).

Every reference takes the values the device sees (f16 operands already rounded, as float64) and does its arithmetic in float64.
Every `*_f32` function is the same formula in float32, in the kernel's documented order: the host test holds it to half of the
bound, the GPU test holds the kernel to the whole bound.  u = 2^-24 is the f32 unit roundoff.

layernorm, f32 output, with mu, rstd, ref in float64:
    |got - ref| <= C_LN u ( |ref| + |g_c| rstd ( |x_c - mu| + max_j |x_j| ) )
(the error of the mean is u max|x|-sized and reaches the output through g rstd).  An f16 output adds half an f16 ulp of ref; GELU
multiplies the bound by max(1, |gelu'(ref)|) and adds 2 u |gelu(ref)|.
token_mean     u sum_t |x_t| + u |ref|                       (sequential f32 sum, one division)
rope           half an f16 ulp of ref + 3 u (|a cos| + |b sin|)          (f16 outputs: the restatement is held to half of the
stem_conv      half an f16 ulp of ref + max(1, |silu'|) 28 u (sum_t |x_t w_t| + |bias|)    float32 part, see excess())
detect_decode  boxes: stride u K_BOX (|anchor| + 15); scores: 2 u K_SIG
maxpool5, upsample2 and assemble_tokens (one f32 add) are bit-exact; scale_boxes is within one f32 ulp."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
# The float32 restatement reaches 2.03 of the unit bound (test_row_ref_host.py prints it, D = 448 on bigmean); the margin is for
# FMA contraction and the reduction orders of the narrow and rows kernels.  Measured on MI355X (test_gpu_rowwise.py prints them):
# 2.40 at most (the rows kernel, 24581 x 448 on mixed); 2.03 for the one-row kernels (ITERS 2, f32 in), 1.93 for the narrow one;
# f16 inputs stay below 1.3.  All under C_LN / 2.
C_LN = 8.0
TEETH = 10.0  # a defect must miss its kernel's bound by at least this factor
# 4x the largest ratio that the float32 restatement of detect_decode reaches on DETECT_CASES: boxes 5.43, scores 0.746 (the host
# test recomputes both and holds them to K / 2).  They cover expf's few ulps through the 16-term softmax.  Measured on MI355X:
# boxes 4.93, scores 0.746.
K_BOX = 22.0
K_SIG = 3.0

STRESSES = ("benign", "bigmean", "small", "mixed")
LN_DEFECTS = ("unbiased", "eps_outside", "drop_tail", "one_pass_f32", "row_shift", "gelu_tanh")
DEFECTS = LN_DEFECTS + ("rope_no_neg", "rope_prefix", "decode_anchor0", "stem_pad_clamp")
DEFECT_STRESS = {d: "benign" for d in DEFECTS}
DEFECT_STRESS.update(eps_outside="small", one_pass_f32="bigmean")

# detect_decode problems of the GPU test: (n, H, W, nc, ldh, logit scale).  Scale 8 lets one bin dominate; at 40 the other
# bins' exp underflows to zero in float32.  The 80 x 79 level has n H W 4 = 530 880 lanes, no multiple of 256.
DETECT_CASES = [
    (2, 6, 10, 80, 148, 2.0),
    (2, 5, 7, 3, 72, 8.0),
    (3, 4, 4, 1, 68, 40.0),
    (21, 80, 80, 3, 68, 8.0),
    (21, 80, 79, 3, 72, 8.0),
]


def fmt(r):
    return f"{r:.3g}"


def half_ulp16(ref):
    """Half an f16 ulp of |ref|: 2^-25 below the normal range."""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -14))  # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e - 12)


def seen(x, dtype):
    """The float64 values a kernel reads from a tensor of `dtype`."""
    return x.to(dtype).double()


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf for a NaN."""
    r = (torch.as_tensor(got).double().cpu() - ref).abs() / bound
    return math.inf if bool(torch.isnan(r).any()) else float(r.max())


def excess(got, ref, rnd, e):
    """max (|got - ref| - rnd) / e: the share of the float32 part `e` of a bound rnd + e that is used once the f16 rounding of
    the output, rnd, is taken off (a correctly rounded result alone uses up to all of rnd)."""
    r = ((torch.as_tensor(got).double().cpu() - ref).abs() - rnd).clamp_min(0) / e
    return math.inf if bool(torch.isnan(r).any()) else float(r.max())


def _rng(seed):
    return np.random.default_rng(seed)


def _rn(g, *shape):
    return torch.from_numpy(g.standard_normal(shape))


# ------------------------------------------------------------------------------------------------ stress inputs
def stress_rows(kind, rows, D, seed):
    """float64 [rows, D], every row distinct (STRESSES):
      benign   3 N + 0.5
      bigmean  0.5 N + 50: a mean 100x the spread (one-pass variance cancels)
      small    3e-3 N + 0.01: variance about 1e-5, the size of eps
      mixed    rows alternating between the three: neighbouring rows of one wave differ by orders of magnitude"""
    assert kind in STRESSES, kind
    n = _rn(_rng(seed), rows, D)
    fam = {"benign": 3 * n + 0.5, "bigmean": 0.5 * n + 50, "small": 3e-3 * n + 0.01}
    if kind != "mixed":
        return fam[kind]
    sel = (torch.arange(rows) % 3)[:, None]
    return torch.where(sel == 0, fam["benign"], torch.where(sel == 1, fam["bigmean"], fam["small"]))


def affine(D, seed):
    """gamma ~ 1 + 0.3 N, beta ~ 0.2 N as f32 [D]."""
    g = _rng(seed)
    return (1 + 0.3 * _rn(g, D)).float(), (0.2 * _rn(g, D)).float()


# ------------------------------------------------------------------------------------------------ layernorm
def gelu(y, tanh=False):
    if tanh:
        return 0.5 * y * (1 + torch.tanh(math.sqrt(2 / math.pi) * (y + 0.044715 * y ** 3)))
    return 0.5 * y * (1 + torch.erf(y / math.sqrt(2)))


def gelu_grad(y):
    return 0.5 * (1 + torch.erf(y / math.sqrt(2))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)


def layernorm(x, gamma, beta, eps, act=False, defect=None):
    """x float64 [R, D], gamma / beta [D] -> (ref, unit): biased variance, eps inside the square root, then erf-GELU if `act`;
    unit [R, D] is the parenthesis of the bound before the GELU.  defect: None or one of LN_DEFECTS, a model of a kernel bug:
      unbiased      variance divided by D - 1            eps_outside  1 / (sqrt(var) + eps)
      drop_tail     the last float4 group of the row left out of both sums
      one_pass_f32  E[x^2] - mu^2 evaluated in float32   row_shift    row r normalised with row r + 1's statistics
      gelu_tanh     the tanh form instead of erf"""
    assert defect is None or defect in LN_DEFECTS, defect
    D = x.shape[1]
    g, b = gamma.double(), beta.double()
    n = D - 4 if defect == "drop_tail" else D
    mu = x[:, :n].sum(1, keepdim=True) / D
    var = ((x - mu)[:, :n] ** 2).sum(1, keepdim=True) / D
    if defect == "unbiased":
        var = var * D / (D - 1)
    if defect == "one_pass_f32":
        x32 = x.float()
        m32 = x32.sum(1, keepdim=True) / D
        mu, var = m32.double(), ((x32 * x32).sum(1, keepdim=True) / D - m32 * m32).double().clamp_min(0)
    rstd = 1 / (var.sqrt() + eps) if defect == "eps_outside" else 1 / (var + eps).sqrt()
    if defect == "row_shift":
        mu, rstd = mu.roll(-1, 0), rstd.roll(-1, 0)
    y = (x - mu) * rstd * g + b
    unit = y.abs() + g.abs() * rstd * ((x - mu).abs() + x.abs().max(1, keepdim=True).values)
    return (gelu(y, tanh=defect == "gelu_tanh") if act else y), (unit, y)


def ln_bound(ref, aux, act, f16_out):
    unit, pre = aux
    e = C_LN * U32 * unit
    if act:
        e = e * gelu_grad(pre).abs().clamp_min(1.0) + 2 * U32 * ref.abs()
    return e + half_ulp16(ref) if f16_out else e


def ln_unit_ratio(got, ref, aux, act, f16_out):
    """The C_LN that `got` needs: its error, less the output rounding and the GELU's own 2 u |ref|, in units of the bound's
    parenthesis (times the GELU slope)."""
    unit, pre = aux
    err = (torch.as_tensor(got).double().cpu() - ref).abs()
    e = U32 * unit
    if act:
        err, e = err - 2 * U32 * ref.abs(), e * gelu_grad(pre).abs().clamp_min(1.0)
    if f16_out:
        err = err - half_ulp16(ref)
    return float((err.clamp_min(0) / e).max())


def layernorm_f32(x, gamma, beta, eps, act=False, lanes=None):
    """float32 in the kernels' order: a float4 per lane and step, (v0 + v1) + (v2 + v3) partials accumulated per lane, a
    `lanes`-wide xor butterfly (64; 32 for the narrow kernel, D <= 128), the variance from the centred values (two passes over the
    registers), 1 / sqrt(var + eps), (x - mean) rstd g + b.  x f32 [R, D] -> f32 [R, D]."""
    R, D = x.shape
    lanes = lanes or (32 if D <= 128 else 64)
    iters = -(-D // (lanes * 4))
    pad = iters * lanes * 4
    valid = (torch.arange(pad) < D).view(iters, lanes, 4)
    xp = torch.zeros((R, pad), dtype=torch.float32)
    xp[:, :D] = x
    v = xp.view(R, iters, lanes, 4)
    idx = torch.arange(lanes)

    def reduce(t):  # t [R, iters, lanes, 4] -> [R, 1]
        s = torch.zeros((R, lanes), dtype=torch.float32)
        for i in range(iters):
            s = s + ((t[:, i, :, 0] + t[:, i, :, 1]) + (t[:, i, :, 2] + t[:, i, :, 3]))
        o = lanes // 2
        while o:
            s = s + s[:, idx ^ o]
            o //= 2
        return s[:, :1]

    Df = torch.tensor(float(D), dtype=torch.float32)
    mean = reduce(v) / Df
    dl = torch.where(valid, v - mean[:, :, None, None], torch.zeros((), dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(reduce(dl * dl) / Df + torch.tensor(eps, dtype=torch.float32))
    o = (x - mean) * rstd * gamma + beta
    if act:
        o = 0.5 * o * (1.0 + torch.erf(o * torch.tensor(0.70710678118654752440, dtype=torch.float32)))
    assert o.dtype == torch.float32
    return o


# ------------------------------------------------------------------------------------------------ tokens
def assemble_tokens(patch, prefix, pos, B, np_, n_prefix, D):
    """patch f16 [B * np, D], prefix f32 [n_prefix, D] | None, pos f32 [np + n_prefix, D] | None -> f32 [B * T, D]: the prefix
    rows then the patches, plus the position row.  One f32 add, so the float64 sum rounded to f32 is what the kernel owes."""
    rows = patch.double().view(B, np_, D)
    if n_prefix:
        rows = torch.cat((prefix.double()[None].expand(B, n_prefix, D), rows), 1)
    if pos is not None:
        rows = rows + pos.double()[None]
    return rows.reshape(B * (np_ + n_prefix), D).float()


def token_mean(x, B, T, D):
    """x float64 [B * T, D] -> (ref [B, D], bound)."""
    x = x.view(B, T, D)
    ref = x.mean(1)
    return ref, U32 * x.abs().sum(1) + U32 * ref.abs()


def token_mean_f32(x, B, T, D):
    x = x.view(B, T, D)
    acc = torch.zeros((B, D), dtype=torch.float32)
    for t in range(T):
        acc = acc + x[:, t]
    return acc / torch.tensor(float(T), dtype=torch.float32)


def rope_inputs(B, T, H, hd, n_prefix, seed):
    """f16 qkv [B * T, 3 H hd] ~ 1.5 N and f32 cos / sin [T - n_prefix, hd] of independent angles per (token, d), so that a low
    half read with the high half's table shows."""
    g = _rng(seed)
    th = torch.from_numpy(g.uniform(-math.pi, math.pi, (T - n_prefix, hd)))
    return (1.5 * _rn(g, B * T, 3 * H * hd)).half(), th.cos().float(), th.sin().float()


def _rope_parts(x, B, T, H, hd, n_prefix, cos_t, sin_t, defect):
    h2 = hd // 2
    x = x.double().view(B, T, H, hd)
    c = torch.ones((T, hd), dtype=torch.float64)
    s = torch.zeros((T, hd), dtype=torch.float64)
    c[n_prefix:], s[n_prefix:] = cos_t.double(), sin_t.double()
    if defect == "rope_prefix" and n_prefix:  # the prefix rotated with the first patches' angles
        c[:n_prefix], s[:n_prefix] = cos_t.double()[:n_prefix], sin_t.double()[:n_prefix]
    sign = 1.0 if defect == "rope_no_neg" else -1.0
    rot = torch.cat((sign * x[..., h2:], x[..., :h2]), -1)  # rotate_half(x) = cat(-x2, x1)
    return x * c[None, :, None, :], rot * s[None, :, None, :]


def rope(x, B, T, H, hd, n_prefix, cos_t, sin_t, defect=None):
    """x f16 [B * T, H hd] -> (ref float64 [B * T, H hd], rnd, e) with the bound rnd + e: x cos + rotate_half(x) sin on the patch tokens, the prefix
    tokens unchanged (their bound is that of cos = 1, sin = 0; the GPU test also wants them bit-equal)."""
    a, b = _rope_parts(x, B, T, H, hd, n_prefix, cos_t, sin_t, None)
    ref = (a + b).reshape(B * T, H * hd)
    rnd, e = half_ulp16(ref), 3 * U32 * (a.abs() + b.abs()).reshape(B * T, H * hd)
    if defect is not None:
        a, b = _rope_parts(x, B, T, H, hd, n_prefix, cos_t, sin_t, defect)
        ref = (a + b).reshape(B * T, H * hd)
    return ref, rnd, e


def rope_f32(x, B, T, H, hd, n_prefix, cos_t, sin_t):
    h2 = hd // 2
    x = x.float().view(B, T, H, hd).clone()
    p = x[:, n_prefix:]
    c, s = cos_t[None, :, None, :], sin_t[None, :, None, :]
    lo = p[..., :h2] * c[..., :h2] - p[..., h2:] * s[..., :h2]
    hi = p[..., h2:] * c[..., h2:] + p[..., :h2] * s[..., h2:]
    x[:, n_prefix:] = torch.cat((lo, hi), -1)
    return x.reshape(B * T, H * hd).half()


# ------------------------------------------------------------------------------------------------ YOLO glue
def stem_inputs(n, H, W, Cout, seed):
    """u8 [n, H, W, 3] with 0 and 255 alternating along the borders, w f32 [3][3][3][Cout] (ky, kx, c, Cout) ~ 0.3 N, bias 0.1 N."""
    g = _rng(seed)
    img = torch.from_numpy(g.integers(0, 256, (n, H, W, 3), dtype=np.uint8))
    edge = ((torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 * 255).to(torch.uint8)
    border = torch.ones((H, W), dtype=torch.bool)
    border[1:H - 1, 1:W - 1] = False
    img = torch.where(border[None, :, :, None], edge[None, :, :, None], img)
    return img, (0.3 * _rn(g, 3, 3, 3, Cout)).float(), (0.1 * _rn(g, Cout)).float()


def _stem_cols(img, clamp):
    """The 27 taps (ky, kx, c) of the k3 s2 p1 window as float64 [n, Ho, Wo, 27] of u8 / 255; outside the frame zero (or, with
    `clamp`, the nearest pixel)."""
    n, H, W, _ = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = img.double() / 255
    oy, ox = torch.arange(Ho) * 2 - 1, torch.arange(Wo) * 2 - 1
    cols = []
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy + ky, ox + kx
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            t = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            cols.append(t if clamp else t * ok[None, :, :, None])
    return torch.cat(cols, -1)


def stem_conv(img, w, bias, defect=None):
    """-> (ref float64 [n, Ho, Wo, Cout], rnd, e) with the bound rnd + e: silu(bias + sum x w), x = u8 / 255, zero padding."""
    assert defect in (None, "stem_pad_clamp")
    wd, bd = w.double().view(27, -1), bias.double()
    cols = _stem_cols(img, False)
    acc = cols @ wd + bd
    sg = torch.sigmoid(acc)
    ref = acc * sg
    grad = sg * (1 + acc * (1 - sg))
    rnd, e = half_ulp16(ref), grad.abs().clamp_min(1.0) * 28 * U32 * (cols @ wd.abs() + bd.abs())
    if defect is not None:
        acc = _stem_cols(img, True) @ wd + bd
        ref = acc * torch.sigmoid(acc)
    return ref, rnd, e


def stem_conv_f32(img, w, bias):
    n, H, W, _ = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = img.float() / torch.tensor(255.0, dtype=torch.float32)
    acc = bias[None, None, None, :].expand(n, Ho, Wo, -1).clone()
    oy, ox = torch.arange(Ho) * 2 - 1, torch.arange(Wo) * 2 - 1
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy + ky, ox + kx
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            t = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)] * ok[None, :, :, None]
            for c in range(3):
                acc = acc + t[..., c:c + 1] * w[ky, kx, c]
    return (acc / (1.0 + torch.exp(-acc))).half()


def pool_inputs(n, H, W, C, seed):
    """f16 [n, H, W, C] ~ 3 N with -65504, +0 and -0 sprinkled in and, where it fits, a 9 x 9 block of -65504 (its centre window
    holds nothing but the identity element of the max)."""
    g = _rng(seed)
    x = (3 * _rn(g, n, H, W, C)).half()
    k = torch.from_numpy(g.integers(0, 16, (n, H, W, C)))
    x[k == 0] = -65504.0
    x[k == 1] = 0.0
    x[k == 2] = -0.0
    x.view(-1)[:3] = torch.tensor([-65504.0, 0.0, -0.0], dtype=torch.float16)
    if H >= 9 and W >= 9:
        x[:, :9, W - 9:, :] = -65504.0
    return x


def maxpool5(x):
    """max_pool2d(k 5, s 1, p 2) of f16 [n, H, W, C]: the maximum over the taps inside the grid."""
    n, H, W, C = x.shape
    p = torch.full((n, H + 4, W + 4, C), -math.inf, dtype=torch.float64)
    p[:, 2:H + 2, 2:W + 2] = x.double()
    out = p[:, 2:H + 2, 2:W + 2].clone()
    for dy in range(5):
        for dx in range(5):
            out = torch.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out.half()


def upsample2(x):
    """nearest x2: out[y][x] = in[y >> 1][x >> 1]."""
    H, W = x.shape[1:3]
    return x[:, torch.arange(2 * H) // 2][:, :, torch.arange(2 * W) // 2]


def detect_inputs(n, H, W, nc, ldh, scale, seed):
    """head f32 [n, H, W, ldh] ~ scale N: 64 box logits (side 16 + bin), nc class logits, then columns the kernel must skip."""
    return (scale * _rn(_rng(seed), n, H, W, ldh)).float()


def _anchors(H, W, dt, off):
    gy, gx = torch.meshgrid(torch.arange(H, dtype=dt) + off, torch.arange(W, dtype=dt) + off, indexing="ij")
    return torch.stack((gx, gy), -1).view(1, H * W, 2)


def _detect(head, nc, stride, dt, anchor0=False):
    n, H, W, _ = head.shape
    h = head.to(dt)
    box = h[..., :64].reshape(n, H * W, 4, 16)
    e = torch.exp(box - box.max(-1, keepdim=True).values)
    dist = ((e / e.sum(-1, keepdim=True)) * torch.arange(16, dtype=dt)).sum(-1)
    a = _anchors(H, W, dt, 0.0 if anchor0 else 0.5)
    x1y1, x2y2 = a - dist[..., :2], a + dist[..., 2:]
    st = torch.tensor(stride, dtype=dt)
    sc = 1 / (1 + torch.exp(-h[..., 64:64 + nc].reshape(n, H * W, nc)))
    return torch.cat(((x1y1 + x2y2) / 2 * st, (x2y2 - x1y1) * st, sc), -1)


def detect_decode(head, nc, stride, defect=None):
    """-> (ref float64 [n, H W, 4 + nc], bound): dist = sum_k k softmax(16 bins)_k per side (l, t, r, b); the anchor is the cell
    centre (x + 0.5, y + 0.5); xywh = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1) stride; the scores are sigmoids."""
    assert defect in (None, "decode_anchor0")
    ref = _detect(head, nc, stride, torch.float64, defect is not None)
    a = _anchors(head.shape[1], head.shape[2], torch.float64, 0.5)
    bound = torch.empty_like(ref)
    bound[..., :4] = stride * U32 * K_BOX * (torch.cat((a, a), -1) + 15)
    bound[..., 4:] = 2 * U32 * K_SIG
    return ref, bound


def detect_decode_f32(head, nc, stride):
    return _detect(head, nc, stride, torch.float32)


def box_inputs(total, seed, padx, pady, gain, w, h):
    """f32 xyxy [total, 4] in letterbox pixels that straddle every clip edge: corners from 40 px outside the frame's image to 40
    px inside, on each side."""
    g = _rng(seed)
    lo = torch.tensor([padx, pady, padx, pady])
    hi = lo + gain * torch.tensor([w, h, w, h])
    side = torch.from_numpy(g.integers(0, 2, (total, 4))).bool()
    return (torch.where(side, hi, lo) + torch.from_numpy(g.uniform(-40.0, 40.0, (total, 4)))).float()


def scale_boxes(boxes, padx, pady, gain, w, h):
    """(xyxy - pad) / gain clipped to [0, w] x [0, h], from the f32 arguments the kernel receives -> (the float64 result rounded to
    f32, the same in float32 arithmetic with an IEEE division)."""
    f = [torch.tensor(v, dtype=torch.float32) for v in (padx, pady, gain, w, h)]
    out = []
    for dt in (torch.float64, torch.float32):
        px, py, gn, ww, hh = (v.to(dt) for v in f)
        b = (boxes.to(dt) - torch.stack((px, py, px, py))) / gn
        out.append(torch.minimum(b.clamp_min(0), torch.stack((ww, hh, ww, hh))).float())
    return out


def ulps32(a, b):
    """Largest distance in f32 ulps between two f32 tensors of one sign pattern (or zeros)."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())
