"""Float64 references of the fused Hiera block kernels (csrc/hiera.hip), the walk of every persistent kernel over its work units, and
the error measure and bound the late-pass tests hold them to.  Shared by tests/test_hiera_ref_host.py (CPU) and
tests/test_gpu_persistent.py (GPU).

The three operations are written from the TF Sam2MultiScaleBlock / Sam2MultiScaleAttention definitions and evaluated PER WINDOW (or per
block of rows), with any number of leading batch dimensions, so that a test can ask for a sample of windows of a very large input:

    attn_half       x + proj(window_attention(qkv(h)))                        h given, or layer_norm1(x)
    attn_pool_half  pool(proj_sc(h)) + attn_proj(window_attention(pool(q), k, v))
    mlp_half        x + fc2(gelu(fc1(layer_norm2(x)))), and layer_norm1 of the next block on the result

Inputs are the f16-rounded weights and the f16 h the kernels get; everything else is float64 and no rounding point is modelled.

A persistent kernel is launched with one workgroup per CU (csrc/api.hip lmx_persistent_grid) and each workgroup walks several units.
"Pass" p of a workgroup is its p-th unit (0-based); in the streamed kernels matrix c — counted over ALL of the workgroup's groups —
lands in ring slot c % 4, so a group that is the workgroup's pass p starts at slot (p * images per group) % 4: its "start slot".
walk() restates that arithmetic; the images per group are read from the packed operand (lmx.sam.pack_*), not written down here."""
import math

import numpy as np
import torch

# 2 x the largest ratio() of the UNFUSED launches (LayerNorm / lmx_k_gemm / lmx_k_attention / lmx_k_maxpool2 chains, lmx_k_ln_mlp)
# against these references on the inputs and samples of tests/test_gpu_persistent.py on MI355X (256 CUs): 2^-10.75, the attn8 chain
# with its LayerNorm launch (LayerNorm -> qkv GEMM -> window attention -> projection GEMM), first group; the other chains reach
# 2^-10.86 (attnp) .. 2^-11.57 (mlp224) — profiles/persistent_passes.txt.  The factor of two is for the other f32 summation order
# of the fused kernels; their own ratios never enter this constant.
C_FUSED = 2.0 ** -9.75
TEETH = 10.0  # a defect model must miss C_FUSED by at least this factor
RING = 4      # slots of the LDS weight ring (NST4 / NSTM in csrc/hiera.hip)
SENT = -1234.0

# kernel -> geometry.  per_group: units of one workgroup pass (windows; rows for the MLP), the constants NW4 * TB4, LMX_HP_NW, NW2 * 4,
# NWM * TBM * 16 of csrc/hiera.hip.  img: the (Gh, Gw) token grid of one small image of the GPU tests — four windows, except attn8's
# six: its pass is 4 windows, and with 4 windows per image no whole number of images leaves its last pass partial.
GEOM = {
    "attn8": dict(Din=112, D=112, heads=2, ws=8, pool=False, per_group=4, img=(24, 16)),
    "attn4": dict(Din=224, D=224, heads=4, ws=4, pool=False, per_group=16, img=(8, 8)),
    "attnp": dict(Din=112, D=224, heads=4, ws=8, pool=True, per_group=8, img=(16, 16)),
    "attnq": dict(Din=224, D=448, heads=8, ws=4, pool=True, per_group=16, img=(8, 8)),
    "mlp112": dict(Din=112, D=112, per_group=384),
    "mlp224": dict(Din=224, D=224, per_group=256),
}
EPS = 1e-6
Q_GAIN = 2.0  # the q rows of wqkv are scaled by this: logits of ~2 standard deviations, so single keys carry weight


def lg(r):
    return f"2^{math.log2(r):.2f}" if r > 0 else "0"


# ------------------------------------------------------------------------------------------------ inputs
def make_params(kernel, gen, device="cpu"):
    """Seeded parameters of one block half as float32 tensors on `device` (weights already rounded to f16): wqkv / bqkv / wo / bo
    [, wsc / bsc] [, gam / bet] for the attention halves, w1 / b1 / w2 / b2 / g2 / e2 / gn / en for the MLP."""
    g = GEOM[kernel]
    Din, D = g["Din"], g["D"]

    def rn(*shape, scale=1.0):
        return torch.randn(shape, generator=gen, device=device) * scale

    def w16(t):
        return t.half().float()

    if kernel.startswith("mlp"):
        return dict(w1=w16(rn(4 * D, D) * D ** -0.5), b1=rn(4 * D, scale=0.2), w2=w16(rn(D, 4 * D) * (4 * D) ** -0.5), b2=rn(D, scale=0.2),
                    g2=1.0 + rn(D, scale=0.2), e2=rn(D, scale=0.2), gn=1.0 + rn(D, scale=0.2), en=rn(D, scale=0.2))
    wqkv = rn(3 * D, Din) * Din ** -0.5
    wqkv[:D] *= Q_GAIN
    p = dict(wqkv=w16(wqkv), bqkv=rn(3 * D, scale=0.2), wo=w16(rn(D, D) * D ** -0.5), bo=rn(D, scale=0.2))
    if g["pool"]:
        p.update(wsc=w16(rn(D, Din) * Din ** -0.5), bsc=rn(D, scale=0.2))
    if kernel == "attn8":
        p.update(gam=1.0 + rn(D, scale=0.2), bet=rn(D, scale=0.2))
    return p


def make_acts(kernel, rows, gen, device="cpu"):
    """(x f32 [rows, D] or None, h f16 [rows, Din] or None): the residual stream and the LayerNorm rows a kernel reads."""
    g = GEOM[kernel]
    x = h = None
    if not g.get("pool"):
        x = torch.randn((rows, g["D"]), generator=gen, device=device) + 0.3
    if not kernel.startswith("mlp"):
        h = torch.randn((rows, g["Din"]), generator=gen, device=device).half()
    return x, h


def f64(p):
    return {k: v.detach().cpu().double() for k, v in p.items()}


def window_rows(w, Gh, Gw, ws):
    """Token rows [len(w), ws * ws] (row-major inside the window) of windows w, numbered as the kernels do: image, then window row,
    then window column, on images of Gh x Gw tokens."""
    w = torch.as_tensor(w, dtype=torch.long).reshape(-1, 1)
    nWy, nWx = Gh // ws, Gw // ws
    img, wi = w // (nWy * nWx), w % (nWy * nWx)
    t = torch.arange(ws * ws).reshape(1, -1)
    y, x = (wi // nWx) * ws + t // ws, (wi % nWx) * ws + t % ws
    return (img * Gh + y) * Gw + x


# ------------------------------------------------------------------------------------------------ the float64 definitions
def layer_norm(x, gamma, beta, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def _qkv(h, p, heads, stale_matrix):
    """q, k, v [..., heads, T, hd] of h [..., T, Din].  stale_matrix = hh: head hh's v matrix is that of head hh - 1."""
    D = p["wqkv"].shape[0] // 3
    hd = D // heads
    w = p["wqkv"].reshape(3, heads, hd, -1)
    if stale_matrix is not None:
        assert 1 <= stale_matrix < heads
        w = w.clone()
        w[2, stale_matrix] = w[2, stale_matrix - 1]
    t = torch.einsum("...ti,shdi->s...htd", h, w) + p["bqkv"].reshape(3, heads, 1, hd)[(slice(None),) + (None,) * (h.dim() - 2)]
    return t[0], t[1], t[2]


def _attend(q, k, v, drop_key):
    """softmax(q k^T / sqrt(hd)) v over the window's keys -> [..., Tq, heads * hd].  drop_key: the window's last key is left out."""
    if drop_key:
        k, v = k[..., :-1, :], v[..., :-1, :]
    s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5
    o = torch.softmax(s, -1) @ v
    return o.transpose(-2, -3).reshape(*o.shape[:-3], o.shape[-2], -1)


def _pool(t, ws):
    """2 x 2 max pool of a window's tokens: [..., ws * ws, C] -> [..., (ws / 2) ** 2, C]."""
    C = t.shape[-1]
    return t.reshape(*t.shape[:-2], ws // 2, 2, ws // 2, 2, C).amax(dim=(-4, -2)).reshape(*t.shape[:-2], ws * ws // 4, C)


def attn_half(x, h, p, heads, ln=False, stale_matrix=None, drop_key=False):
    """x [..., T, D] + proj(window_attention(qkv(h))) for windows of T = ws * ws tokens; h [..., T, D], or with ln the LayerNorm of x
    (p['gam'], p['bet'])."""
    x = x.double()
    h = layer_norm(x, p["gam"], p["bet"]) if ln else h.double()
    q, k, v = _qkv(h, p, heads, stale_matrix)
    return x + _attend(q, k, v, drop_key) @ p["wo"].t() + p["bo"]


def attn_pool_half(h, p, heads, ws, stale_matrix=None, drop_key=False):
    """pool(proj_sc(h)) + attn_proj(window_attention(pool(q), k, v)) for h [..., ws * ws, Din] -> [..., (ws / 2) ** 2, Dout]."""
    h = h.double()
    sc = _pool(h @ p["wsc"].t() + p["bsc"], ws)
    q, k, v = _qkv(h, p, heads, stale_matrix)
    hd = q.shape[-1]
    qf = q.transpose(-2, -3).reshape(*q.shape[:-3], ws * ws, heads * hd)  # pooled on all channels at once
    qp = _pool(qf, ws)
    qp = qp.reshape(*qp.shape[:-1], heads, hd).transpose(-2, -3)
    return sc + _attend(qp, k, v, drop_key) @ p["wo"].t() + p["bo"]


def mlp_half(x, p, stale_matrix=None):
    """(x + fc2(gelu(fc1(LayerNorm(x)))), the next LayerNorm of that) for rows x [..., D].  stale_matrix = c: the 64 fc1 rows of
    step c are those of step c - 1."""
    x = x.double()
    w1 = p["w1"]
    if stale_matrix is not None:
        c = stale_matrix
        assert 1 <= c < w1.shape[0] // 64
        w1 = w1.clone()
        w1[64 * c:64 * c + 64] = w1[64 * c - 64:64 * c]
    u = layer_norm(x, p["g2"], p["e2"]) @ w1.t() + p["b1"]
    u = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    y = x + u @ p["w2"].t() + p["b2"]
    return y, layer_norm(y, p["gn"], p["en"])


def reference(kernel, x, h, p, form="h", **defect):
    """The kernel's operation on gathered windows: x / h [n, T, D] (rows for the MLP: [n, D]); form 'ln' is attn8 with the LayerNorm
    inside.  -> float64 result (the MLP: x and h_next concatenated on the last axis)."""
    g = GEOM[kernel]
    if kernel.startswith("mlp"):
        return torch.cat(mlp_half(x, p, **defect), -1)
    if g["pool"]:
        return attn_pool_half(h, p, g["heads"], g["ws"], **defect)
    return attn_half(x, h, p, g["heads"], ln=form == "ln", **defect)


def ratio(got, ref):
    """The error measure of every late-pass test: max over the elements of |got - ref| / (|ref| + max |ref row|)."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    return float(((got - ref).abs() / (ref.abs() + ref.abs().amax(-1, keepdim=True))).max())


# ------------------------------------------------------------------------------------------------ the walk
_IMAGES = {}


def images_per_group(kernel):
    """Matrices a workgroup streams per group: the leading dimension of the packed operand.  attn8 keeps its weights resident: 0."""
    if kernel in ("attn8", "attn_spp"):
        return 0
    if kernel not in _IMAGES:
        from lmx import sam

        g = GEOM[kernel]
        z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
        Din, D = g["Din"], g["D"]
        if kernel.startswith("mlp"):
            w_img = sam.pack_ln_mlp(z(4 * D, D), z(4 * D), z(D, 4 * D), z(D), z(D), z(D), z(D), z(D))[0]
        elif g["pool"]:
            w_img = sam.pack_hiera_attn_pool(z(D, Din), z(D), z(3 * D, Din), z(3 * D), z(D, D), z(D), g["heads"])[0]
        else:
            w_img = sam.pack_hiera_attn4(z(3 * D, D), z(3 * D), z(D, D), z(D), g["heads"])[0]
        _IMAGES[kernel] = int(w_img.shape[0])
    return _IMAGES[kernel]


def walk(kernel, n_units, n_cu):
    """[(workgroup, pass, start_slot)] of every unit of a launch on n_cu CUs, as the kernels count.
    Streamed kernels (attn4, attnp, attnq, mlp112, mlp224): the unit is a group, `grp = blockIdx.x; grp += gridDim.x`; the start slot is
    (pass * images per group) % 4.  attn8: the unit is a window, w = blockIdx.x * 4 + wave, w += gridDim.x * 4; weights are resident
    (slot 0).  attn_spp: the unit is a (batch, head) item; XCD x = blockIdx.x & 7 owns a contiguous range of the items and its
    workgroups stride through it; the slot is the half of the double buffer the item lands in (pass & 1)."""
    if kernel == "attn8":
        grid = min((n_units + 3) // 4, n_cu)
        return [((w // 4) % grid, (w // 4) // grid, 0) for w in range(n_units)]
    if kernel == "attn_spp":
        grid = min(n_units, n_cu)
        out = [None] * n_units
        iq, ir = n_units >> 3, n_units & 7
        for b in range(grid):
            xcd, jx = b & 7, b >> 3
            nwg = (grid + 7 - xcd) >> 3
            ibase = xcd * (iq + 1) if xcd < ir else ir * (iq + 1) + (xcd - ir) * iq
            icnt = iq + (1 if xcd < ir else 0)
            for p, li in enumerate(range(jx, icnt, nwg)):
                assert out[ibase + li] is None
                out[ibase + li] = (b, p, p & 1)
        assert all(o is not None for o in out), "attn_spp: an item no workgroup walks"
        return out
    n_img = images_per_group(kernel)
    grid = min(n_units, n_cu)
    return [(g % grid, g // grid, (g // grid) * n_img % RING) for g in range(n_units)]


def n_groups(kernel, units):
    """Groups (workgroup passes) of `units` windows / rows."""
    return -(-units // GEOM[kernel]["per_group"])


def round_up_partial(target, per_image, per_group):
    """The smallest count >= target that is whole images and leaves the last group partial."""
    n = -(-target // per_image) * per_image
    while n % per_group == 0:
        n += per_image
    return n
