"""Yardstick of the gait transformer tests (a helper, not a test): the network of include/lmx.h "The gait transformer" restated
functionally in torch — matmuls, F.layer_norm, torch.softmax, dropout as explicit keep arrays — in float32 or float64; a seeded weight
generator that emits a state_dict under the reference's key names (LayerNorm weights around 1, every bias nonzero); the cases with their
masks; and the tolerance rule of tcnref.tolerances, extended to the saliency."""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

import tcnref
from lmx import xfm

SHIPPED = xfm.XfmConfig()
TINY = xfm.XfmConfig(input_dim=5, d_model=32, n_heads=2, n_layers=1, ff=48, head=16, dropout=0.3, max_len=40)  # ragged input, FF % 64 != 0
WIDE = xfm.XfmConfig(input_dim=44, d_model=64, n_heads=2, n_layers=2, ff=128, head=32, dropout=0.1, max_len=160)  # head_dim 32, the T limit
CONFIGS = {"shipped": SHIPPED, "tiny": TINY, "wide": WIDE}
# every 16-row boundary up to the 128 steps of the 8-wave kernel, the first lengths of the 4-wave one (129 ..), the service's 125, the limits
T_BY_CONFIG = {"shipped": (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 125, 128, 129, 150), "tiny": (1, 7, 33, 40), "wide": (5, 125, 160)}
S_VALUES = (0, 2, 10)
M64 = tcnref.M64
PRED_FLOOR = tcnref.PRED_FLOOR


def state_dict(cfg, seed, with_pe=True):
    """A state_dict as `torch.save(model.state_dict())` of the reference's GaitTransformer writes it, with Xavier-sized matrices."""
    g = torch.Generator().manual_seed(seed)

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    def linear(prefix, n, k, sd):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = uniform((n, k), (6.0 / (n + k)) ** 0.5), uniform((n,), 0.2)

    def norm(prefix, sd):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = 1.0 + uniform((cfg.d_model,), 0.3), uniform((cfg.d_model,), 0.2)

    D, sd = cfg.d_model, {}
    linear("input_projection", D, cfg.input_dim, sd)
    if with_pe:
        from lmx import checkpoints

        sd["pos_encoder.pe"] = checkpoints.xfm_positional_table(cfg.max_len, D).unsqueeze(0)
    for i in range(cfg.n_layers):
        p = f"encoder_layers.{i}"
        sd[f"{p}.self_attn.in_proj_weight"], sd[f"{p}.self_attn.in_proj_bias"] = uniform((3 * D, D), (6.0 / (4 * D)) ** 0.5), uniform((3 * D,), 0.2)
        linear(f"{p}.self_attn.out_proj", D, D, sd)
        linear(f"{p}.ffn.0", cfg.ff, D, sd)
        linear(f"{p}.ffn.3", D, cfg.ff, sd)
        norm(f"{p}.norm1", sd)
        norm(f"{p}.norm2", sd)
    norm("final_norm", sd)
    linear("classifier.0", cfg.head, D, sd)
    linear("classifier.3", 1, cfg.head, sd)
    return sd


def site_shapes(cfg, T):
    """The activation each dropout site multiplies, in torch's memory order (include/lmx.h has the table)."""
    out = [(T, cfg.d_model)]
    for _ in range(cfg.n_layers):
        out += [(cfg.n_heads, T, T), (T, cfg.d_model), (T, cfg.ff), (T, cfg.d_model)]
    return out + [(cfg.head,)]


def keep_arrays(cfg, T, seed, sample):
    """Every site's keep array of one (clip, sample), shaped as the activation it multiplies."""
    return [torch.from_numpy(tcnref.keep_bits(seed, sample, site, cfg.n_sites, int(np.prod(sh)), cfg.dropout).astype(np.float64)).reshape(sh)
            for site, sh in enumerate(site_shapes(cfg, T))]


def bernoulli_keeps(cfg, T, batch, generator):
    """keep arrays drawn by torch's own generator, as nn.Dropout draws them: Bernoulli(1 - p) per element"""
    return [torch.bernoulli(torch.full((batch,) + sh, 1.0 - cfg.dropout), generator=generator) for sh in site_shapes(cfg, T)]


def forward(cfg, w, x, mask=None, keeps=None, dtype=torch.float64):
    """x [T, F] -> (trunk [T, D], pred scalar tensor, saliency [T]) in `dtype`; x [B, T, F] -> ([B, T, D], [B], [B, T]).  mask: None or
    bool [T] / [B, T], True = masked.  keeps: None (eval mode), one 0/1 array per dropout site (site_shapes, with a leading B for a
    batch), or a function (activation, site) -> activation that does the dropout itself (tools/xfm_ab.py: F.dropout)."""
    W = {k: v.to(dtype) for k, v in w.items()}
    batched = x.dim() == 3
    scale = torch.tensor(float(np.float32(1.0 / (1.0 - cfg.dropout))), dtype=dtype)
    qs = torch.tensor(float(np.float32(1.0 / np.sqrt(float(cfg.head_dim)))), dtype=dtype, device=x.device)
    D, H, dh = cfg.d_model, cfg.n_heads, cfg.head_dim

    def drop(v, site):
        if callable(keeps):
            return keeps(v, site)
        if keeps is None:
            return v
        k = keeps[site].to(dtype)
        return v * (k if batched else k[None]) * scale

    xb = (x if batched else x[None]).to(dtype)
    B, T = xb.shape[:2]
    mk = None if mask is None else (mask if mask.dim() == 2 else mask[None]).bool()
    h = drop(xb @ W["in.weight"].t() + W["in.bias"] + W["pe"][:T], 0)
    P = None
    for l in range(cfg.n_layers):
        p = f"layer.{l}."
        a = F.layer_norm(h, (D,), W[p + "ln1.weight"], W[p + "ln1.bias"], 1e-5)
        q, k, v = ((a @ W[p + "qkv.weight"].t() + W[p + "qkv.bias"]).reshape(B, T, 3, H, dh).permute(2, 0, 3, 1, 4))  # each [B, H, T, dh]
        s = (q * qs) @ k.transpose(-1, -2)
        if mk is not None:
            s = s.masked_fill(mk[:, None, None, :], float("-inf"))
        P = drop(torch.softmax(s, -1), 1 + 4 * l)
        o = (P @ v).permute(0, 2, 1, 3).reshape(B, T, D)
        h = h + drop(o @ W[p + "out.weight"].t() + W[p + "out.bias"], 2 + 4 * l)
        a = F.layer_norm(h, (D,), W[p + "ln2.weight"], W[p + "ln2.bias"], 1e-5)
        f = drop(F.gelu(a @ W[p + "ff1.weight"].t() + W[p + "ff1.bias"]), 3 + 4 * l)
        h = h + drop(f @ W[p + "ff2.weight"].t() + W[p + "ff2.bias"], 4 + 4 * l)
    trunk = F.layer_norm(h, (D,), W["lnf.weight"], W["lnf.bias"], 1e-5)
    if mk is None:
        pooled = trunk.mean(1)
    else:
        live = (~mk).to(dtype)[..., None]
        pooled = (trunk * live).sum(1) / live.sum(1).clamp(min=1)
    hid = drop(torch.relu(pooled @ W["head.fc1.weight"].t() + W["head.fc1.bias"]), 4 * cfg.n_layers + 1)
    pred = torch.sigmoid(hid @ W["head.fc2.weight"].t() + W["head.fc2.bias"])[:, 0]
    sal = P.mean(1).sum(1)  # head-averaged weights of the last layer, summed over the queries
    return (trunk, pred, sal) if batched else (trunk[0], pred[0], sal[0])


def make_masks(n, T, g, single=False):
    """bool [n, T]: clip 0 unmasked, clip 1 about 30 % masked at random, clip 2 masked at both ends as pad_or_truncate pads; further clips
    repeat.  single: every clip has ONE unmasked step.  Every clip keeps at least one unmasked step."""
    m = torch.zeros((n, T), dtype=torch.bool)
    for i in range(n):
        if single:
            m[i] = True
            m[i, int(torch.randint(0, T, (1,), generator=g))] = False
        elif i % 3 == 1:
            m[i] = torch.rand((T,), generator=g) < 0.3
            m[i, T // 2] = False
        elif i % 3 == 2:
            before = T // 4
            m[i, :before] = True
            m[i, T - (before + 1 if before else 0):] = True  # the longer half behind, as (target - n) // 2 leaves it
    return m


@dataclasses.dataclass
class Case:
    """One (configuration, T, S) of a test module with its inputs and its float64 / float32 references, computed once."""
    name: str
    cfg: object
    weights: dict
    x: torch.Tensor      # [n, T, F]
    mask: torch.Tensor   # uint8 [n, T]
    seeds: list
    S: int
    trunk64: torch.Tensor = None  # [n, max(S, 1), T, D]
    pred64: torch.Tensor = None   # [n, max(S, 1)]
    sal64: torch.Tensor = None    # [n, T], S = 0 only
    e_trunk: float = 0.0          # max |float32 - float64| / max |float64|
    e_pred: float = 0.0
    e_sal: float = 0.0


def make_case(name, cfg, weights, T, S, n=3, seed=0, single=False):
    g = torch.Generator().manual_seed(1000 * T + 10 * S + seed)
    x = torch.randn((n, T, cfg.input_dim), generator=g)
    seeds = [int(v) & M64 for v in torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g).tolist()]
    seeds[0] |= 1 << 63  # the top bit too
    mask = make_masks(n, T, g, single)
    case = Case(name, cfg, weights, x, mask.to(torch.uint8), seeds, S)
    smax = max(S, 1)
    t64, p64, s64, t32, p32, s32 = [], [], [], [], [], []
    for i in range(n):
        for s in range(smax):
            keeps = keep_arrays(cfg, T, seeds[i], s) if S else None
            a, b, c = forward(cfg, weights, x[i], mask[i], keeps, torch.float64)
            d, e, f = forward(cfg, weights, x[i], mask[i], keeps, torch.float32)
            t64.append(a), p64.append(b), s64.append(c), t32.append(d.double()), p32.append(e.double()), s32.append(f.double())
    D = cfg.d_model
    case.trunk64, case.pred64 = torch.stack(t64).reshape(n, smax, T, D), torch.stack(p64).reshape(n, smax)
    case.e_trunk = float((torch.stack(t32).reshape(n, smax, T, D) - case.trunk64).abs().max() / case.trunk64.abs().max())
    case.e_pred = float((torch.stack(p32).reshape(n, smax) - case.pred64).abs().max())
    if S == 0:
        case.sal64 = torch.stack(s64)
        case.e_sal = float((torch.stack(s32) - case.sal64).abs().max() / case.sal64.abs().max())
    return case


def tolerances(cases):
    """The rule of tcnref.tolerances, unchanged: e_ref is the largest float32-vs-float64 difference of xfmref itself over ALL cases of
    the module (trunk and saliency: relative to max |float64| of their case); the code under test may be off from float64 by 4 e_ref —
    the same f32 operations in another order — and a prediction by 4 f32 spacings at 1.0 more.  Returns (tol_trunk, tol_pred, tol_sal,
    e_trunk, e_pred, e_sal)."""
    e_trunk, e_pred, e_sal = max(c.e_trunk for c in cases), max(c.e_pred for c in cases), max(c.e_sal for c in cases)
    return 4 * e_trunk, 4 * e_pred + PRED_FLOOR, 4 * e_sal, e_trunk, e_pred, e_sal


def check_case(case, trunk, pred, sal, tols, what):
    """trunk / pred / saliency of the code under test against the case's float64 reference; returns the ratios error / allowed."""
    tol_trunk, tol_pred, tol_sal = tols[:3]
    scale = float(case.trunk64.abs().max())
    dt = float((trunk.double().cpu() - case.trunk64).abs().max())
    dp = float((pred.double().cpu() - case.pred64).abs().max())
    rt, rp, rs, ds, sscale = dt / (tol_trunk * scale), dp / tol_pred, 0.0, 0.0, 0.0
    if case.S == 0:
        sscale = float(case.sal64.abs().max())
        ds = float((sal.double().cpu() - case.sal64).abs().max())
        rs = ds / (tol_sal * sscale)
    print(f"{what} {case.name}: trunk |d| {dt:.3g} of max {scale:.3g} (ratio to the bound {rt:.3f}), pred |d| {dp:.3g} (ratio {rp:.3f}), "
          f"saliency |d| {ds:.3g} of max {sscale:.3g} (ratio {rs:.3f})")
    assert dt <= tol_trunk * scale, (what, case.name, "trunk", dt, tol_trunk * scale)
    assert dp <= tol_pred, (what, case.name, "pred", dp, tol_pred)
    assert case.S != 0 or ds <= tol_sal * sscale, (what, case.name, "saliency", ds, tol_sal * sscale)
    return rt, rp, rs
