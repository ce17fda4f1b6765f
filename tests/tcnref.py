"""Yardstick of the TCN gait model tests (a helper, not a test): the network of include/lmx.h "The TCN gait model" restated functionally
in torch — F.conv1d on a left-padded series, dropout as explicit keep arrays — in float32 or float64; the keep decision restated in
numpy uint64 from the header's text; a seeded weight generator that emits a state_dict under the reference's key names; and the
tolerance rule the host and GPU tests share."""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from lmx import tcn

SHIPPED = tcn.TcnConfig()
TINY = tcn.TcnConfig(input_dim=5, channels=(16, 32), kernel_size=2, dropout=0.2, head=32)  # a residual 1x1 in block 0 AND block 1, ragged input
DEEP = tcn.TcnConfig(input_dim=44, channels=(64,) * 6, kernel_size=3, dropout=0.2, head=32)  # dilation 32 exceeds a small T
CONFIGS = {"shipped": SHIPPED, "tiny": TINY, "deep": DEEP}
M64 = (1 << 64) - 1
PRED_FLOOR = 4 * 2.0 ** -24  # 4 spacings of float32 just below 1.0: 2.4e-7


def state_dict(cfg, seed, legacy=False):
    """A state_dict as `torch.save(model.state_dict())` of the reference's TCN writes it (legacy: the weight_g / weight_v spelling of
    older torch).  v is drawn like torch's default Conv1d initialisation, g is ||v|| times a factor in 0.8 .. 1.2 so that folding matters."""
    g = torch.Generator().manual_seed(seed)

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    sd = {}
    for i, n in enumerate(cfg.channels):
        cin = cfg.block_inputs(i)
        for name, c in (("conv1", cin), ("conv2", n)):
            bound = 1.0 / (c * cfg.kernel_size) ** 0.5
            v = uniform((n, c, cfg.kernel_size), bound)
            gain = v.flatten(1).norm(dim=1).reshape(n, 1, 1) * (0.8 + 0.4 * torch.rand((n, 1, 1), generator=g))
            names = ("weight_g", "weight_v") if legacy else ("parametrizations.weight.original0", "parametrizations.weight.original1")
            sd[f"network.{i}.{name}.conv.{names[0]}"], sd[f"network.{i}.{name}.conv.{names[1]}"] = gain, v
            sd[f"network.{i}.{name}.conv.bias"] = uniform((n,), bound)
        if cin != n:
            sd[f"network.{i}.residual.weight"] = uniform((n, cin, 1), 1.0 / cin ** 0.5)
            sd[f"network.{i}.residual.bias"] = uniform((n,), 1.0 / cin ** 0.5)
    c = cfg.channels[-1]
    sd["classifier.2.weight"], sd["classifier.2.bias"] = uniform((cfg.head, c), 1.0 / c ** 0.5), uniform((cfg.head,), 1.0 / c ** 0.5)
    sd["classifier.5.weight"], sd["classifier.5.bias"] = uniform((1, cfg.head), 1.0 / cfg.head ** 0.5), uniform((1,), 1.0 / cfg.head ** 0.5)
    return sd


def keep_bits(seed, sample, site, n_sites, count, p):
    """The keep decision of include/lmx.h in numpy uint64 (arithmetic mod 2^64 by wrap-around): uint8 [count]."""
    with np.errstate(over="ignore"):
        u = np.arange(count, dtype=np.uint64)
        stream = np.uint64(sample * n_sites + site)
        z = np.uint64(seed & M64) + np.uint64(0x9E3779B97F4A7C15) * ((stream << np.uint64(32)) + u + np.uint64(1))
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    thr = np.uint64(int(np.floor(p * 2.0 ** 32)))
    return ((z >> np.uint64(32)) >= thr).astype(np.uint8)


def site_counts(cfg, T):
    """elements of each dropout site: C * T after each convolution, the head's width at the end"""
    return [cfg.channels[s // 2] * T for s in range(2 * cfg.n_blocks)] + [cfg.head]


def keep_arrays(cfg, T, seed, sample):
    """Every site's keep array of one (clip, sample), shaped as the activation it multiplies: [C, T] per convolution, [head]."""
    out = []
    for site, count in enumerate(site_counts(cfg, T)):
        k = torch.from_numpy(keep_bits(seed, sample, site, cfg.n_sites, count, cfg.dropout).astype(np.float64))
        out.append(k.reshape(-1, T) if site < 2 * cfg.n_blocks else k)
    return out


def forward(cfg, folded, x, keeps=None, dtype=torch.float64):
    """x [T, F] -> (trunk [T, C], pred scalar tensor) in `dtype`; x [B, T, F] -> ([B, T, C], [B]).  keeps: None (eval mode) or one 0/1
    array per dropout site ([C, T] or [B, C, T]; [head] or [B, head]); kept values are multiplied by float32(1 / (1 - p)).  keeps may
    also be a function (activation, site) -> activation that does the dropout itself (tools/tcn_ab.py: F.dropout, as the reference runs)."""
    w = {k: v.to(dtype) for k, v in folded.items()}
    scale = torch.tensor(float(np.float32(1.0 / (1.0 - cfg.dropout))), dtype=dtype)
    k = cfg.kernel_size

    def drop(v, site):
        if callable(keeps):
            return keeps(v, site)
        return v if keeps is None else v * keeps[site].to(dtype).reshape((-1,) + v.shape[1:]) * scale

    h = (x[None] if x.dim() == 2 else x).to(dtype).transpose(1, 2)  # [B, F, T]
    for i in range(cfg.n_blocks):
        d = 2 ** i
        a = F.conv1d(F.pad(h, ((k - 1) * d, 0)), w[f"block.{i}.conv1.weight"], w[f"block.{i}.conv1.bias"], dilation=d)
        a = drop(torch.relu(a), 2 * i)
        b = F.conv1d(F.pad(a, ((k - 1) * d, 0)), w[f"block.{i}.conv2.weight"], w[f"block.{i}.conv2.bias"], dilation=d)
        b = drop(torch.relu(b), 2 * i + 1)
        res = F.conv1d(h, w[f"block.{i}.res.weight"], w[f"block.{i}.res.bias"]) if f"block.{i}.res.weight" in w else h
        h = torch.relu(b + res)
    pooled = h.mean(dim=2)
    hid = drop(torch.relu(pooled @ w["head.fc1.weight"].t() + w["head.fc1.bias"]), 2 * cfg.n_blocks)
    pred = torch.sigmoid(hid @ w["head.fc2.weight"].t() + w["head.fc2.bias"])[:, 0]
    trunk = h.transpose(1, 2).contiguous()
    return (trunk[0], pred[0]) if x.dim() == 2 else (trunk, pred)


def bernoulli_keeps(cfg, T, batch, generator):
    """keep arrays drawn by torch's own generator, as nn.Dropout draws them: Bernoulli(1 - p) per element"""
    shapes = [(batch, cfg.channels[s // 2], T) for s in range(2 * cfg.n_blocks)] + [(batch, cfg.head)]
    return [torch.bernoulli(torch.full(sh, 1.0 - cfg.dropout), generator=generator) for sh in shapes]


@dataclasses.dataclass
class Case:
    """One (configuration, T, S) of a test module with its inputs and its float64 / float32 references, computed once."""
    name: str
    cfg: object
    folded: dict
    x: torch.Tensor      # [n, T, F]
    seeds: list
    S: int
    trunk64: torch.Tensor = None  # [n, max(S, 1), T, C]
    pred64: torch.Tensor = None   # [n, max(S, 1)]
    e_trunk: float = 0.0          # max |float32 - float64| / max |float64|
    e_pred: float = 0.0


def make_case(name, cfg, folded, T, S, n=3, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * S + seed)
    x = torch.randn((n, T, cfg.input_dim), generator=g)
    seeds = [int(v) & M64 for v in torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g).tolist()]
    seeds[0] |= 1 << 63  # the top bit too
    case = Case(name, cfg, folded, x, seeds, S)
    smax = max(S, 1)
    t64, p64, t32, p32 = [], [], [], []
    for i in range(n):
        for s in range(smax):
            keeps = keep_arrays(cfg, T, seeds[i], s) if S else None
            a, b = forward(cfg, folded, x[i], keeps, torch.float64)
            c, d = forward(cfg, folded, x[i], keeps, torch.float32)
            t64.append(a), p64.append(b), t32.append(c.double()), p32.append(d.double())
    C = cfg.channels[-1]
    case.trunk64, case.pred64 = torch.stack(t64).reshape(n, smax, T, C), torch.stack(p64).reshape(n, smax)
    case.e_trunk = float((torch.stack(t32).reshape(n, smax, T, C) - case.trunk64).abs().max() / case.trunk64.abs().max())
    case.e_pred = float((torch.stack(p32).reshape(n, smax) - case.pred64).abs().max())
    return case


def tolerances(cases):
    """The rule of the tests: e_ref is the largest float32-vs-float64 difference of tcnref itself over ALL cases of the module (trunk:
    relative to max |trunk64| of its case); the code under test may be off from float64 by 4 e_ref — the same f32 operations in another
    summation order — and a prediction by 4 f32 spacings at 1.0 more (an accurate exp, an add and a divide)."""
    e_trunk, e_pred = max(c.e_trunk for c in cases), max(c.e_pred for c in cases)
    return 4 * e_trunk, 4 * e_pred + PRED_FLOOR, e_trunk, e_pred


def check_case(case, trunk, pred, tol_trunk, tol_pred, what):
    """trunk / pred of the code under test against the case's float64 reference; returns the two ratios error / allowed."""
    scale = float(case.trunk64.abs().max())
    dt = float((trunk.double().cpu() - case.trunk64).abs().max())
    dp = float((pred.double().cpu() - case.pred64).abs().max())
    rt, rp = dt / (tol_trunk * scale), dp / tol_pred
    print(f"{what} {case.name}: trunk |d| {dt:.3g} of max {scale:.3g} (ratio to the bound {rt:.3f}), pred |d| {dp:.3g} (ratio {rp:.3f})")
    assert dt <= tol_trunk * scale, (what, case.name, dt, tol_trunk * scale)
    assert dp <= tol_pred, (what, case.name, dp, tol_pred)
    return rt, rp


def check_stats(pred, stats, S):
    """stats is the float64 mean and unbiased standard deviation of the pred row it read, to a few f32 spacings of the value"""
    p, s = pred.double().cpu(), stats.double().cpu()
    if S == 0:
        assert torch.equal(stats[:, 0], pred[:, 0]) and not stats[:, 1].any()
        return
    mean, std = p.mean(1), p.std(1)  # unbiased
    assert (s[:, 0] - mean).abs().max() <= 4 * 2.0 ** -24, (s[:, 0], mean)       # the mean lies in (0, 1): spacing <= 2^-24
    # the deviations are differences of values in (0, 1) known to 2^-24 each: their root mean square is known to a few 2^-24 as well
    assert (s[:, 1] - std).abs().max() <= 8 * 2.0 ** -24, (s[:, 1], std)
