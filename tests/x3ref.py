"""Float64 model of the exact plan's x3 operand format (include/lmx.h "EXACT-precision plan"), written
from the documented semantics and shared by tests/test_exact_x3_host.py (CPU) and tests/test_gpu_exact.py (GPU).

An f32 value x travels as the f16 triple [hi | lo | hi] per channel group of width g, hi = f16(x), lo = f16((x - hi) * 2048);
a weight row as [whi | whi / 2048 | wlo] over the same groups, pre-scaled by 2^e (lmx.exact.split_rows_x3).  One f16 GEMM over
the 3K columns then yields x . w up to the dropped (x - hi)(w - whi) term.  The bound the tests hold every kernel of the plan to
is per output element

    |got - ref| <= c * sum_k |x_k w_k|

with ref the float64 result of the same operation on the f32 values."""
import numpy as np
import torch


def x3_split(x):
    """f32 tensor -> (hi, lo) f16 with x = hi + lo / 2048 up to lo's rounding (x - hi is exact in f32)."""
    x = torch.as_tensor(x).float()
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    return hi, lo


def _groups(N, g):
    """Channel group widths: g = None (one group), an int (equal groups) or a list (as split_rows_x3 takes)."""
    if g is None:
        return [N]
    if isinstance(g, int):
        return [g] * (N // g)
    assert sum(g) == N, (g, N)
    return list(g)


def x3_pack(x, g=None, drop_lo=False):
    """f32 [..., N] -> f16 [..., 3N]: per channel group (widths g, see _groups) the triple [hi | lo | hi]."""
    x = torch.as_tensor(x).float()
    hi, lo = x3_split(x)
    if drop_lo:
        lo = torch.zeros_like(lo)
    parts, o = [], 0
    for w in _groups(x.shape[-1], g):
        s = slice(o, o + w)
        parts += [hi[..., s], lo[..., s], hi[..., s]]
        o += w
    return torch.cat(parts, -1)


def x3_value(t3, g=None):
    """f16 [..., 3N] x3 groups -> float64 [..., N] = hi + lo / 2048 (the value the plan carries)."""
    return _x3_part(t3, g, 0) + _x3_part(t3, g, 1) / 2048.0


def _x3_part(t3, g, j):
    """Channel j (0: hi, 1: lo, 2: hi again) of every group of an x3 tensor, float64 [..., N]."""
    t3 = torch.as_tensor(t3).double()
    out, o = [], 0
    for w in _groups(t3.shape[-1] // 3, g):
        out.append(t3[..., o + j * w:o + (j + 1) * w])
        o += 3 * w
    return torch.cat(out, -1)


def x3_hi(t3, g=None):
    """The hi channels of an x3 tensor, float64 [..., N]."""
    return _x3_part(t3, g, 0)


def x3_hi2(t3, g=None):
    """The third channel of every triple (must equal hi bit for bit), float64 [..., N]."""
    return _x3_part(t3, g, 2)


def drop_wlo(w3, groups):
    """A copy of split_rows_x3's [whi | whi/2048 | wlo] rows with the wlo columns zeroed (an f16-only weight)."""
    w3 = np.array(w3, copy=True)
    o = 0
    for g in groups:
        w3[:, o + 2 * g:o + 3 * g] = 0
        o += 3 * g
    return w3


def x3_dot(a3, w3, scale):
    """float64 value of the plan's GEMM on its f16 operands: (a3 . w3^T) * scale, every product and sum exact — what an f16 MFMA
    chain computes before its f32 roundings."""
    a = torch.as_tensor(a3).double()
    w = torch.as_tensor(np.asarray(w3)).double()
    return (a @ w.t()) * torch.as_tensor(np.asarray(scale)).double()


def f32_chain_dot(a3, w3, scale, chunk=32):
    """The same product with the accumulator rounded to f32 after every `chunk` columns (one 16x16x32 MFMA step), the row scale
    applied to the f32 result: a CPU stand-in for the device's accumulation order."""
    a = torch.as_tensor(a3).double()
    w = torch.as_tensor(np.asarray(w3)).double()
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    for k0 in range(0, a.shape[1], chunk):
        acc = (acc.double() + a[:, k0:k0 + chunk] @ w[:, k0:k0 + chunk].t()).float()
    return acc.double() * torch.as_tensor(np.asarray(scale)).double()


def abs_dot(x, w):
    """sum_k |x_k w_k| in float64: x [M, K], w [N, K] -> [M, N]."""
    return torch.as_tensor(x).double().abs() @ torch.as_tensor(np.asarray(w)).double().abs().t()


def ratio(got, ref, absdot, floor=0.0):
    """max over elements of |got - ref| / sum_k |x_k w_k| (elements whose sum is 0 must be exact: they count as inf if not)."""
    err = (torch.as_tensor(got).double().cpu() - torch.as_tensor(ref).double().cpu()).abs()
    den = torch.as_tensor(absdot).double().cpu() + floor
    r = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())
