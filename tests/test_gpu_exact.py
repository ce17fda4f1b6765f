"""The exact plan's kernels (csrc/exact.hip, include/lmx.h) against float64 references written from the
documented semantics, at the shapes, layouts and value ranges where they could go wrong.

The claim under test: a value carried as the x3 triple [hi | lo | hi] and a weight row as [whi | whi/2048 | wlo] (lmx.exact.
split_rows_x3) give, through ONE f16-MFMA GEMM over 3K columns, the f32 result of the operation.  Every GEMM-like check asserts
per output element

    |got - ref| <= C * (sum_k |x_k w_k| + |b| + |res|)

(the magnitude of all the summands: an f32 computation of the same sum can be no closer), prints the measured max ratio, and
runs the same check on the same launch with the `lo` / `wlo` channels zeroed — f16-only operands — which must miss the bound
by at least TEETH x.  References never reuse tests/cpu_kernels.py: the x3 model is tests/x3ref.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import x3ref as X

pytestmark = pytest.mark.gpu

C_GEMM = 2.0 ** -21   # GEMM / convolution bound: 1.8x the largest ratio measured on MI355X (2^-21.88; the printed ratios)
C_ELEM = 2.0 ** -21   # split3 / stem: |got - ref| <= C_ELEM * (|ref| + |inputs| + 2^-13)
FLOOR = 2.0 ** -13    # below it lo leaves the normal f16 range (lmx.h): the x3 format is exact to 2^-22 relative to max(|x|, 2^-13)
TEETH = 100.0


def _lg(r):
    return f"2^{math.log2(r):.2f}" if r > 0 else "0"


def _rows_sample(M, step=97, edge=256):
    idx = set(range(0, M, step)) | set(range(min(edge, M))) | set(range(max(0, M - edge), M))
    return torch.tensor(sorted(idx), dtype=torch.long)


def _operands(M, N, K, seed, edge=True):
    """f32 activations / weights / bias with the edge rows of the plan's range: weight row 0 all zero (e = 0), weight row 1 one
    large weight and the rest 2^-16 of it (wlo and whi / 2048 subnormal; the activation channel it meets is small, so the
    subnormal terms are what the row sums); activation row 0 in [2^-14, 2^-13) (lo subnormal), row 1 up to the f16 maximum 65504."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    if edge:
        w[0] = 0
        w[1] = (rng.standard_normal(K) * 2.0 ** -16).astype(np.float32)
        w[1, 0] = 1.0
        sgn = np.sign(rng.standard_normal((2, K)))
        x[0] = sgn[0] * np.exp2(rng.uniform(-14, -13, K))
        x[1] = sgn[1] * rng.uniform(0.5, 1.0, K) * 65504
        x[2:, 0] *= 2.0 ** -12
    return torch.from_numpy(x), w, b


def _teeth(got_t, ref, den, what):
    t = X.ratio(got_t, ref, den)
    assert t >= TEETH * C_GEMM, f"{what}: f16-only operands stay within {t / C_GEMM:.1f} x the bound: the bound has no teeth"
    return t / C_GEMM


# (label, M, N, logical K, channel groups, act, residual) — every tiling lmx_k_gemm can choose for an a_mode 0 launch
GEMM_CASES = [
    ("v1 128x64 (Detect N=80)", 1000, 80, 96, None, 0, False),
    ("v1 128x64, K'=120 (not a multiple of 64)", 300, 64, 40, None, 3, True),
    ("v1 128x128", 300, 256, 160, [64, 48, 48], 0, True),
    ("gemm2 256x256x64", 51712, 256, 160, None, 3, True),
    ("gemm2 256x256x32 short K", 51712, 224, 64, [32, 32], 0, False),
    ("gemm2 256x256x64 short K, K'=120", 51712, 224, 40, None, 0, True),
    ("gemm2 staggered 256x128x64", 4096, 256, 160, [64, 48, 48], 3, False),
    ("gemm2 256x128x32", 51712, 192, 160, None, 0, True),
]


@pytest.mark.parametrize("label,M,N,K,groups,act,res", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_x3_gemm_matches_float64(cuda, label, M, N, K, groups, act, res):
    """K.gemm on x3 activations and split weights (scale = 2^-e, bias pre-scaled by 2^e, f32 out; act / f32 residual as the SAM
    decoder's _lin) against float64 act(x @ w^T + b) + res on a row sample, through every kernel the dispatch can choose."""
    from lmx import kernels as K_
    from lmx.exact import split_rows_x3

    gl = groups or [K]
    x, w, b = _operands(M, N, K, seed=M + N + K)
    w3, sc, e = split_rows_x3(w, gl)
    bs = torch.from_numpy(np.ldexp(b, e).astype(np.float32)).to(cuda)
    sc_d = torch.from_numpy(sc).to(cuda)
    r = torch.randn((M, N), generator=torch.Generator().manual_seed(5)) * 4 if res else None
    r_d = r.to(cuda) if res else None

    def run(a3, w3_):
        return K_.gemm(a3.to(cuda), torch.from_numpy(w3_).to(cuda), bias=bs, act=act, scale=sc_d, res=r_d, out_dtype=torch.float32)

    got = run(X.x3_pack(x, gl), w3)
    s = _rows_sample(M)
    xs = x[s].double()
    pre = xs @ torch.from_numpy(w).double().t() + torch.from_numpy(b).double()
    ref = F.relu(pre) if act == K_.ACT_RELU else pre
    den = X.abs_dot(xs, w) + torch.from_numpy(np.abs(b)).double()
    if res:
        ref = ref + r[s].double()
        den = den + r[s].double().abs()
    ratio = X.ratio(got[s.to(cuda)], ref, den)
    exp0 = torch.full((len(s),), float(b[0]))  # weight row 0 is zero (e = 0): act(bias) (+ residual) exactly
    exp0 = exp0.clamp_min(0) if act == K_.ACT_RELU else exp0
    exp0 = exp0 + r[s][:, 0] if res else exp0
    assert torch.equal(got[s.to(cuda)][:, 0].cpu(), exp0), "zero weight row: the output must be act(bias) (+ residual) exactly"
    ta = _teeth(run(X.x3_pack(x, gl, drop_lo=True), w3)[s.to(cuda)], ref, den, f"{label}: lo zeroed")
    tw = _teeth(run(X.x3_pack(x, gl), X.drop_wlo(w3, gl))[s.to(cuda)], ref, den, f"{label}: wlo zeroed")
    print(f"x3 gemm {label}: max ratio {_lg(ratio)} (bound {_lg(C_GEMM)}); lo zeroed {ta:.0f} x, wlo zeroed {tw:.0f} x the bound")
    assert ratio <= C_GEMM, f"{label}: {_lg(ratio)} > {_lg(C_GEMM)}"


# (label, n, H, W, logical Cin, Cout, stride, split_k, frames the float64 reference covers)
CONV_CASES = [
    ("v1 128x64, 1 frame 16x16", 1, 16, 16, 32, 64, 1, 1, [0]),
    ("gemm2 256x128x32", 2, 24, 40, 32, 128, 1, 1, [0, 1]),
    ("gemm2 256x128x32 stride 2", 2, 48, 80, 32, 128, 2, 1, [0, 1]),
    ("gemm2 256x128x32 N=64, M >= 65536", 5, 96, 160, 32, 64, 1, 1, [4]),
    ("gemm2 staggered 256x256x32", 24, 40, 64, 32, 256, 1, 1, [0, 23]),
    ("gemm2 256x128x32 split-K 3", 2, 24, 40, 32, 128, 1, 3, [0, 1]),
    ("gemm2 staggered 256x256x32 split-K 4", 24, 40, 64, 32, 256, 1, 4, [11]),
]


@pytest.mark.parametrize("label,n,H,W,cin,cout,stride,S,frames", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_x3_conv3x3_matches_float64(cuda, label, n, H, W, cin, cout, stride, S, frames):
    """The exact plan's 3 x 3 convolution: x3 NHWC input (pixel = [hi | lo | hi] over Cin), weights split per filter tap
    (split_rows_x3(w, [Cin] * 9)), f32 pre-activation with scale / pre-scaled bias, split-K partials added in index order (as
    lmx_k_split3 does) — against float64 conv2d(x, w) + b on the listed frames."""
    from lmx import kernels as K_
    from lmx.exact import split_rows_x3

    rng = np.random.default_rng(n * 1000 + cin + cout + stride + S)
    x = torch.from_numpy(rng.standard_normal((n, H, W, cin)).astype(np.float32))
    x[0, 0, 0] = torch.from_numpy((np.sign(rng.standard_normal(cin)) * np.exp2(rng.uniform(-14, -13, cin))).astype(np.float32))
    x[0, 1, 1] = torch.from_numpy((np.sign(rng.standard_normal(cin)) * rng.uniform(0.5, 1.0, cin) * 65504).astype(np.float32))
    w = (rng.standard_normal((cout, 3, 3, cin)) * (9 * cin) ** -0.5).astype(np.float32)  # (co, ky, kx, ci): the packed order
    w[0] = 0
    w[1] = rng.standard_normal((3, 3, cin)) * 2.0 ** -16
    w[1, 1, 1, 0] = 1.0
    x[..., 0] *= 2.0 ** -12
    x[0, 1, 1, 0] = 65504.0
    b = rng.standard_normal(cout).astype(np.float32)
    w3, sc, e = split_rows_x3(w.reshape(cout, 9 * cin), [cin] * 9)
    bs = torch.from_numpy(np.ldexp(b, e).astype(np.float32)).to(cuda)
    sc_d = torch.from_numpy(sc).to(cuda)

    def run(x3, w3_):
        out = K_.conv3x3(x3.to(cuda), torch.from_numpy(w3_).to(cuda), bs, act=K_.ACT_NONE, stride=stride, scale=sc_d,
                         out_dtype=torch.float32, split_k=S)
        if S > 1:
            assert out.shape[0] == S
            tot = out[0].clone()
            for i in range(1, S):
                tot += out[i]
            out = tot
        return out[frames].cpu()

    got = run(X.x3_pack(x), w3)
    xs = x[frames].double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(w).double().permute(0, 3, 1, 2)
    ref = (F.conv2d(xs, wt, torch.from_numpy(b).double(), stride=stride, padding=1)).permute(0, 2, 3, 1)
    den = (F.conv2d(xs.abs(), wt.abs(), torch.from_numpy(np.abs(b)).double(), stride=stride, padding=1)).permute(0, 2, 3, 1)
    ratio = X.ratio(got, ref, den)
    ta = _teeth(run(X.x3_pack(x, drop_lo=True), w3), ref, den, f"{label}: lo zeroed")
    tw = _teeth(run(X.x3_pack(x), X.drop_wlo(w3, [cin] * 9)), ref, den, f"{label}: wlo zeroed")
    print(f"x3 conv3x3 {label}: max ratio {_lg(ratio)} (bound {_lg(C_GEMM)}); lo zeroed {ta:.0f} x, wlo zeroed {tw:.0f} x the bound")
    assert ratio <= C_GEMM, f"{label}: {_lg(ratio)} > {_lg(C_GEMM)}"


@pytest.mark.parametrize("M,N,Ka", [(600, 96, 64), (4096, 768, 256), (2048, 3072, 768)])
def test_a_rep2_matches_float64_and_the_explicit_copy(cuda, M, N, Ka):
    """a_rep = 2 (the SAM ViT exact plan, lmx/sam.py): f16 activations against [whi | wlo] f16 weights, one launch.  Float64
    a16 @ w32 within the bound (wlo unscaled: subnormal for small weights, 2^-24 absolute), and the SAME bits as the explicit
    torch.cat([a, a], 1) form sam.py falls back to."""
    from lmx import kernels as K_

    rng = np.random.default_rng(M + N)
    a = torch.from_numpy(rng.standard_normal((M, Ka)).astype(np.float32)).half()
    w = (rng.standard_normal((N, Ka)) * Ka ** -0.5).astype(np.float32)
    b = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    w2 = torch.from_numpy(np.ascontiguousarray(np.concatenate([hi, lo], 1))).to(cuda)
    a_d, b_d = a.to(cuda), b.to(cuda)
    got = K_.gemm(a_d, w2, bias=b_d, a_rep=2, out_dtype=torch.float32)
    cat = K_.gemm(torch.cat([a_d, a_d], 1), w2, bias=b_d, out_dtype=torch.float32)
    assert torch.equal(got, cat), "a_rep = 2 differs from the explicit [a | a] copy"
    got16 = K_.gemm(a_d, w2, bias=b_d, a_rep=2, act=K_.ACT_GELU)
    assert torch.equal(got16, K_.gemm(torch.cat([a_d, a_d], 1), w2, bias=b_d, act=K_.ACT_GELU))
    s = _rows_sample(M)
    ref = a[s].double() @ torch.from_numpy(w).double().t() + b.double()
    den = X.abs_dot(a[s].float(), w) + b.double().abs()
    ratio = X.ratio(got[s.to(cuda)], ref, den)
    t = X.ratio(K_.gemm(a_d, w2[:, :Ka].contiguous(), bias=b_d, out_dtype=torch.float32)[s.to(cuda)], ref, den)
    print(f"a_rep 2 {M}x{N}x{Ka}: max ratio {_lg(ratio)} (bound {_lg(C_GEMM)}); whi alone {t / C_GEMM:.0f} x the bound")
    assert ratio <= C_GEMM and t >= TEETH * C_GEMM, (_lg(ratio), t / C_GEMM)


# ------------------------------------------------------------------------------------------------ split3 / split3_rows
def _act64(x, act):
    return [x, x / (1 + torch.exp(-x)), 0.5 * x * (1 + torch.erf(x / math.sqrt(2))), x.clamp_min(0)][act]


def _check_x3(out3, g, ref, den, what):
    """hi + lo/2048 within C_ELEM of ref, the third channel the first bit for bit, and hi alone far outside the bound."""
    v = X.x3_value(out3, g)
    r = X.ratio(v, ref, den)
    assert torch.equal(X.x3_hi(out3, g), X.x3_hi2(out3, g)), f"{what}: third channel differs from the first"
    t = X.ratio(X.x3_hi(out3, g), ref, den)
    assert r <= C_ELEM, f"{what}: {_lg(r)} > {_lg(C_ELEM)}"
    assert t >= TEETH * C_ELEM, f"{what}: hi alone stays within {t / C_ELEM:.1f} x the bound"
    return r, t / C_ELEM


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("N,g,nsum,res,ldx_pad", [(64, None, 1, False, 0), (96, 32, 1, True, 0), (128, 64, 3, True, 16), (48, 16, 2, False, 8)])
def test_split3_matches_float64(cuda, act, N, g, nsum, res, ldx_pad):
    """lmx_k_split3: y = act(sum of nsum partials) + value(res3), written as per-group [hi | lo | hi] triples into a channel slice
    of a wider buffer (canary-filled neighbours unchanged), from a strided input (ldx > N) and partials at a sum_stride."""
    from lmx import kernels as K_

    n, H, W = 2, 5, 7
    gen = torch.Generator().manual_seed(N * 10 + act)
    base = torch.randn((nsum, n, H, W, N + ldx_pad), generator=gen) * 3
    base[0, 0, 0, 0, 0] = 60000.0
    base[0, 0, 0, 0, 1:4] = torch.tensor([1e-5, -7e-4, 2.0 ** -13])
    parts = base[..., :N]
    C3 = 3 * N
    buf = torch.full((n, H, W, C3 + 48), 1234.0).half()  # the output is channels 24 .. 24 + 3N of a wider x3 buffer
    dev_buf = buf.to(cuda)
    out3 = dev_buf[..., 24:24 + C3]
    xv = base.to(cuda)[..., :N]
    x_in = xv if nsum > 1 else xv[0]
    gl = g or N
    rv = None
    res3 = None
    if res:
        rv = torch.randn((n, H, W, N), generator=gen) * 2
        res3 = X.x3_pack(rv, gl).to(cuda)
        rv = X.x3_value(res3.cpu(), gl)
    K_.split3(x_in, act, out3, g=g, res3=res3)
    host = dev_buf.cpu()
    assert torch.equal(host[..., :24].view(torch.int16), buf[..., :24].view(torch.int16)) and \
        torch.equal(host[..., 24 + C3:].view(torch.int16), buf[..., 24 + C3:].view(torch.int16)), "split3 wrote outside its channel slice"
    xs = parts.double().sum(0)
    ref = _act64(xs, act)
    den = ref.abs() + parts.double().abs().sum(0) + FLOOR
    if res:
        ref = ref + rv
        den = den + rv.abs()
    r, t = _check_x3(host[..., 24:24 + C3], gl, ref, den, f"split3 act={act} N={N} g={g} nsum={nsum}")
    print(f"split3 act={act} N={N} g={g} nsum={nsum} res={res}: max ratio {_lg(r)} (bound {_lg(C_ELEM)}); hi alone {t:.0f} x")


@pytest.mark.parametrize("act", [0, 2])
def test_split3_rows_matches_float64(cuda, act):
    """split3_rows (the decoder's x3 A operand): contiguous [hi | lo | hi] rows of act(x) from a strided f32 row view."""
    from lmx import kernels as K_

    x = torch.randn((301, 160), generator=torch.Generator().manual_seed(act)) * 4
    x[0, :3] = torch.tensor([65000.0, 1e-6, -3e-5])
    xd = x.to(cuda)[:, :128]
    out = K_.split3_rows(xd, act)
    assert out.shape == (301, 384) and out.is_contiguous()
    ref = _act64(x[:, :128].double(), act)
    r, t = _check_x3(out.cpu(), None, ref, ref.abs() + x[:, :128].double().abs() + FLOOR, f"split3_rows act={act}")
    print(f"split3_rows act={act}: max ratio {_lg(r)} (bound {_lg(C_ELEM)}); hi alone {t:.0f} x")


# ------------------------------------------------------------------------------------------------ maxpool5_x3
@pytest.mark.parametrize("n,H,W,C", [(2, 3, 4, 16), (1, 9, 13, 8), (3, 1, 6, 24)])
def test_maxpool5_x3_picks_the_max_and_its_pair(cuda, n, H, W, C):
    """max_pool2d(5, 1, 2) on an x3 slice: the joined output value equals the float64 maximum of the joined inputs in the
    window exactly, the (hi, lo) pair is the pair of a pixel that attains it, the third channel equals the first; H or W below
    5, borders, ties and negative values (all-negative windows)."""
    from lmx import kernels as K_

    gen = torch.Generator().manual_seed(n * 100 + H * 10 + W)
    v = -torch.rand((n, H, W, C), generator=gen) * 8 - 0.5  # negative everywhere
    v[0, 0, :, :4] = 3.25  # ties: a row of equal values
    v[..., -1] = torch.randint(-3, 3, (n, H, W), generator=gen).float()  # integer plateaus: many ties
    x3 = X.x3_pack(v)
    src = torch.full((n, H, W, 3 * C + 8), 7.0).half()
    src[..., :3 * C] = x3
    dst = torch.full((n, H, W, 3 * C + 16), 55.0).half().to(cuda)
    K_.maxpool5_x3(src.to(cuda)[..., :3 * C], dst[..., 8:8 + 3 * C])
    got = dst.cpu()
    assert (got[..., :8] == 55).all() and (got[..., 8 + 3 * C:] == 55).all(), "maxpool5_x3 wrote outside its slice"
    got = got[..., 8:8 + 3 * C]
    val = X.x3_value(x3)  # [n,H,W,C] float64
    ref = F.max_pool2d(val.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)
    assert torch.equal(X.x3_value(got), ref), "joined maximum differs from the float64 maximum"
    assert torch.equal(got[..., :C].view(torch.int16), got[..., 2 * C:].view(torch.int16))
    # the pair: some pixel of the window has exactly this (hi, lo)
    hi_o, lo_o = got[..., :C].view(torch.int16).long(), got[..., C:2 * C].view(torch.int16).long()
    key_o = hi_o * 65536 + (lo_o & 0xFFFF)
    key_i = (x3[..., :C].view(torch.int16).long() * 65536 + (x3[..., C:2 * C].view(torch.int16).long() & 0xFFFF)).double()
    found = torch.zeros_like(key_o, dtype=torch.bool)
    kp = F.pad(key_i.permute(0, 3, 1, 2), (2, 2, 2, 2), value=float("nan")).permute(0, 2, 3, 1)
    for dy in range(5):
        for dx in range(5):
            found |= kp[:, dy:dy + H, dx:dx + W, :] == key_o.double()
    assert found.all(), "an output (hi, lo) pair is not the pair of any pixel in its window"


# ------------------------------------------------------------------------------------------------ stem_conv_x3
@pytest.mark.parametrize("n,H,W,Cout", [(1, 17, 23, 16), (2, 9, 31, 64), (1, 33, 15, 256)])
def test_stem_conv_x3_matches_float64(cuda, n, H, W, Cout):
    """The exact plan's stem (Conv(3 -> Cout, k3, s2, p1) + bias + SiLU from the u8 frame, written x3): odd H and W, u8 values 0
    and 255 included, against float64 silu(conv2d(u8 / 255, w) + b)."""
    from lmx import kernels as K_

    gen = torch.Generator().manual_seed(H * W + Cout)
    img = torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8)
    img[0, :3] = 255
    img[0, -3:] = 0
    w = torch.randn((3, 3, 3, Cout), generator=gen) * 0.5  # (ky, kx, c, co)
    b = torch.randn((Cout,), generator=gen)
    out = K_.stem_conv_x3(img.to(cuda), w.to(cuda), b.to(cuda)).cpu()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert out.shape == (n, Ho, Wo, 3 * Cout)
    xs = img.double().permute(0, 3, 1, 2) / 255
    wt = w.double().permute(3, 2, 0, 1)
    z = F.conv2d(xs, wt, b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
    ref = z / (1 + torch.exp(-z))
    den = F.conv2d(xs, wt.abs(), b.double().abs(), stride=2, padding=1).permute(0, 2, 3, 1) + FLOOR
    r, t = _check_x3(out, None, ref, den, f"stem_conv_x3 {H}x{W} Cout={Cout}")
    print(f"stem_conv_x3 {n}x{H}x{W} Cout={Cout}: max ratio {_lg(r)} (bound {_lg(C_ELEM)}); hi alone {t:.0f} x")


# ------------------------------------------------------------------------------------------------ attention_f32
@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("Tk", [1, 7, 16, 17, 64, 4096])
def test_attention_f32_matches_float64(cuda, hd, Tk):
    """lmx_k_attention_f32 on both sides of its thread / wave switch (Tk 16 | 17): B*H*Tq not a multiple of 4, q / k / v / o row
    views with ld > H*hd, scores up to ~300 (exp without the max subtraction would overflow f32), against a float64 softmax."""
    from lmx import kernels as K_

    B, H, Tq = 3, 3 if hd == 32 else 5, 7
    gen = torch.Generator().manual_seed(hd * 10000 + Tk)
    pad = 12
    q = torch.randn((B * Tq, H * hd + pad), generator=gen) * 4
    k = torch.randn((B * Tk, H * hd + 2 * pad), generator=gen) * 4
    v = torch.randn((B * Tk, H * hd + pad), generator=gen)
    scale = hd ** -0.5 * 3
    qd, kd, vd = (t.to(cuda)[:, :H * hd] for t in (q, k, v))
    got = K_.attention_f32(qd, kd, vd, B, H, Tq, Tk, hd, scale).cpu().view(B, Tq, H, hd).double()
    qh = q[:, :H * hd].double().view(B, Tq, H, hd).permute(0, 2, 1, 3)
    kh = k[:, :H * hd].double().view(B, Tk, H, hd).permute(0, 2, 1, 3)
    vh = v[:, :H * hd].double().view(B, Tk, H, hd).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(-1, -2) * scale
    assert float(s.abs().max()) > 100, "scores must be large enough to overflow exp without the max subtraction"
    p = torch.softmax(s, -1)
    ref = (p @ vh).permute(0, 2, 1, 3)
    # an f32 score of magnitude S carries ~hd * 2^-24 * S absolute error, which exp turns into that relative error of p: the
    # bound scales with the row's largest absolute score sum_d |q_d k_d| * scale
    sabs = ((qh.abs() @ kh.abs().transpose(-1, -2)) * scale).amax(-1, keepdim=True)
    den = ((1 + sabs) * (p @ vh.abs())).permute(0, 2, 1, 3)
    r = float(((got - ref).abs() / den).max())
    assert torch.isfinite(got).all()
    print(f"attention_f32 hd={hd} Tk={Tk}: max |err| / ((1 + max_j sum_d |q k| scale) sum_j p_j |v_j|) = {_lg(r)} (bound 2^-18)")
    assert r <= 2.0 ** -18, _lg(r)


# ------------------------------------------------------------------------------------------------ hyper_mask_f32
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("n,G,C", [(1, 3, 32), (2, 16, 16), (3, 5, 64)])
def test_hyper_mask_f32_matches_float64(cuda, act, n, G, C):
    """lmx_k_hyper_mask_f32: logits = act(up) . hyper over C, up in nested quadrant order [n][G*G][4][4][C]; the reference puts
    pixels where two ConvTranspose2d(k2, s2) steps put them — two pixel_shuffle(., 2) — not by the kernel's index formula."""
    from lmx import kernels as K_

    gen = torch.Generator().manual_seed(n * 100 + G * C + act)
    up = torch.randn((n, G * G, 4, 4, C), generator=gen) * 2
    hyper = torch.randn((n, C), generator=gen)
    got = K_.hyper_mask_f32(up.to(cuda), hyper.to(cuda), n, G, C, act=act).cpu().double()
    u = _act64(up.double(), act)
    small = torch.einsum("ngabc,nc->ngab", u, hyper.double()).view(n, G, G, 4, 4)  # [n, y, x, q1, q2]
    a = small.permute(0, 4, 3, 1, 2).reshape(n, 16, G, G)   # channel = q2 * 4 + q1: the first step shuffles q1
    a = F.pixel_shuffle(a, 2)                               # [n, 4 (q2), 2G, 2G] at (2y + dy1, 2x + dx1)
    ref = F.pixel_shuffle(a, 2)[:, 0]                       # [n, 4G, 4G] at (2(2y + dy1) + dy2, ...)
    mag = u.abs() + up.double().abs()  # GELU's 1 + erf cancels for negative inputs: f32 error there scales with |x|, not |gelu(x)|
    den = F.pixel_shuffle(F.pixel_shuffle(torch.einsum("ngabc,nc->ngab", mag, hyper.double().abs()).view(n, G, G, 4, 4)
                                          .permute(0, 4, 3, 1, 2).reshape(n, 16, G, G), 2), 2)[:, 0]
    r = X.ratio(got, ref, den)
    print(f"hyper_mask_f32 act={act} n={n} G={G} C={C}: max ratio {_lg(r)}")
    assert r <= 2.0 ** -20, _lg(r)


# ------------------------------------------------------------------------------------------------ add_bcast
@pytest.mark.parametrize("a_dt", [torch.float16, torch.float32])
@pytest.mark.parametrize("o_dt", [torch.float16, torch.float32])
@pytest.mark.parametrize("rows,b_rows", [(37, 37), (7 * 9, 7), (4096 * 2, 4096)])
def test_add_bcast_bit_exact(cuda, a_dt, o_dt, rows, b_rows):
    """lmx_k_add_bcast: out[r] = a[r] + b[r % b_rows], strided row views on every side, bit for bit torch's CPU
    (a.float() + b).to(out dtype): one f32 addition, one round-to-nearest-even to f16 — no freedom to differ."""
    from lmx import kernels as K_

    D = 32
    gen = torch.Generator().manual_seed(rows + b_rows)
    a = (torch.randn((rows, D + 8), generator=gen) * 100).to(a_dt)
    b = torch.randn((b_rows, D + 4), generator=gen) * 100
    out = torch.full((rows, D + 12), 3.0, dtype=o_dt).to(cuda)
    K_.add_bcast(a.to(cuda)[:, :D], b.to(cuda)[:, :D], out=out[:, :D])
    ref = (a[:, :D].float() + b[torch.arange(rows) % b_rows, :D]).to(o_dt)
    got = out.cpu()
    assert torch.equal(got[:, :D], ref)
    assert (got[:, D:] == 3).all()
