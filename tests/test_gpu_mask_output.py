"""SAM's mask output chain on the MI355X against float64 (tests/maskref.py) at odd frame sizes: lmx_k_hyper_mask / _multi
(csrc/sam.hip, csrc/prompt.hip), lmx_k_mask_post (csrc/sam.hip), lmx_k_mask_logits (csrc/prompt.hip) and lmx_k_mask_score
(csrc/amg.hip).  tests/test_mask_ref_host.py establishes the bounds and the ambiguous-pixel cap without the kernels.

  frame h x w     L / T       what it reaches
  97 x 130        256 / 1024  frame smaller than the input (source step > 1, taps skipped), w % 4 == 2, one grid pass
  333 x 517       256 / 1024  w % 4 == 1, more than 96 * 256 quads: the grid-stride loop takes a second pass
  541 x 962       256 / 1024  w % 4 == 2
  1030 x 1031     256 / 1024  w % 4 == 3, scale just below 1
  1079 x 1919     256 / 1024  odd full-size frame
  1 x 1024        256 / 1024  nh == 1, h == 1
  1024 x 1        256 / 1024  nw == 1, one quad per row
  2 x 3           256 / 1024  smallest frame
  64 x 64         64 / 256    tiny Hiera's L and T
  150 x 100       128 / 512   SAM ViT test configuration, portrait
  1080 x 1920     256 / 1024  anchor of the constants
"""
import ctypes as C

import numpy as np
import pytest
import torch

import maskref as M

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 256  # guard bytes on either side of a mask
EINVAL = -1


def _lg(r):
    return f"2^{np.log2(max(r, 1e-300)):.2f}"


def _lib():
    from lmx import _lib as L

    return L.load()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _guarded_mask(n, h, w, dev):
    """(whole buffer, view [n, h, w]) with PAD bytes of 0xA5 before and after; the view starts at an address that is 1 modulo 4
    when w % 4 != 0 (rows of such a mask start at every residue anyway; the base then rules out a 4-byte store at row 0 too)."""
    off = PAD + (1 if w % 4 else 0)
    buf = torch.full((off + n * h * w + PAD,), GUARD, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    view = buf[off:off + n * h * w].view(n, h, w)
    assert view.data_ptr() % 4 == (1 if w % 4 else 0) and view.is_contiguous()
    return buf, view, off


def _mask_post_into(low, T, nh, nw, h, w, mask):
    n, L, _ = low.shape
    stats = torch.full((n, 8), -77, dtype=torch.int64, device=low.device)
    ws = torch.empty((n, nh, nw), dtype=torch.float32, device=low.device)
    rc = _lib().lmx_k_mask_post(_p(low), n, L, T, nh, nw, h, w, _p(mask), _p(stats), _p(ws), _stream(low.device))
    assert rc == 0, _lib().lmx_last_error().decode()
    torch.cuda.synchronize()
    return stats


def _check_guards(buf, off, count):
    b = buf.cpu().numpy()
    assert (b[:off] == GUARD).all(), f"{int((b[:off] != GUARD).sum())} guard bytes before the mask were written"
    assert (b[off + count:] == GUARD).all(), f"{int((b[off + count:] != GUARD).sum())} guard bytes after the mask were written"
    inside = b[off:off + count]
    assert (inside <= 1).all(), f"{int((inside > 1).sum())} mask bytes are neither 0 nor 1 (first at {int(np.argmax(inside > 1))})"


# ------------------------------------------------------------------------------------------------------------ smooth fixture
@pytest.mark.parametrize("geo", M.GEOMETRIES, ids=M.geo_id)
def test_resize_chain_matches_float64(cuda, geo):
    """Per geometry, n = 3 logits per launch: (mask_logits > 0) == mask_post's mask with no pixel excepted; mask_logits within
    the bound of float64 and of torch's f32 interpolate; mask_post's mask == (float64 > 0) on every unambiguous pixel; all seven
    statistics == numpy's of the device's own mask; mask_score(thr=0)'s area and box too; guard bytes around the mask intact."""
    from lmx import kernels as K
    from lmx import sam

    h, w, L, T = geo
    nh, nw = sam.resize_longest_side(h, w, T)
    n = M.N_MASKS
    low = M.fixture(geo)
    d = low.to(cuda)
    top = float(low.abs().max())

    buf, mask, off = _guarded_mask(n, h, w, cuda)
    stats = _mask_post_into(d, T, nh, nw, h, w, mask)
    _check_guards(buf, off, n * h * w)
    lg = K.mask_logits(d, T, nh, nw, h, w)
    assert lg.shape == (n, h, w) and bool(torch.isfinite(lg).all())
    assert torch.equal((lg > 0).to(torch.uint8), mask)

    ref64 = M.postprocess(low.double(), T, (nh, nw), (h, w))
    ref32 = M.postprocess(d, T, (nh, nw), (h, w)).cpu().double()
    got = lg.cpu().double()
    r64 = float((got - ref64).abs().max()) / M.bound64(geo, top)
    r32 = float((got - ref32).abs().max()) / M.bound32(top)
    print(f"resize {M.geo_id(geo)}: vs float64 {_lg(r64)} of the 2^{M.LOG2_BOUND64[geo]} bound, vs torch f32 {_lg(r32)} of the "
          f"2^{M.LOG2_BOUND32} bound")
    assert r64 <= 1.0 and r32 <= 1.0, (r64, r32)

    amb = M.ambiguous(ref64, M.bound64(geo, top))
    mk = mask.cpu()
    st = stats.cpu().numpy()
    score = K.mask_score(d, T, nh, nw, h, w, 0.0, 1.0).cpu().numpy()
    for i in range(n):
        k = int(amb[i].sum())
        assert k <= M.AMBIGUOUS_CAP * h * w, (i, k)
        wrong = (mk[i].bool() != (ref64[i] > 0)) & ~amb[i]
        assert not bool(wrong.any()), f"mask {i}: {int(wrong.sum())} unambiguous pixels differ from float64, first at {torch.nonzero(wrong)[0].tolist()}"
        want = M.stats(mk[i].numpy())
        assert want[0] > 0 and st[i, :7].tolist() == want and st[i, 7] == 0, (i, st[i].tolist(), want)
        assert score[i, 2] == want[0] and score[i, 3:7].tolist() == want[3:], (i, score[i].tolist(), want)


# ---------------------------------------------------------------------------------------------------------------- made masks
@pytest.mark.parametrize("hw", [(333, 517), (97, 130)], ids=["333x517", "97x130"])
def test_empty_full_and_border_masks(cuda, hw):
    from lmx import kernels as K
    from lmx import sam

    h, w = hw
    nh, nw = sam.resize_longest_side(h, w, 1024)
    low = torch.cat([M.made_low(k) for k in ("empty", "full", "border")]).to(cuda)
    buf, mask, off = _guarded_mask(3, h, w, cuda)
    st = _mask_post_into(low, 1024, nh, nw, h, w, mask).cpu().numpy()
    _check_guards(buf, off, 3 * h * w)
    mk = mask.cpu().numpy()
    assert not mk[0].any() and mk[1].all()
    # empty: lmx.h's "+-big when empty"
    assert st[0, :3].tolist() == [0, 0, 0] and st[0, 3] >= w and st[0, 4] >= h and st[0, 5] < 0 and st[0, 6] < 0, st[0].tolist()
    assert st[1, :7].tolist() == M.full_stats(h, w), st[1].tolist()
    assert st[2, 3:7].tolist() == [0, 0, w - 1, h - 1] and st[2, :7].tolist() == M.stats(mk[2]) and 0 < st[2, 0] < h * w, st[2].tolist()
    assert torch.equal((K.mask_logits(low, 1024, nh, nw, h, w) > 0).to(torch.uint8), mask)
    sc = K.mask_score(low, 1024, nh, nw, h, w, 0.0, 1.0).cpu().numpy()
    assert sc[:, 2].tolist() == st[:, 0].tolist() and sc[0, 3:7].tolist() == [0, 0, 0, 0]
    assert sc[1, 3:7].tolist() == sc[2, 3:7].tolist() == [0, 0, w - 1, h - 1]


def test_full_mask_at_4k_sums_beyond_32_bits(cuda):
    """2160 x 3840, one launch, n = 1: sum_x = h w (w - 1) / 2 = 15 921 100 800 does not fit 32 bits."""
    h, w = 2160, 3840
    nh, nw = M.resized(h, w, 1024)
    buf, mask, off = _guarded_mask(1, h, w, cuda)
    st = _mask_post_into(M.made_low("full").to(cuda), 1024, nh, nw, h, w, mask).cpu().numpy()
    want = M.full_stats(h, w)
    assert want[1] > 2 ** 32 and want[2] > 2 ** 32
    assert st[0, :7].tolist() == want and st[0, 7] == 0, (st[0].tolist(), want)
    assert bool((mask == 1).all())
    _check_guards(buf, off, h * w)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refusal_cases():
    # (id, n, L, T, nh, nw, h, w)
    return [("nh > T", 3, 256, 1024, 1025, 1024, 97, 130), ("T < L", 3, 256, 128, 96, 128, 97, 130),
            ("n = 65536", 65536, 256, 1024, 764, 1024, 97, 130), ("h = 0", 3, 256, 1024, 764, 1024, 0, 130)]


@pytest.mark.parametrize("entry", ["lmx_k_mask_post", "lmx_k_mask_logits", "lmx_k_mask_score"])
def test_bad_geometry_is_refused_and_nothing_is_written(cuda, entry):
    """LMX_EINVAL naming the entry point; every output keeps its sentinel."""
    lib = _lib()
    low = M.fixture((97, 130, 256, 1024)).to(cuda)
    for cid, n, L, T, nh, nw, h, w in _refusal_cases():
        mask = torch.full((3 * 97 * 130,), GUARD, dtype=torch.uint8, device=cuda)
        stats = torch.full((3, 8), -77, dtype=torch.int64, device=cuda)
        ws = torch.full((3 * 1025 * 1024,), -3.0, dtype=torch.float32, device=cuda)
        out = torch.full((3 * 97 * 130,), -3.0, dtype=torch.float32, device=cuda)
        if entry == "lmx_k_mask_post":
            rc = lib.lmx_k_mask_post(_p(low), n, L, T, nh, nw, h, w, _p(mask), _p(stats), _p(ws), _stream(cuda))
        elif entry == "lmx_k_mask_logits":
            rc = lib.lmx_k_mask_logits(_p(low), n, L, T, nh, nw, h, w, _p(out), _stream(cuda))
        else:
            rc = lib.lmx_k_mask_score(_p(low), n, L, T, nh, nw, h, w, 0.0, 1.0, None, _p(stats), _stream(cuda))
        msg = lib.lmx_last_error().decode()
        assert rc == EINVAL and entry + ":" in msg, (cid, rc, msg)
        torch.cuda.synchronize()
        assert bool((mask == GUARD).all()) and bool((stats == -77).all()) and bool((ws == -3.0).all()) and bool((out == -3.0).all()), cid


def test_mask_logits_refuses_an_output_that_is_not_16_byte_aligned(cuda):
    lib = _lib()
    h, w = 97, 130
    nh, nw = M.resized(h, w, 1024)
    low = M.fixture((97, 130, 256, 1024)).to(cuda)
    out = torch.full((3 * h * w + 4,), -3.0, dtype=torch.float32, device=cuda)
    assert out.data_ptr() % 16 == 0
    rc = lib.lmx_k_mask_logits(_p(low), 3, 256, 1024, nh, nw, h, w, _p(out, 4), _stream(cuda))
    msg = lib.lmx_last_error().decode()
    assert rc == EINVAL and "lmx_k_mask_logits:" in msg and "align" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


# ---------------------------------------------------------------------------------------------------------------- hyper_mask
HYPER = [(2, 5, 8), (1, 16, 32), (9, 64, 64)]  # the last: 9 * 64 * 64 * 16 threads > 2048 * 256, a second grid-stride pass
_HYPER_REF = {}


def _hyper_case(n, G, C_):
    key = (n, G, C_)
    if key not in _HYPER_REF:
        g = torch.Generator().manual_seed(100 * n + C_)
        up = (torch.randn(n, G, G, 2, 2, 2, 2, C_, generator=g) * 0.7).half()
        hyper = torch.randn(n, 4, C_, generator=g)
        ref, mag = M.hyper_mask(up, hyper)
        swapped, _ = M.hyper_mask(up.permute(0, 1, 2, 5, 6, 3, 4, 7), hyper)
        _HYPER_REF[key] = (up, hyper, ref, M.hyper_mask_bound(mag, C_), swapped)
    return _HYPER_REF[key]


@pytest.mark.parametrize("M_", [1, 4], ids=["M1", "M4"])
@pytest.mark.parametrize("shape", HYPER, ids=[f"n{n}-G{G}-C{c}" for n, G, c in HYPER])
def test_hyper_mask_matches_float64(cuda, shape, M_):
    """f16 `up` against float64 within (C + 1) 2^-24 sum_c |up_c hyper_c| (a C-term f32 fma chain), every cell written (NaN
    sentinel); the reference with (dy1, dx1) and (dy2, dx2) exchanged misses that bound by >= 100 x on the same launch.
    M = 1 runs lmx_k_hyper_mask and lmx_k_hyper_mask_multi, M = 4 lmx_k_hyper_mask_multi."""
    n, G, C_ = shape
    lib = _lib()
    up, hyper, ref, bound, swapped = _hyper_case(n, G, C_)
    d_up = up.to(cuda)
    hy = hyper[:, :M_].contiguous().to(cuda)
    launches = [("hyper_mask_multi", lambda o: lib.lmx_k_hyper_mask_multi(_p(d_up), _p(hy), _p(o), n, M_, G, C_, _stream(cuda)))]
    if M_ == 1:
        launches.append(("hyper_mask", lambda o: lib.lmx_k_hyper_mask(_p(d_up), _p(hy), _p(o), n, G, C_, _stream(cuda))))
    for name, launch in launches:
        out = torch.full((n, M_, 4 * G, 4 * G), float("nan"), dtype=torch.float32, device=cuda)
        assert launch(out) == 0, lib.lmx_last_error().decode()
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} cells were not written"
        r = float(((got - ref[:, :M_]).abs() / bound[:, :M_]).max())
        teeth = float(((got - swapped[:, :M_]).abs() / bound[:, :M_]).max())
        print(f"{name} n={n} G={G} C={C_} M={M_}: {_lg(r)} of the bound; quadrant levels exchanged: {teeth:.3g} x the bound")
        assert r <= 1.0, (name, r)
        assert teeth >= 100, (name, teeth)


# ------------------------------------------------------------------------------------------------------------------ the chain
def test_chain_at_an_odd_width(cuda):
    """333 x 517, n = 3: mask -> pack_bits == numpy.packbits; statistics + contour features == the host's feature extraction."""
    from lmx import kernels as K
    from lmx.services.sam3_pipeline import extract_segmentation_features, features_from_device

    geo = (333, 517, 256, 1024)
    h, w, L, T = geo
    nh, nw = M.resized(h, w, T)
    mask, stats = K.mask_post(M.fixture(geo).to(cuda), T, nh, nw, h, w)
    bits = K.pack_bits(mask)
    cont = K.contour_features(mask)
    torch.cuda.synchronize()
    mh, sh, ch = mask.cpu().numpy(), stats.cpu().numpy(), cont.cpu().numpy()
    assert bits.shape == (3, h, (w + 7) // 8) and np.array_equal(bits.cpu().numpy(), np.packbits(mh, axis=-1))
    for i in range(3):
        assert features_from_device(sh[i], ch[i], h, w) == extract_segmentation_features(mh[i]), i
