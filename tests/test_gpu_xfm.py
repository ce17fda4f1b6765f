"""The gait transformer on the GPU (csrc/xfm.hip, csrc/gait_model.hip; include/lmx.h "The gait transformer"): one launch for n clips and
S MC-dropout samples, against xfmref in float64 with the same keep bits under the tolerance rule of xfmref.tolerances, and the
properties that need no reference — the saliency's sum, masked steps that reach nothing, independence of the batch and of S, stats from
pred, untouched guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import xfmref
from lmx import checkpoints, native, xfm
from lmx import kernels as K
from tcnref import check_stats

pytestmark = pytest.mark.gpu

T_BY_CONFIG, S_VALUES = xfmref.T_BY_CONFIG, xfmref.S_VALUES
FILL = 0x7FC0DEAD  # a NaN with a recognisable payload


@pytest.fixture(scope="module")
def models(cuda):
    out = {}
    for i, (name, cfg) in enumerate(xfmref.CONFIGS.items()):
        got, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(cfg, 21 + i), n_heads=cfg.n_heads, dropout=cfg.dropout)
        assert got == cfg
        out[name] = (cfg, w, xfm.XfmScorer(cfg, w, device=cuda), xfm.XfmScorer(cfg, w, backend="host"))
    return out


@pytest.fixture(scope="module")
def cases(models):
    """(configuration, T, S) with n = 3 clips each (unmasked, 30 % masked at random, masked at both ends) and one case per configuration
    whose clips have a single unmasked step; the float64 and float32 references are computed once and never changed"""
    out = [xfmref.make_case(f"{name}-T{T}-S{S}", models[name][0], models[name][1], T, S, n=3)
           for name, Ts in T_BY_CONFIG.items() for T in Ts for S in S_VALUES]
    out += [xfmref.make_case(f"{name}-single-T{T}-S{S}", models[name][0], models[name][1], T, S, n=3, single=True)
            for name, T, S in (("shipped", 125, 0), ("tiny", 33, 2), ("wide", 160, 0))]
    return out


def test_device_and_host_forward_against_float64(cuda, models, cases):
    tols = xfmref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases: trunk {tols[3]:.3g}, saliency {tols[5]:.3g} (relative to the case's max), pred {tols[4]:.3g}")
    worst = {"device": [0.0, 0.0, 0.0], "host": [0.0, 0.0, 0.0]}
    for case in cases:
        _, _, dev, host = models[case.name.split("-")[0]]
        sal = case.S == 0
        pred, stats, s, trunk = dev.forward(case.x.to(cuda), case.mask.to(cuda), case.seeds, case.S, trunk=True, saliency=sal)
        hpred, _, hs, htrunk = host.forward(case.x, case.mask, case.seeds, case.S, trunk=True, saliency=sal)
        for who, t, p, sl in (("device", trunk, pred, s), ("host", htrunk, hpred, hs)):
            ratios = xfmref.check_case(case, t, p, sl, tols, who)
            worst[who] = [max(a, b) for a, b in zip(worst[who], ratios)]
        check_stats(pred, stats, case.S)
    print("worst error / bound (trunk, pred, saliency):", worst)


def _clip(cfg, T, seed, n=1):
    return torch.randn((n, T, cfg.input_dim), generator=torch.Generator().manual_seed(seed))


def _mask(n, T, seed):
    return xfmref.make_masks(n, T, torch.Generator().manual_seed(seed)).to(torch.uint8)


def test_saliency_sums_to_T(cuda, models):
    """Every row of P sums to 1, so the column sums of the head average add up to T — masked or not."""
    for name, T in (("shipped", 125), ("shipped", 150), ("tiny", 33), ("wide", 160)):
        cfg, _, dev, _ = models[name]
        x = _clip(cfg, T, 5, n=3).to(cuda)
        for mask in (None, _mask(3, T, 6).to(cuda)):
            sal = dev.forward(x, mask, None, 0, saliency=True)[2].double().cpu()
            assert (sal.sum(1) - T).abs().max() <= T * 2.0 ** -21, (name, T, sal.sum(1))
            if mask is not None:
                assert not sal[mask.cpu().bool()].any()  # a masked step receives no attention at all
        assert torch.equal(dev.saliency(x), dev.forward(x, None, None, 0, saliency=True)[2])


def test_masked_steps_reach_nothing(cuda, models):
    for name, T in (("shipped", 125), ("tiny", 33)):
        cfg, _, dev, _ = models[name]
        x, mask = _clip(cfg, T, 11, n=3), _mask(3, T, 12)
        seeds = [5, 6, 7]
        y = x.clone()
        y[mask.bool()] = torch.randn((int(mask.sum()), cfg.input_dim), generator=torch.Generator().manual_seed(13))
        for S in (0, 3):
            p0, _, _, t0 = dev.forward(x.to(cuda), mask.to(cuda), seeds, S, trunk=True)
            p1, _, _, t1 = dev.forward(y.to(cuda), mask.to(cuda), seeds, S, trunk=True)
            live = ~mask.bool().to(cuda)
            assert torch.equal(p0, p1), (name, S)
            for i in range(3):
                assert torch.equal(t0[i][:, live[i]], t1[i][:, live[i]]), (name, S, i)
            assert not torch.equal(t0, t1)  # masked steps are computed as queries, and trunk shows them


def test_a_mask_of_zeros_is_no_mask_and_an_all_masked_clip_is_nan(cuda, models):
    cfg, _, dev, host = models["shipped"]
    x = _clip(cfg, 125, 17, n=3)
    a = dev.forward(x.to(cuda), None, None, 0, trunk=True, saliency=True)
    b = dev.forward(x.to(cuda), torch.zeros((3, 125), dtype=torch.uint8, device=cuda), None, 0, trunk=True, saliency=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    mask = torch.zeros((3, 125), dtype=torch.uint8)
    mask[1] = 1
    for S in (0, 4):
        pred, stats, _, _ = dev.forward(x.to(cuda), mask.to(cuda), [1, 2, 3], S)
        alone = [dev.forward(x[i:i + 1].to(cuda), None, [[1, 2, 3][i]], S)[0] for i in (0, 2)]
        assert bool(torch.isnan(pred[1]).all()) and bool(torch.isnan(stats[1, 0]))
        assert torch.equal(pred[0], alone[0][0]) and torch.equal(pred[2], alone[1][0])
        assert bool(torch.isnan(host.forward(x, mask, [1, 2, 3], S)[0][1]).all())


def _raw_forward(scorer, x, mask, seeds, S, pred, stats, sal, trunk):
    """lmx_k_xfm_forward into the caller's own buffers"""
    lib = native._lib.load()
    n, T = x.shape[:2]
    sd = np.array(seeds, np.uint64)
    ws = torch.empty((max(n, 1),), dtype=torch.int64, device=x.device)
    K.check(lib.lmx_k_xfm_forward(C.byref(scorer.weights), K._ptr(x), K._ptr(mask), C.c_void_p(sd.ctypes.data), n, T, S, scorer.cfg.dropout,
                                  K._ptr(pred), K._ptr(stats), K._ptr(sal), K._ptr(trunk), K._ptr(ws), K._stream(x.device)), "lmx_k_xfm_forward")


def test_padding_does_not_leak_and_guard_words_hold(cuda, models):
    """T = 125 is no multiple of the 16-row tile: the rows 125 .. 127 of the tiles exist in LDS only.  Nothing outside pred, stats,
    saliency and trunk is written, whatever they held before, every word inside is, and the bytes around x and mask reach no result."""
    cfg, _, dev, _ = models["shipped"]
    n, T, D, G = 2, 125, cfg.d_model, 512
    seeds = [11, 12]
    x, mask = _clip(cfg, T, 3, n=n), _mask(3, T, 4)[1:]
    for S in (3, 0):
        results = []
        for fill_byte in (0x00, 0xFF):
            xb = torch.full((G + x.numel() + G,), 0, dtype=torch.float32, device=cuda)
            xb.view(torch.uint8).fill_(fill_byte)
            xin = xb[G:G + x.numel()].view(n, T, cfg.input_dim)
            xin.copy_(x)
            mb = torch.full((G + n * T + G,), fill_byte, dtype=torch.uint8, device=cuda)
            min_ = mb[G:G + n * T].view(n, T)
            min_.copy_(mask)
            bufs = {}
            for name, count in (("pred", n * max(S, 1)), ("stats", n * 2), ("trunk", n * max(S, 1) * T * D)) + ((("sal", n * T),) if S == 0 else ()):
                b = torch.full((G + count + G,), FILL, dtype=torch.int32, device=cuda)
                bufs[name] = (b, b[G:G + count].view(torch.float32))
            _raw_forward(dev, xin, min_, seeds, S, bufs["pred"][1], bufs["stats"][1], bufs["sal"][1] if S == 0 else None, bufs["trunk"][1])
            for name, (b, inner) in bufs.items():
                assert bool((b[:G] == FILL).all()) and bool((b[G + inner.numel():] == FILL).all()), name
                assert bool(torch.isfinite(inner).all()), name  # every word inside is written
            results.append({k: v[1].clone() for k, v in bufs.items()})
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), k
        pred, stats, sal, trunk = dev.forward(x.to(cuda), mask.to(cuda), seeds, S, trunk=True, saliency=S == 0)
        assert torch.equal(pred.flatten(), results[0]["pred"]) and torch.equal(stats.flatten(), results[0]["stats"])
        assert torch.equal(trunk.flatten(), results[0]["trunk"]) and (S or torch.equal(sal.flatten(), results[0]["sal"]))


def test_a_clip_does_not_depend_on_its_batch_or_on_S(cuda, models):
    for name, T in (("shipped", 125), ("tiny", 33), ("wide", 160)):
        cfg, _, dev, _ = models[name]
        clip, others = _clip(cfg, T, 7), _clip(cfg, T, 8, n=2)
        masks = _mask(3, T, 9)
        cm, om = masks[1:2], masks[[0, 2]]
        alone = dev.forward(clip.to(cuda), cm.to(cuda), [99], 10, trunk=True)
        alone0 = dev.forward(clip.to(cuda), cm.to(cuda), None, 0, saliency=True)
        for pos in range(3):
            rows, mrows, seeds = list(others), list(om), [1, 2]
            rows.insert(pos, clip[0]), mrows.insert(pos, cm[0]), seeds.insert(pos, 99)
            xb, mb = torch.stack(rows).to(cuda), torch.stack(mrows).to(cuda)
            pred, stats, _, trunk = dev.forward(xb, mb, seeds, 10, trunk=True)
            assert torch.equal(pred[pos], alone[0][0]) and torch.equal(stats[pos], alone[1][0]) and torch.equal(trunk[pos], alone[3][0]), (name, pos)
            pred0, _, sal0, _ = dev.forward(xb, mb, None, 0, saliency=True)
            assert torch.equal(pred0[pos], alone0[0][0]) and torch.equal(sal0[pos], alone0[2][0]), (name, pos)
        p4, _, _, t4 = dev.forward(clip.to(cuda), cm.to(cuda), [99], 4, trunk=True)
        assert torch.equal(p4[0], alone[0][0, :4]) and torch.equal(t4[0], alone[3][0, :4])
        assert not torch.equal(dev.forward(clip.to(cuda), cm.to(cuda), [98], 10)[0], alone[0])  # another seed is another draw


def test_native_handle_gives_the_scorers_bits(cuda, models, tmp_path):
    cfg, w, dev, _ = models["shipped"]
    path = tmp_path / "xfm.lmx"
    native.write_xfm_image(cfg, w, path)
    x, mask, seeds = _clip(cfg, 125, 9, n=3), _mask(3, 125, 10), [xfm.clip_seed(v) for v in ("a", "b", "c")]
    with native.NativeXfm(path, max_clips=4, max_samples=10, device=cuda) as h:
        i = h.info
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.ff, i.head, i.max_len, i.max_clips, i.max_samples) == (44, 64, 4, 4, 256, 32, 150, 4, 10)
        for S in (10, 0):
            pred, stats, sal, _ = dev.forward(x.to(cuda), mask.to(cuda), seeds, S, saliency=S == 0)
            m1, s1, p1, a1 = h.score(x.to(cuda), mask.to(cuda), seeds, S, saliency=S == 0)
            m2, s2, p2, a2 = h.score_host(x.numpy(), mask.numpy(), seeds, S, saliency=S == 0)
            assert torch.equal(p1, pred) and torch.equal(m1, stats[:, 0]) and torch.equal(s1, stats[:, 1])
            assert np.array_equal(p2, pred.cpu().numpy()) and np.array_equal(m2, stats[:, 0].cpu().numpy()) and np.array_equal(s2, stats[:, 1].cpu().numpy())
            if S == 0:
                assert torch.equal(a1, sal) and np.array_equal(a2, sal.cpu().numpy())
        with pytest.raises(K.LmxError, match="n = 5"):
            h.score(_clip(cfg, 8, 1, n=5).to(cuda), None, [1] * 5)
        with pytest.raises(K.LmxError, match="S = 11"):
            h.score(x.to(cuda), None, seeds, 11)
        with pytest.raises(K.LmxError, match="S 1"):
            h.score(x.to(cuda), None, seeds, 1)
        with pytest.raises(K.LmxError, match="saliency"):
            h.score(x.to(cuda), None, seeds, 10, saliency=True)
    torch.cuda.synchronize(cuda)


def test_zero_clips_and_refusals(cuda, models):
    cfg, _, dev, _ = models["shipped"]
    x = _clip(cfg, 16, 2, n=2).to(cuda)
    pred, stats, _, _ = dev.forward(x[:0], None, [], 10)
    assert tuple(pred.shape) == (0, 10) and tuple(stats.shape) == (0, 2)
    with pytest.raises(K.LmxError, match="CPU tensor"):
        dev.forward(x.cpu(), None, [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x.double(), None, [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x[:, ::2], None, [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x[..., :40].contiguous(), None, [1, 2], 10)
    with pytest.raises(K.LmxError, match="T 151"):
        dev.forward(torch.zeros((1, 151, cfg.input_dim), device=cuda), None, [1], 10)
    with pytest.raises(K.LmxError, match="S 1"):
        dev.forward(x, None, [1, 2], 1)
    with pytest.raises(K.LmxError, match="saliency"):
        dev.forward(x, None, [1, 2], 10, saliency=True)
    with pytest.raises(K.LmxError, match="mask"):
        dev.forward(x, torch.zeros((2, 16), dtype=torch.uint8), [1, 2], 10)
    with pytest.raises(K.LmxError, match="seeds"):
        dev.forward(x, None, [1], 10)
    with pytest.raises(K.LmxError, match="HOST memory"):
        dev.forward(x, None, torch.tensor([1, 2], device=cuda), 10)
    for field, bad, match in (("d_model", 24, "d_model 24"), ("n_heads", 8, "n_heads 8"), ("ff", 40, "ff 40"), ("max_len", 161, "max_len 161"),
                              ("n_layers", 9, "n_layers 9"), ("head", 65, "head 65"), ("input_dim", 65, "input_dim 65")):
        shape = dict(zip(("input_dim", "d_model", "n_heads", "n_layers", "ff", "head", "max_len"), cfg.shape()))
        shape[field] = bad
        with pytest.raises(K.LmxError, match=match):
            K.xfm_weights(*shape.values(), dev.tensors)
    # the library itself refuses what the Python checks refuse: a struct with a bad field goes straight to the entry point
    w = type(dev.weights).from_buffer_copy(dev.weights)
    w.ff = 40
    pred, stats = torch.empty((2, 1), device=cuda), torch.empty((2, 2), device=cuda)
    rc = native._lib.load().lmx_k_xfm_forward(C.byref(w), K._ptr(x), None, None, 2, 16, 0, 0.1, K._ptr(pred), K._ptr(stats), None, None, None,
                                              K._stream(cuda))
    assert rc != 0 and "ff 40" in native._lib.load().lmx_last_error().decode()
    torch.cuda.synchronize(cuda)


def test_spread_agrees_with_torchs_generator(cuda, models):
    """Parity with torch's generator is statistical: xfmref in float32 under 2000 draws of torch.bernoulli masks (what nn.Dropout draws
    in train mode), with a random mask on the clip, against the device's mean over S = 200 of the library's own bits.  5 standard errors of
    a mean of 200, from the torch run's own standard deviation."""
    cfg, w, dev, _ = models["shipped"]
    x, mask = _clip(cfg, 125, 4), _mask(2, 125, 5)[1:]
    g = torch.Generator().manual_seed(0)
    preds = torch.cat([xfmref.forward(cfg, w, x.expand(250, -1, -1), mask.bool().expand(250, -1), xfmref.bernoulli_keeps(cfg, 125, 250, g),
                                      torch.float32)[1] for _ in range(8)]).double()
    mean, std = float(preds.mean()), float(preds.std())
    got_mean, got_std, _ = dev.score(x.to(cuda), mask.to(cuda), [xfm.clip_seed("clip")], 200)
    se = std / 200 ** 0.5
    print(f"torch: mean {mean:.5f} std {std:.5f} over 2000; device: mean {float(got_mean[0]):.5f} std {float(got_std[0]):.5f} over 200; se {se:.5f}")
    assert std > 0 and abs(float(got_mean[0]) - mean) <= 5 * se
