"""The TCN gait model on the GPU (csrc/tcn.hip, csrc/gait_model.hip; include/lmx.h "The TCN gait model"): one launch for n clips and S
MC-dropout samples, against tcnref in float64 with the same keep bits under the tolerance rule of tcnref.tolerances, and the properties
that need no reference — causality, no leak from padding, independence of the batch and of S, stats from pred, untouched guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

import tcnref
from lmx import checkpoints, native, tcn
from lmx import kernels as K

pytestmark = pytest.mark.gpu

# every 16-row tile boundary the three kernel instantiations (1, 2, 4 tiles per wave) see, the receptive field 61 and the limit 256
T_BY_CONFIG = {"shipped": (1, 2, 3, 15, 16, 17, 31, 32, 33, 60, 61, 62, 125, 127, 128, 129, 256), "tiny": (1, 7, 33), "deep": (5, 125)}
S_VALUES = (0, 2, 10)
FILL = 0x7FC0DEAD  # a NaN with a recognisable payload


@pytest.fixture(scope="module")
def models(cuda):
    out = {}
    for i, (name, cfg) in enumerate(tcnref.CONFIGS.items()):
        _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 21 + i), cfg.dropout)
        out[name] = (cfg, folded, tcn.TcnScorer(cfg, folded, device=cuda), tcn.TcnScorer(cfg, folded, backend="host"))
    return out


@pytest.fixture(scope="module")
def cases(models):
    """(configuration, T, S) with n = 3 clips each; the float64 and float32 references are computed once and never changed"""
    return [tcnref.make_case(f"{name}-T{T}-S{S}", models[name][0], models[name][1], T, S, n=3)
            for name, Ts in T_BY_CONFIG.items() for T in Ts for S in S_VALUES]


def test_device_and_host_forward_against_float64(cuda, models, cases):
    tol_trunk, tol_pred, e_trunk, e_pred = tcnref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases: trunk {e_trunk:.3g} (relative to max |trunk|), pred {e_pred:.3g}")
    worst = {"device": [0.0, 0.0], "host": [0.0, 0.0]}
    for case in cases:
        _, _, dev, host = models[case.name.split("-")[0]]
        pred, stats, trunk = dev.forward(case.x.to(cuda), case.seeds, case.S, trunk=True)
        hpred, _, htrunk = host.forward(case.x, case.seeds, case.S, trunk=True)
        for who, t, p in (("device", trunk, pred), ("host", htrunk, hpred)):
            rt, rp = tcnref.check_case(case, t, p, tol_trunk, tol_pred, who)
            worst[who] = [max(worst[who][0], rt), max(worst[who][1], rp)]
        tcnref.check_stats(pred, stats, case.S)
    print("worst error / bound:", worst)


def _clip(cfg, T, seed, n=1):
    return torch.randn((n, T, cfg.input_dim), generator=torch.Generator().manual_seed(seed))


def test_causality(cuda, models):
    cfg, _, dev, _ = models["shipped"]
    x = _clip(cfg, 125, 1, n=2).to(cuda)
    seeds = [5, 6]
    for S in (0, 3):
        _, _, base = dev.forward(x, seeds, S, trunk=True)
        for t0 in (1, 61, 124):
            y = x.clone()
            y[:, t0:, :] = torch.randn((2, 125 - t0, cfg.input_dim), generator=torch.Generator().manual_seed(t0)).to(cuda)
            _, _, tr = dev.forward(y, seeds, S, trunk=True)
            assert torch.equal(tr[:, :, :t0], base[:, :, :t0]), (S, t0)
            assert not torch.equal(tr[:, :, t0:], base[:, :, t0:])


def _raw_forward(scorer, x, seeds, S, pred, stats, trunk):
    """lmx_k_tcn_forward into the caller's own buffers"""
    lib = native._lib.load()
    n, T = x.shape[:2]
    sd = np.array(seeds, np.uint64)
    ws = torch.empty((max(n, 1),), dtype=torch.int64, device=x.device)
    K.check(lib.lmx_k_tcn_forward(C.byref(scorer.weights), C.c_void_p(x.data_ptr()), C.c_void_p(sd.ctypes.data), n, T, S, scorer.cfg.dropout,
                                  C.c_void_p(pred.data_ptr()), C.c_void_p(stats.data_ptr()), C.c_void_p(trunk.data_ptr() if trunk is not None else 0),
                                  C.c_void_p(ws.data_ptr()), K._stream(x.device)), "lmx_k_tcn_forward")


def test_padding_does_not_leak_and_guard_words_hold(cuda, models):
    """T = 125 is no multiple of the 16-row tile: the rows 125 .. 127 of the tiles exist in LDS only.  Nothing outside [n][S][T][C] of
    trunk, [n][S] of pred and [n][2] of stats is written, whatever they held before, and the words around x are never read into a result."""
    cfg, _, dev, _ = models["shipped"]
    n, T, S, Cc, G = 2, 125, 3, cfg.channels[-1], 512
    seeds = [11, 12]
    x = _clip(cfg, T, 3, n=n)
    results = []
    for fill_byte in (0x00, 0xFF):
        xb = torch.full((G + x.numel() + G,), 0, dtype=torch.float32, device=cuda)
        xb.view(torch.uint8).fill_(fill_byte)
        xin = xb[G:G + x.numel()].view(n, T, cfg.input_dim)
        xin.copy_(x)
        bufs = {}
        for name, count in (("pred", n * S), ("stats", n * 2), ("trunk", n * S * T * Cc)):
            b = torch.full((G + count + G,), FILL, dtype=torch.int32, device=cuda)
            bufs[name] = (b, b[G:G + count].view(torch.float32))
        _raw_forward(dev, xin, seeds, S, bufs["pred"][1], bufs["stats"][1], bufs["trunk"][1])
        for name, (b, inner) in bufs.items():
            assert bool((b[:G] == FILL).all()) and bool((b[G + inner.numel():] == FILL).all()), name
            assert bool(torch.isfinite(inner).all()), name  # every word inside is written: stats and pred do not depend on what they held
        results.append({k: v[1].clone() for k, v in bufs.items()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    pred, stats, trunk = dev.forward(x.to(cuda), seeds, S, trunk=True)
    assert torch.equal(pred.flatten(), results[0]["pred"]) and torch.equal(stats.flatten(), results[0]["stats"])
    assert torch.equal(trunk.flatten(), results[0]["trunk"])


def test_a_clip_does_not_depend_on_its_batch_or_on_S(cuda, models):
    for name, T in (("shipped", 125), ("tiny", 33)):
        cfg, _, dev, _ = models[name]
        clip, others = _clip(cfg, T, 7), _clip(cfg, T, 8, n=2)
        alone = dev.forward(clip.to(cuda), [99], 10, trunk=True)
        for pos in range(3):
            rows = list(others)
            rows.insert(pos, clip[0])
            seeds = [1, 2]
            seeds.insert(pos, 99)
            pred, stats, trunk = dev.forward(torch.stack(rows).to(cuda), seeds, 10, trunk=True)
            assert torch.equal(pred[pos], alone[0][0]) and torch.equal(stats[pos], alone[1][0]) and torch.equal(trunk[pos], alone[2][0]), (name, pos)
        p4, _, t4 = dev.forward(clip.to(cuda), [99], 4, trunk=True)
        assert torch.equal(p4[0], alone[0][0, :4]) and torch.equal(t4[0], alone[2][0, :4])
        # another seed is another draw
        assert not torch.equal(dev.forward(clip.to(cuda), [98], 10)[0], alone[0])


def test_native_handle_gives_the_scorers_bits(cuda, models, tmp_path):
    cfg, folded, dev, _ = models["shipped"]
    path = tmp_path / "tcn.lmx"
    native.write_tcn_image(cfg, folded, path)
    x, seeds = _clip(cfg, 125, 9, n=3), [tcn.clip_seed(v) for v in ("a", "b", "c")]
    with native.NativeTcn(path, max_clips=4, max_samples=10, device=cuda) as h:
        assert (h.info.input_dim, h.info.n_blocks, h.info.receptive_field, h.info.max_clips, h.info.max_samples) == (44, 4, 61, 4, 10)
        for S in (10, 0):
            mean, std, pred = dev.score(x.to(cuda), seeds, S)
            m1, s1, p1 = h.score(x.to(cuda), seeds, S)
            m2, s2, p2 = h.score_host(x.numpy(), seeds, S)
            assert torch.equal(p1, pred) and torch.equal(m1, mean) and torch.equal(s1, std)
            assert np.array_equal(p2, pred.cpu().numpy()) and np.array_equal(m2, mean.cpu().numpy()) and np.array_equal(s2, std.cpu().numpy())
        with pytest.raises(K.LmxError, match="n = 5"):
            h.score(_clip(cfg, 8, 1, n=5).to(cuda), [1] * 5)
        with pytest.raises(K.LmxError, match="S = 11"):
            h.score(x.to(cuda), seeds, 11)
        with pytest.raises(K.LmxError, match="S 1"):
            h.score(x.to(cuda), seeds, 1)
    torch.cuda.synchronize(cuda)


def test_zero_clips_and_refusals(cuda, models):
    cfg, _, dev, _ = models["shipped"]
    x = _clip(cfg, 16, 2, n=2).to(cuda)
    pred, stats, _ = dev.forward(x[:0], [], 10)
    assert tuple(pred.shape) == (0, 10) and tuple(stats.shape) == (0, 2)
    with pytest.raises(K.LmxError, match="CPU tensor"):
        dev.forward(x.cpu(), [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x.double(), [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x[:, ::2], [1, 2], 10)
    with pytest.raises(K.LmxError, match="contiguous float32"):
        dev.forward(x[..., :40].contiguous(), [1, 2], 10)
    with pytest.raises(K.LmxError, match="T 257"):
        dev.forward(torch.zeros((1, 257, cfg.input_dim), device=cuda), [1], 10)
    with pytest.raises(K.LmxError, match="S 1"):
        dev.forward(x, [1, 2], 1)
    with pytest.raises(K.LmxError, match="seeds"):
        dev.forward(x, [1], 10)
    with pytest.raises(K.LmxError, match="HOST memory"):
        dev.forward(x, torch.tensor([1, 2], device=cuda), 10)
    with pytest.raises(K.LmxError, match=r"channels\[0\] = 24"):
        K.tcn_weights(44, (24,), 3, 32, dev.tensors)
    with pytest.raises(K.LmxError, match="k 4"):
        K.tcn_weights(44, (64,), 4, 32, dev.tensors)
    torch.cuda.synchronize(cuda)


def test_spread_agrees_with_torchs_generator(cuda, models):
    """Parity with torch's generator is statistical: tcnref under 2000 draws of torch.bernoulli masks (what nn.Dropout draws in train
    mode) against the device's mean over S = 200 of the library's own bits.  5 standard errors of a mean of 200, from the torch run's
    own standard deviation."""
    cfg, folded, dev, _ = models["shipped"]
    x = _clip(cfg, 125, 4)
    g = torch.Generator().manual_seed(0)
    preds = torch.cat([tcnref.forward(cfg, folded, x.expand(500, -1, -1), tcnref.bernoulli_keeps(cfg, 125, 500, g), torch.float32)[1]
                       for _ in range(4)]).double()
    mean, std = float(preds.mean()), float(preds.std())
    got_mean, got_std, _ = dev.score(x.to(cuda), [tcn.clip_seed("clip")], 200)
    se = std / 200 ** 0.5
    print(f"torch: mean {mean:.5f} std {std:.5f} over 2000; device: mean {float(got_mean[0]):.5f} std {float(got_std[0]):.5f} over 200; se {se:.5f}")
    assert std > 0 and abs(float(got_mean[0]) - mean) <= 5 * se
