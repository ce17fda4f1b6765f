"""The gait transformer without a GPU (include/lmx.h "The gait transformer"; csrc/host_xfm.cpp, csrc/host_xfm_image.cpp, lmx/xfm.py,
lmx/services/transformer_pipeline.py):
  * xfmref in eval mode against freshly written torch modules (nn.MultiheadAttention, nn.LayerNorm, nn.Linear) with the test's own wiring;
  * lmx_h_xfm_forward against xfmref in float64 under the tolerance rule of xfmref.tolerances; the element order of every dropout site;
  * xfm_from_state_dict: every key, a missing positional table, the refusals;
  * lmx_h_xfm_mask against TransformerPipeline's mask; an all-masked clip;
  * the weight image: write, check, refusals with the field named;
  * TransformerPipeline on InProcessBus with the host backend."""
import asyncio
import json
import struct

import numpy as np
import pytest
import torch
from torch import nn

import xfmref
from lmx import checkpoints, native, xfm
from lmx import kernels as K
from lmx.services import TransformerPipeline
from lmx.services.runtime import InProcessBus


@pytest.fixture(scope="module")
def models():
    out = {}
    for i, (name, cfg) in enumerate(xfmref.CONFIGS.items()):
        sd = xfmref.state_dict(cfg, 31 + i)
        got, w = checkpoints.xfm_from_state_dict(sd, n_heads=cfg.n_heads, dropout=cfg.dropout)
        assert got == cfg
        out[name] = (cfg, w, xfm.XfmScorer(cfg, w, backend="host"), sd)
    return out


# ---- the yardstick itself ----------------------------------------------------------------------------------------------------------
class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(cfg.d_model, cfg.n_heads, batch_first=True)
        self.ffn = nn.Sequential(nn.Linear(cfg.d_model, cfg.ff), nn.GELU(), nn.Identity(), nn.Linear(cfg.ff, cfg.d_model))
        self.norm1, self.norm2 = nn.LayerNorm(cfg.d_model), nn.LayerNorm(cfg.d_model)


class _Modules(nn.Module):
    """The network of the header wired from torch's own modules; attribute names are chosen so that the state_dict loads strictly."""

    def __init__(self, cfg):
        super().__init__()
        self.input_projection = nn.Linear(cfg.input_dim, cfg.d_model)
        self.encoder_layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.n_layers)])
        self.final_norm = nn.LayerNorm(cfg.d_model)
        self.classifier = nn.Sequential(nn.Linear(cfg.d_model, cfg.head), nn.ReLU(), nn.Identity(), nn.Linear(cfg.head, 1))

    def forward(self, x, pe, mask):
        h = self.input_projection(x) + pe[:x.shape[1]]
        weights = None
        for layer in self.encoder_layers:
            a = layer.norm1(h)
            o, weights = layer.self_attn(a, a, a, key_padding_mask=mask, need_weights=True)  # head-averaged
            h = h + o
            h = h + layer.ffn(layer.norm2(h))
        trunk = self.final_norm(h)
        if mask is None:
            pooled = trunk.mean(1)
        else:
            live = (~mask).unsqueeze(-1).float()
            pooled = (trunk * live).sum(1) / live.sum(1).clamp(min=1)
        return trunk, torch.sigmoid(self.classifier(pooled))[:, 0], weights


@pytest.mark.parametrize("name", list(xfmref.CONFIGS))
def test_xfmref_equals_torchs_modules(models, name):
    cfg, w, _, sd = models[name]
    net = _Modules(cfg).eval()
    net.load_state_dict({k: v for k, v in sd.items() if k != "pos_encoder.pe"}, strict=True)
    T = min(37, cfg.max_len)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, T, cfg.input_dim), generator=g)
    for mask in (None, xfmref.make_masks(3, T, g)):
        with torch.no_grad():
            trunk, pred, weights = net(x, sd["pos_encoder.pe"][0], mask)
        t, p, s = xfmref.forward(cfg, w, x, mask, None, torch.float32)
        assert (t - trunk).abs().max() <= 1e-6 * float(trunk.abs().max()) and (p - pred).abs().max() <= 1e-6
        assert (s - weights.sum(1)).abs().max() <= 1e-6 * float(weights.sum(1).abs().max())
        assert (s.sum(1) - T).abs().max() <= T * 2.0 ** -21


# ---- the host forward ----------------------------------------------------------------------------------------------------------------
def test_host_forward_against_float64(models):
    cases = [xfmref.make_case(f"{name}-T{T}-S{S}", models[name][0], models[name][1], T, S, n=3)
             for name, Ts in xfmref.T_BY_CONFIG.items() for T in Ts for S in xfmref.S_VALUES]
    tols = xfmref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases: trunk {tols[3]:.3g}, saliency {tols[5]:.3g} (relative to the case's max), pred {tols[4]:.3g}")
    worst = [0.0, 0.0, 0.0]
    for case in cases:
        host = models[case.name.split("-")[0]][2]
        pred, stats, sal, trunk = host.forward(case.x, case.mask, case.seeds, case.S, trunk=True, saliency=case.S == 0)
        worst = [max(a, b) for a, b in zip(worst, xfmref.check_case(case, trunk, pred, sal, tols, "host"))]
        p = pred.double()
        if case.S:
            assert (stats[:, 0].double() - p.mean(1)).abs().max() <= 4 * 2.0 ** -24 and (stats[:, 1].double() - p.std(1)).abs().max() <= 8 * 2.0 ** -24
        else:
            assert torch.equal(stats[:, 0], pred[:, 0]) and not stats[:, 1].any()
    print("worst error / bound (trunk, pred, saliency):", worst)


def test_every_dropout_site_numbers_its_elements_in_torchs_order(models):
    """With p = 0.02 a site drops a handful of elements.  xfmref with the header's keep arrays, shaped as the table says, agrees with the
    host forward under the rule; with ONE site's array in another element order (transposed, or reversed for a vector) it is off by orders
    of magnitude more: the agreement pins each site's order, one dropped element at a time."""
    cfg0, w, _, _ = models["tiny"]
    cfg = xfm.XfmConfig(**{**cfg0.__dict__, "dropout": 0.02})
    host = xfm.XfmScorer(cfg, w, backend="host")
    T, seed = 23, 0xC0FFEE
    x = torch.randn((1, T, cfg.input_dim), generator=torch.Generator().manual_seed(2))
    pred, _, _, trunk = host.forward(x, None, [seed], 2, trunk=True)
    keeps = xfmref.keep_arrays(cfg, T, seed, 1)
    assert len(keeps) == cfg.n_sites == 6
    t64, p64, _ = xfmref.forward(cfg, w, x[0], None, keeps, torch.float64)
    t32, _, _ = xfmref.forward(cfg, w, x[0], None, keeps, torch.float32)
    tol = 4 * float((t32.double() - t64).abs().max())
    assert (trunk[0, 1].double() - t64).abs().max() <= tol and abs(float(pred[0, 1]) - float(p64)) <= 1e-6
    for site in range(cfg.n_sites - 1):
        k = keeps[site]
        assert 0 < int((k == 0).sum()) < k.numel() // 10
        other = list(keeps)
        other[site] = k.transpose(-1, -2).reshape(k.shape) if k.shape[-1] != k.shape[-2] else k.transpose(-1, -2).contiguous()
        assert not torch.equal(other[site], k)
        wrong, _, _ = xfmref.forward(cfg, w, x[0], None, other, torch.float64)
        assert (trunk[0, 1].double() - wrong).abs().max() > 1000 * tol, site
    # the head's site changes the prediction only: p large enough to drop some of its 16 elements
    cfg5 = xfm.XfmConfig(**{**cfg0.__dict__, "dropout": 0.5})
    pred5 = xfm.XfmScorer(cfg5, w, backend="host").forward(x, None, [seed], 2)[0]
    keeps5 = xfmref.keep_arrays(cfg5, T, seed, 1)
    assert 0 < int(keeps5[-1].sum()) < cfg5.head
    assert abs(float(pred5[0, 1]) - float(xfmref.forward(cfg5, w, x[0], None, keeps5, torch.float64)[1])) <= 1e-6
    keeps5[-1] = keeps5[-1].flip(0)
    assert abs(float(pred5[0, 1]) - float(xfmref.forward(cfg5, w, x[0], None, keeps5, torch.float64)[1])) > 1e-4


def test_an_all_masked_clip_is_nan(models):
    cfg, _, host, _ = models["tiny"]
    x = torch.randn((2, 9, cfg.input_dim), generator=torch.Generator().manual_seed(3))
    mask = torch.tensor([[1] * 9, [0] * 9], dtype=torch.uint8)
    for S in (0, 3):
        pred, stats, _, trunk = host.forward(x, mask, [1, 2], S, trunk=True)
        assert bool(torch.isnan(pred[0]).all()) and bool(torch.isnan(stats[0, 0])) and bool(torch.isnan(trunk[0]).all())
        assert bool(torch.isfinite(pred[1]).all()) and bool(torch.isfinite(trunk[1]).all())
        assert torch.equal(pred[1], host.forward(x[1:], None, [2], S)[0][0])


def test_forward_refusals(models):
    cfg, _, host, _ = models["tiny"]
    x = torch.zeros((2, 8, cfg.input_dim))
    with pytest.raises(K.LmxError, match="T 41"):
        host.forward(torch.zeros((1, 41, cfg.input_dim)), None, [1], 2)
    with pytest.raises(K.LmxError, match="S 1"):
        host.forward(x, None, [1, 2], 1)
    with pytest.raises(K.LmxError, match="saliency"):
        host.forward(x, None, [1, 2], 2, saliency=True)
    with pytest.raises(K.LmxError, match="mask"):
        host.forward(x, torch.zeros((2, 7), dtype=torch.uint8), [1, 2], 2)
    with pytest.raises(K.LmxError, match="backend"):
        xfm.XfmScorer(cfg, models["tiny"][1], backend="cpu")
    pred, stats, _, _ = host.forward(x[:0], None, [], 2)
    assert tuple(pred.shape) == (0, 2)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
def test_from_state_dict_reads_every_key_and_refuses_what_the_kernel_refuses(models):
    cfg, w, _, sd = models["shipped"]
    assert cfg == xfm.XfmConfig() and (cfg.n_sites, cfg.head_dim) == (18, 16)
    assert len(w) == 3 + 12 * cfg.n_layers + 6
    assert torch.equal(w["layer.2.qkv.weight"], sd["encoder_layers.2.self_attn.in_proj_weight"]) and torch.equal(w["pe"], sd["pos_encoder.pe"][0])
    assert torch.equal(w["layer.3.ff2.bias"], sd["encoder_layers.3.ffn.3.bias"]) and torch.equal(w["head.fc2.weight"], sd["classifier.3.weight"])
    # without the table: computed once by the reference's formula, the same bits
    cfg2, w2 = checkpoints.xfm_from_state_dict({k: v for k, v in sd.items() if k != "pos_encoder.pe"})
    assert cfg2 == cfg and torch.equal(w2["pe"], w["pe"])
    t = torch.arange(150.0)[:, None] * torch.exp(torch.arange(0, 64, 2).float() * (-np.log(10000.0) / 64))
    assert torch.equal(w2["pe"][:, 0::2], torch.sin(t)) and torch.equal(w2["pe"][:, 1::2], torch.cos(t))
    for key in ("input_projection.bias", "encoder_layers.1.self_attn.in_proj_bias", "encoder_layers.0.ffn.3.weight", "final_norm.weight", "classifier.3.bias"):
        with pytest.raises(K.LmxError, match=key.replace(".", r"\.")):
            checkpoints.xfm_from_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(K.LmxError, match="not a GaitTransformer"):
        checkpoints.xfm_from_state_dict({"network.0.conv1.conv.bias": torch.zeros(4)})
    with pytest.raises(K.LmxError, match="n_heads 8"):
        checkpoints.xfm_from_state_dict(sd, n_heads=8)
    with pytest.raises(K.LmxError, match="p 1.0"):
        checkpoints.xfm_from_state_dict(sd, dropout=1.0)
    with pytest.raises(K.LmxError, match="max_len 161"):
        checkpoints.xfm_from_state_dict({**sd, "pos_encoder.pe": torch.zeros((1, 161, 64))})
    big = xfm.XfmConfig(input_dim=44, d_model=80, n_heads=5, n_layers=1, ff=64, head=8, max_len=20)
    with pytest.raises(K.LmxError, match="d_model 80"):
        big.validate()
    with pytest.raises(K.LmxError, match="ff 272"):
        xfm.XfmConfig(ff=272).validate()
    with pytest.raises(K.LmxError, match="classes"):
        checkpoints.xfm_from_state_dict({**sd, "classifier.3.weight": torch.zeros((2, 32)), "classifier.3.bias": torch.zeros(2)})
    with pytest.raises(K.LmxError, match=r"layer\.1\.out\.weight"):
        checkpoints.xfm_from_state_dict({**sd, "encoder_layers.1.self_attn.out_proj.weight": torch.zeros((64, 32))})


# ---- the mask --------------------------------------------------------------------------------------------------------------------------
def _pose_frames(n, rng, low=0.3):
    """n T-LEAP frames with confidences: fewer than 20 keypoints in some, no confidence on some keypoints, low-confidence frames (low > 1: every frame)"""
    frames = []
    for t in range(n):
        x0, y0 = float(rng.uniform(0, 600)), float(rng.uniform(0, 300))
        w, h = float(rng.uniform(50, 600)), float(rng.uniform(50, 400))
        level = float(rng.uniform(0.05, 0.5 if low <= 1 else 0.2)) if rng.uniform() < low else float(rng.uniform(0.5, 1.0))
        kps = []
        for i in range(20 if t % 3 else 13):
            kp = {"x": float(rng.uniform(x0, x0 + w)), "y": float(rng.uniform(y0, y0 + h))}
            if (t + i) % 11:
                kp["confidence"] = float(np.clip(level + rng.uniform(-0.05, 0.05), 0, 1))
            kps.append(kp)
        frame = {"keypoints": kps, "bbox": [x0, y0, x0 + w, y0 + h]}
        if t % 4:
            frame["detection_confidence"] = float(rng.uniform(0.6, 1.0))
        frames.append(frame)
    return frames


def _mask_arrays(frames):
    n = len(frames)
    kc, nk, dc = np.zeros((n, 20)), np.zeros((n,), np.int32), np.ones((n,))
    for t, f in enumerate(frames):
        nk[t] = len(f["keypoints"])
        kc[t, :nk[t]] = [k.get("confidence", 0.5) for k in f["keypoints"]]
        dc[t] = f.get("detection_confidence", 1.0)
    return kc, nk, dc


@pytest.mark.parametrize("n", [1, 2, 60, 125, 126, 301])
def test_mask_equals_the_service_mirror(n, tmp_path):
    frames = _pose_frames(n, np.random.default_rng(n))
    pipe = TransformerPipeline(None, InProcessBus(), config={"nats": {}}, tleap_dir=tmp_path, results_dir=tmp_path)
    feats, mask = pipe.extract_features_from_tleap({"pose_sequences": frames})
    assert feats.shape == (n, 44) and mask.shape == (n,) and mask.dtype == bool
    fp, mp = pipe.pad_or_truncate(feats, mask, 125)
    got = K.xfm_mask(*_mask_arrays(frames), 125)
    assert fp.shape == (125, 44) and got.shape == (125,) and np.array_equal(got.astype(bool), mp)
    if n >= 60:
        assert 0 < int(mp.sum()) < 125
    if n < 125:
        before = (125 - n) // 2
        assert mp[:before].all() and mp[before + n:].all() and not fp[:before].any()
    # the features are the TCN's, from lmx_h_tcn_features
    kp, bb = np.zeros((n, 20, 2)), np.zeros((n, 4))
    for t, f in enumerate(frames):
        kp[t, :len(f["keypoints"])] = [[k["x"], k["y"]] for k in f["keypoints"]]
        bb[t] = f["bbox"]
    assert np.array_equal(K.tcn_features(kp, _mask_arrays(frames)[1], bb, 125).view(np.uint32), fp.view(np.uint32))
    assert pipe.extract_features_from_tleap({"pose_sequences": []}) == (None, None)


def test_mask_refuses_bad_arguments():
    with pytest.raises(K.LmxError, match="n_kp"):
        K.xfm_mask(np.zeros((2, 20)), np.array([3, 21], np.int32), np.ones((2,)))
    with pytest.raises(K.LmxError, match="confidences"):
        K.xfm_mask(np.zeros((2, 19)), np.array([3, 3], np.int32), np.ones((2,)))
    with pytest.raises(K.LmxError, match="target"):
        K.xfm_mask(np.zeros((2, 20)), np.array([3, 3], np.int32), np.ones((2,)), 0)


# ---- the weight image ------------------------------------------------------------------------------------------------------------------
def test_image_round_trip_and_refusals(models, tmp_path):
    for name, (cfg, w, _, _) in models.items():
        path = tmp_path / f"{name}.lmx"
        size = native.write_xfm_image(cfg, w, path)
        assert size == path.stat().st_size
        i = native.check_xfm_image(path)
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.ff, i.head, i.max_len, i.p) == cfg.shape() + (cfg.dropout,)
    raw = (tmp_path / "shipped.lmx").read_bytes()
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    bad = {
        "cut_header": (raw[:40], ""), "cut_config": (raw[:70], ""), "cut_directory": (raw[:dir_off + 3 * native.ENTRY_BYTES + 17], ""),
        "cut_data": (raw[:data_off + (len(raw) - data_off) // 2], ""), "cut_last_byte": (raw[:-1], ""),
        "kind": (raw[:12] + struct.pack("<I", native.KIND_TCN) + raw[16:], "kind"),
        "d_model_24": (raw[:48 + 4] + struct.pack("<i", 24) + raw[48 + 8:], "d_model 24"),
        "n_heads_3": (raw[:48 + 8] + struct.pack("<i", 3) + raw[48 + 12:], "n_heads 3"),
        "n_layers_9": (raw[:48 + 12] + struct.pack("<i", 9) + raw[48 + 16:], "n_layers 9"),
        "ff_40": (raw[:48 + 16] + struct.pack("<i", 40) + raw[48 + 20:], "ff 40"),
        "max_len_161": (raw[:48 + 24] + struct.pack("<i", 161) + raw[48 + 28:], "max_len 161"),
        "max_len_100": (raw[:48 + 24] + struct.pack("<i", 100) + raw[48 + 28:], "pe"),
        "reserved": (raw[:48 + 28] + struct.pack("<i", 1) + raw[48 + 32:], "reserved"),
        "p_nan": (raw[:48 + 32] + struct.pack("<d", float("nan")) + raw[48 + 40:], "p "),
        "n_tensors_huge": (raw[:20] + struct.pack("<I", 2 ** 20) + raw[24:], ""),
    }
    for name, (data, match) in bad.items():
        path = tmp_path / f"bad_{name}.lmx"
        path.write_bytes(data)
        with pytest.raises(K.LmxError, match=match or None):
            native.check_xfm_image(path)
    with pytest.raises(K.LmxError):
        native.check_xfm_image(tmp_path / "absent.lmx")
    tcn_like = tmp_path / "shipped.lmx"
    with pytest.raises(K.LmxError, match="kind"):
        native.check_tcn_image(tcn_like)


# ---- the service -----------------------------------------------------------------------------------------------------------------------
def _write_tleap(tleap_dir, video_id, n, seed, low=0.3):
    (tleap_dir / f"{video_id}_tleap.json").write_text(json.dumps({"video_id": video_id, "pose_sequences": _pose_frames(n, np.random.default_rng(seed), low)}))


def test_pipeline_on_the_in_process_bus(models, tmp_path):
    cfg, w, scorer, _ = models["shipped"]
    tleap, results = tmp_path / "tleap", tmp_path / "transformer"
    tleap.mkdir()
    bus = InProcessBus()
    pipe = TransformerPipeline(scorer, bus, config={"nats": {"subjects": {}}}, tleap_dir=tleap, results_dir=results)
    ids = ["cow_a", "cow_b", "cow_c"]
    for i, (vid, n) in enumerate(zip(ids, (90, 125, 200))):
        _write_tleap(tleap, vid, n, i)
    _write_tleap(tleap, "blurred", 40, 9, low=2.0)  # every frame below the confidence threshold: every step masked
    (tleap / "empty_tleap.json").write_text(json.dumps({"pose_sequences": []}))

    async def run():
        await pipe.start()
        await bus.publish("pipeline.tleap", {"video_id": "cow_a"})
        first = (results / "cow_a_transformer.json").read_bytes()
        await bus.publish("pipeline.tleap", {"video_id": "cow_a"})          # the same clip again: the same bytes
        assert (results / "cow_a_transformer.json").read_bytes() == first
        for vid in ("absent", "empty", "blurred"):                           # no file, no pose_sequences, every step masked
            await bus.publish("pipeline.tleap", {"video_id": vid})
        await bus.publish("pipeline.tleap", {})                              # no video_id
        for vid in ids[1:]:
            await pipe.process_video({"video_id": vid})
        singles = {vid: (results / f"{vid}_transformer.json").read_bytes() for vid in ids}
        for vid in ids:
            (results / f"{vid}_transformer.json").unlink()
        n_before = len(bus.published)
        await pipe.process_videos([{"video_id": "absent"}, {"video_id": "blurred"}] + [{"video_id": v} for v in ids])
        assert {vid: (results / f"{vid}_transformer.json").read_bytes() for vid in ids} == singles
        return singles, n_before

    singles, n_before = asyncio.run(run())
    assert sorted(p.name for p in results.iterdir()) == [f"{v}_transformer.json" for v in ids]
    out = [(s, m) for s, m in bus.published if s == "pipeline.transformer"]
    assert len(out) == 2 + 2 + 3 and len(bus.published) == n_before + 3
    doc = json.loads(singles["cow_a"])
    assert list(doc) == ["video_id", "pipeline", "severity_score", "uncertainty", "prediction", "confidence", "input_frames", "input_features",
                         "masked_frames", "temporal_saliency", "model_info"]
    assert (doc["video_id"], doc["pipeline"], doc["input_frames"], doc["input_features"]) == ("cow_a", "transformer", 125, 44)
    assert doc["model_info"] == {"d_model": 64, "num_layers": 4, "nhead": 4} and len(doc["temporal_saliency"]) == 20
    assert doc["prediction"] == int(doc["severity_score"] > 0.5) and doc["confidence"] == 1.0 - doc["uncertainty"] and doc["uncertainty"] > 0
    assert out[0][1] == {"video_id": "cow_a", "pipeline": "transformer", "results_path": str(results / "cow_a_transformer.json"),
                         "severity_score": doc["severity_score"], "uncertainty": doc["uncertainty"]}
    assert out[0][1] == out[1][1] == out[4][1]
    # the score is the scorer's for the clip's own seed and mask; the saliency is the unmasked eval run's
    feats, mask = pipe.pad_or_truncate(*pipe.extract_features_from_tleap(json.loads((tleap / "cow_a_tleap.json").read_text())))
    assert doc["masked_frames"] == int(mask.sum()) and 35 < doc["masked_frames"] < 125
    x = torch.from_numpy(feats)[None].contiguous()
    mean, std, pred = scorer.score(x, torch.from_numpy(mask)[None], [xfm.clip_seed("cow_a")])
    assert doc["severity_score"] == float(mean[0]) and doc["uncertainty"] == float(std[0]) and pred.shape == (1, 10)
    assert doc["temporal_saliency"] == [float(v) for v in scorer.saliency(x)[0, :20]]
