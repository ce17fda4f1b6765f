"""The TCN gait model without a GPU (include/lmx.h "The TCN gait model"; csrc/host_tcn.cpp, csrc/host_tcn_image.cpp, lmx/tcn.py,
lmx/services/tcn_pipeline.py):
  * lmx_h_tcn_keep_bits against the numpy restatement of the header's text (tcnref.keep_bits);
  * lmx_h_tcn_features and TCNPipeline's feature methods against values computed by hand from the formulas;
  * lmx_h_tcn_forward against tcnref in float64 under the tolerance rule of tcnref.tolerances;
  * the weight image: write, check, refusals with the field named; both state_dict spellings;
  * TCNPipeline on InProcessBus with the host backend."""
import asyncio
import json
import struct

import numpy as np
import pytest
import torch

import tcnref
from lmx import checkpoints, native, tcn
from lmx import kernels as K
from lmx.services import TCNPipeline
from lmx.services.runtime import InProcessBus

FORWARD_T = (1, 2, 3, 60, 61, 62, 125)


# ---- keep bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
def test_keep_bits_equal_the_header_text(p):
    N = 8000
    for seed in (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1):
        for sample, site, n_sites in ((0, 0, 9), (3, 8, 9), (9, 4, 13), (65534, 16, 17)):
            got = K.tcn_keep_bits(seed, sample, site, n_sites, N, p)
            assert np.array_equal(got, tcnref.keep_bits(seed, sample, site, n_sites, N, p)), (seed, sample, site)
            if p == 0.0:
                assert got.all()
            frac = got.mean()
            assert abs(frac - (1 - p)) <= 5 * (p * (1 - p) / N) ** 0.5, (seed, sample, site, frac)
    a, b = K.tcn_keep_bits(7, 0, 0, 9, N, 0.5), K.tcn_keep_bits(7, 0, 1, 9, N, 0.5)
    c, d = K.tcn_keep_bits(7, 1, 0, 9, N, 0.5), K.tcn_keep_bits(8, 0, 0, 9, N, 0.5)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d) and not np.array_equal(b, c)
    with pytest.raises(K.LmxError, match="site"):
        K.tcn_keep_bits(1, 0, 9, 9, 4, 0.2)
    with pytest.raises(K.LmxError, match="p "):
        K.tcn_keep_bits(1, 0, 0, 9, 4, 1.0)


# ---- features -------------------------------------------------------------------------------------------------------------------
def _pose_frames(n, rng):
    """n T-LEAP frames: fewer than 20 keypoints in some, a bbox narrower than 1 in some"""
    frames = []
    for t in range(n):
        x0, y0 = float(rng.uniform(0, 600)), float(rng.uniform(0, 300))
        w = 0.25 if t % 5 == 2 else float(rng.uniform(50, 600))
        h = 0.5 if t % 7 == 3 else float(rng.uniform(50, 400))
        kps = [{"x": float(rng.uniform(x0, x0 + w)), "y": float(rng.uniform(y0, y0 + h))} for _ in range(20 if t % 3 else 13)]
        frames.append({"keypoints": kps, "bbox": [x0, y0, x0 + w, y0 + h]})
    return frames


def _by_hand(frames, target):
    """[target, 44] float32 straight from the formulas of the issue"""
    rows = []
    for f in frames:
        x0, y0, x1, y1 = f["bbox"]
        bw, bh = x1 - x0, y1 - y0
        row = []
        for kp in f["keypoints"][:20]:
            row += [np.float32((kp["x"] - x0) / max(bw, 1)), np.float32((kp["y"] - y0) / max(bh, 1))]
        row += [np.float32(0)] * (40 - len(row))
        row += [np.float32((x0 + x1) / 2 / 1280), np.float32((y0 + y1) / 2 / 720), np.float32(bw * bh / (1280 * 720)), np.float32(0)]
        rows.append(row)
    a = np.array(rows, np.float32)
    for t in range(1, len(a)):
        a[t, 43] = np.float32(a[t, 40]) - np.float32(a[t - 1, 40])  # the float32 column's difference, in float32
    n = len(a)
    if n >= target:
        s = (n - target) // 2
        return a[s:s + target]
    out = np.zeros((target, 44), np.float32)
    before = (target - n) // 2
    out[before:before + n] = a
    return out


@pytest.mark.parametrize("n", [1, 124, 125, 126, 300])
def test_features_equal_the_formulas(n, tmp_path):
    frames = _pose_frames(n, np.random.default_rng(n))
    want = _by_hand(frames, 125)
    kp, nk, bb = np.zeros((n, 20, 2)), np.zeros((n,), np.int32), np.zeros((n, 4))
    for t, f in enumerate(frames):
        nk[t] = len(f["keypoints"])
        kp[t, :nk[t]] = [[k["x"], k["y"]] for k in f["keypoints"]]
        bb[t] = f["bbox"]
    got = K.tcn_features(kp, nk, bb, 125)
    assert got.shape == (125, 44) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pipe = TCNPipeline(None, InProcessBus(), config={"nats": {}}, tleap_dir=tmp_path, results_dir=tmp_path)
    feats = pipe.extract_features_from_tleap({"pose_sequences": frames})
    assert feats.shape == (n, 44) and feats.dtype == np.float32
    got = pipe.pad_or_truncate(feats, 125)
    assert got.shape == (125, 44) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if n > 1:  # the velocity is NOT the float64 difference rounded once
        exact = np.float32(np.diff(np.array([(f["bbox"][0] + f["bbox"][2]) / 2 / 1280 for f in frames])))
        assert np.array_equal(feats[1:, 43], np.diff(feats[:, 40])) and not np.array_equal(feats[1:, 43], exact)
    assert pipe.extract_features_from_tleap({"pose_sequences": []}) is None and pipe.extract_features_from_tleap({}) is None


def test_features_refuse_bad_arguments():
    with pytest.raises(K.LmxError, match="n_kp"):
        K.tcn_features(np.zeros((2, 20, 2)), np.array([3, 21], np.int32), np.zeros((2, 4)))
    with pytest.raises(K.LmxError, match="T0"):
        K.tcn_features(np.zeros((0, 20, 2)), np.zeros((0,), np.int32), np.zeros((0, 4)))


# ---- the host forward against float64 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    out = {}
    for i, (name, cfg) in enumerate(tcnref.CONFIGS.items()):
        got, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 11 + i), cfg.dropout)
        assert got == cfg
        out[name] = (cfg, folded, tcn.TcnScorer(cfg, folded, backend="host"))
    return out


@pytest.fixture(scope="module")
def cases(models):
    """every configuration x T x {eval, S = 10}; the float64 and float32 references are computed once"""
    out = []
    for name, (cfg, folded, _) in models.items():
        for T in FORWARD_T:
            for S in (0, 10):
                out.append(tcnref.make_case(f"{name}-T{T}-S{S}", cfg, folded, T, S, n=2))
    return out


def test_host_forward_against_float64(models, cases):
    tol_trunk, tol_pred, e_trunk, e_pred = tcnref.tolerances(cases)
    print(f"e_ref: trunk {e_trunk:.3g} (relative), pred {e_pred:.3g}")
    worst = [0.0, 0.0]
    for case in cases:
        scorer = models[case.name.split("-")[0]][2]
        pred, stats, trunk = scorer.forward(case.x, case.seeds, case.S, trunk=True)
        rt, rp = tcnref.check_case(case, trunk, pred, tol_trunk, tol_pred, "host")
        worst = [max(worst[0], rt), max(worst[1], rp)]
        want = pred.double()
        if case.S:
            assert torch.allclose(stats[:, 0].double(), want.mean(1), rtol=0, atol=2e-7)
            assert torch.allclose(stats[:, 1].double(), want.std(1), rtol=0, atol=2e-7)
        else:
            assert torch.equal(stats[:, 0], pred[:, 0]) and not stats[:, 1].any()
    print(f"worst ratio to the bound: trunk {worst[0]:.3f}, pred {worst[1]:.3f}")


# ---- the image, the checkpoint spellings, the refusals ---------------------------------------------------------------------------
def test_both_key_spellings_fold_to_the_same_weights():
    for i, cfg in enumerate(tcnref.CONFIGS.values()):
        a_cfg, a = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 5 + i, legacy=False))
        b_cfg, b = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 5 + i, legacy=True))
        assert a_cfg == b_cfg == cfg and a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
        sd = tcnref.state_dict(cfg, 5 + i)
        v, g = sd["network.0.conv1.conv.parametrizations.weight.original1"], sd["network.0.conv1.conv.parametrizations.weight.original0"]
        assert torch.equal(a["block.0.conv1.weight"], torch._weight_norm(v, g, 0)) and not torch.equal(a["block.0.conv1.weight"], v)


def test_image_round_trip_and_refusals(models, tmp_path):
    for name, (cfg, folded, scorer) in models.items():
        path = tmp_path / f"{name}.lmx"
        size = native.write_tcn_image(cfg, folded, path)
        assert size == path.stat().st_size
        info = native.check_tcn_image(path)
        assert (info.input_dim, info.n_blocks, info.k, info.head, info.p) == (cfg.input_dim, cfg.n_blocks, cfg.kernel_size, cfg.head, cfg.dropout)
        assert list(info.channels)[:cfg.n_blocks] == list(cfg.channels) and info.receptive_field == cfg.receptive_field
    assert tcnref.SHIPPED.receptive_field == 61
    cfg, folded, scorer = models["shipped"]
    raw = (tmp_path / "shipped.lmx").read_bytes()
    # what the image holds is what the scorer holds: the same tensors, so the host scores from either are the same
    packed = tcn.pack_tensors(cfg, folded)
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    for j, (tname, a) in enumerate(packed.items()):
        ent = raw[dir_off + j * native.ENTRY_BYTES:dir_off + (j + 1) * native.ENTRY_BYTES]
        off, nbytes = struct.unpack_from("<QQ", ent, 72)
        assert ent[:48].rstrip(b"\0").decode() == tname and raw[off:off + nbytes] == a.tobytes()
        assert torch.equal(scorer.tensors[tname], torch.from_numpy(a))

    def refused(data, word):
        bad = tmp_path / "bad.lmx"
        bad.write_bytes(data)
        with pytest.raises(native.LmxError, match=word):
            native.check_tcn_image(bad)

    refused(raw[:len(raw) // 2], "file_bytes")                                    # a truncated file
    refused(raw[:48 + 16] + struct.pack("<i", 24) + raw[48 + 20:], r"channels\[0\] = 24")
    refused(raw[:48 + 8] + struct.pack("<i", 4) + raw[48 + 12:], "k 4")
    refused(raw[:12] + struct.pack("<I", native.KIND_DINO) + raw[16:], "kind")
    refused(raw[:48 + 48] + struct.pack("<d", 1.0) + raw[48 + 56:], "p 1")
    assert native.check_tcn_image(tmp_path / "shipped.lmx").k == 3
    # the same refusals from Python, each with its field named
    with pytest.raises(K.LmxError, match=r"channels\[1\] = 24"):
        tcn.TcnConfig(channels=(64, 24)).validate()
    with pytest.raises(K.LmxError, match="k 4"):
        native.write_tcn_image(tcn.TcnConfig(kernel_size=4), folded, tmp_path / "x.lmx")
    x = torch.zeros((1, 257, cfg.input_dim))
    with pytest.raises(K.LmxError, match="T 257"):
        scorer.score(x, [1])
    with pytest.raises(K.LmxError, match="S 1"):
        scorer.score(x[:, :8].contiguous(), [1], n_samples=1)
    with pytest.raises(K.LmxError, match="seeds"):
        scorer.score(x[:, :8].contiguous(), [1, 2])
    with pytest.raises(K.LmxError, match="float32"):
        scorer.score(x[:, :8].double(), [1])
    # the library itself refuses them too, whatever the binding lets through
    lib = native._lib.load()
    p8, s8 = torch.zeros((1, 2)), torch.zeros((1, 2))
    seeds = np.array([1], np.uint64)
    for T, S, word in ((257, 2, b"T 257"), (8, 1, b"S 1")):
        rc = lib.lmx_h_tcn_forward(native.C.byref(scorer.weights), x.data_ptr(), seeds.ctypes.data, 1, T, S, 0.2, p8.data_ptr(), s8.data_ptr(), None)
        assert rc == -1 and word in lib.lmx_last_error()
    sd = tcnref.state_dict(cfg, 3)
    sd["classifier.5.weight"] = torch.zeros((2, 32))
    with pytest.raises(K.LmxError, match="num_classes 2"):
        checkpoints.tcn_from_state_dict(sd)


# ---- the service -------------------------------------------------------------------------------------------------------------------
def _write_tleap(tleap_dir, video_id, n, seed):
    (tleap_dir / f"{video_id}_tleap.json").write_text(json.dumps({"video_id": video_id, "pose_sequences": _pose_frames(n, np.random.default_rng(seed))}))


def test_pipeline_on_the_in_process_bus(models, tmp_path):
    cfg, folded, scorer = models["shipped"]
    tleap, results = tmp_path / "tleap", tmp_path / "tcn"
    tleap.mkdir()
    bus = InProcessBus()
    pipe = TCNPipeline(scorer, bus, config={"nats": {"subjects": {}}}, tleap_dir=tleap, results_dir=results)
    ids = ["cow_a", "cow_b", "cow_c"]
    for i, (vid, n) in enumerate(zip(ids, (90, 125, 200))):
        _write_tleap(tleap, vid, n, i)
    (tleap / "empty_tleap.json").write_text(json.dumps({"pose_sequences": []}))

    async def run():
        await pipe.start()
        await bus.publish("pipeline.tleap", {"video_id": "cow_a"})
        first = (results / "cow_a_tcn.json").read_bytes()
        await bus.publish("pipeline.tleap", {"video_id": "cow_a"})          # the same clip again: the same bytes
        assert (results / "cow_a_tcn.json").read_bytes() == first
        await bus.publish("pipeline.tleap", {"video_id": "absent"})         # no T-LEAP file
        await bus.publish("pipeline.tleap", {"video_id": "empty"})          # no pose_sequences
        await bus.publish("pipeline.tleap", {})                              # no video_id
        for vid in ids[1:]:
            await pipe.process_video({"video_id": vid})
        singles = {vid: (results / f"{vid}_tcn.json").read_bytes() for vid in ids}
        for vid in ids:
            (results / f"{vid}_tcn.json").unlink()
        n_before = len(bus.published)
        await pipe.process_videos([{"video_id": "absent"}] + [{"video_id": v} for v in ids])
        assert {vid: (results / f"{vid}_tcn.json").read_bytes() for vid in ids} == singles
        return singles, n_before

    singles, n_before = asyncio.run(run())
    assert sorted(p.name for p in results.iterdir()) == [f"{v}_tcn.json" for v in ids]
    out = [(s, m) for s, m in bus.published if s == "pipeline.tcn"]
    assert len(out) == 2 + 2 + 3 and len(bus.published) == n_before + 3
    doc = json.loads(singles["cow_a"])
    assert list(doc) == ["video_id", "pipeline", "severity_score", "uncertainty", "prediction", "confidence", "input_frames", "input_features",
                         "model_receptive_field"]
    assert (doc["video_id"], doc["pipeline"], doc["input_frames"], doc["input_features"], doc["model_receptive_field"]) == ("cow_a", "tcn", 125, 44, 61)
    assert doc["prediction"] == int(doc["severity_score"] > 0.5) and doc["confidence"] == 1.0 - doc["uncertainty"] and doc["uncertainty"] > 0
    assert out[0][1] == {"video_id": "cow_a", "pipeline": "tcn", "results_path": str(results / "cow_a_tcn.json"),
                         "severity_score": doc["severity_score"], "uncertainty": doc["uncertainty"]}
    assert out[0][1] == out[1][1] == out[4][1]
    # the score is the scorer's for the clip's own seed
    feats = pipe.pad_or_truncate(pipe.extract_features_from_tleap(json.loads((tleap / "cow_a_tleap.json").read_text())))
    mean, std, pred = scorer.score(torch.from_numpy(feats)[None].contiguous(), [tcn.clip_seed("cow_a")])
    assert doc["severity_score"] == float(mean[0]) and doc["uncertainty"] == float(std[0]) and pred.shape == (1, 10)
    assert tcn.clip_seed("cow_a") == int.from_bytes(__import__("hashlib").sha256(b"cow_a").digest()[:8], "little")
