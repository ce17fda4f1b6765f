"""DeviceVectorStore and DeviceIdentityStore where MemoryVectorStore and MemoryIdentityStore stand: the same neighbours, labels,
evidence and identities, scores within the pinned dot product's bound plus the f32 rounding of the two unit vectors.

The handle lmx_vstore keeps its rows in HBM and cannot exist without a device, so these run under `-m gpu`."""
import asyncio
import itertools
import json

import numpy as np
import pytest
import torch

import vstoreref as V
from lmx import services, vstore
from lmx.services import runtime as R
from lmx.services import tracking as TR

pytestmark = pytest.mark.gpu

D = 384
TOL = V.bound(D) + 2.0 ** -22  # the extra term: the f32 rounding of the two unit vectors


class NoEmbedder:
    device = torch.device("cpu")

    class cfg:
        hidden = D


def _cfg():
    return {"nats": {"subjects": dict(R.DEFAULT_SUBJECTS)}}


def _points(rng, per_cluster):
    """[(cluster, vector)], float64: point i of a cluster is its unit centre plus (0.2 + 0.05 i) times a unit direction of its own, all
    centres and directions orthonormal.  The cosine of two points of a cluster is 1 / sqrt((1 + a^2) (1 + b^2)), so the ranks a query
    sees are at least 5e-3 apart; other clusters are at 0."""
    basis = np.linalg.qr(rng.standard_normal((D, 4 + 4 * per_cluster)))[0].T
    return [(c, basis[c] + (0.2 + 0.05 * i) * basis[4 + c * per_cluster + i]) for i in range(per_cluster) for c in range(4)]


def test_dinov3_finish_agrees_with_the_memory_store(cuda, tmp_path):
    rng = np.random.default_rng(21)
    points = _points(rng, 10)
    history, clips = points[:24], points[24:]  # six labelled points per cluster: every query has its five neighbours and a sixth in its cluster
    stores = {"mem": R.MemoryVectorStore(), "dev": vstore.DeviceVectorStore(cuda)}
    svc = {name: services.DINOv3Pipeline(NoEmbedder(), R.InProcessBus(), s, _cfg(), results_dir=tmp_path / name) for name, s in stores.items()}
    for i, (c, v) in enumerate(history):
        for s in stores.values():
            s.upsert(f"old{i}", v.tolist(), {"video_id": f"old{i}", "label": (i // 4 + c) % 2, "metadata": {"cluster": c}})
    rng.shuffle(clips)
    for i, (c, v) in enumerate(clips):
        frames = np.stack([v, v, v])
        data = svc["mem"].embeddings_result([{"frame": f, "time": float(f), "embedding": e.tolist()} for f, e in enumerate(frames)], 3, 1)
        top6 = [h["score"] for h in stores["mem"].search(np.mean(frames, axis=0), 6)]
        assert min(-np.diff(top6)) >= 1e-3, "the synthetic clusters must keep float64 rank gaps of 1e-3"
        msg = {"video_id": f"clip{i}", "processed_path": "unused", "filename": f"clip{i}.mp4", "metadata": {"cluster": c}}
        for p in svc.values():
            asyncio.run(p.finish(msg, data))
        a, b = (json.load(open(tmp_path / name / f"clip{i}_dinov3.json")) for name in ("mem", "dev"))
        assert len(a["similar_cases"]) == 5
        assert [(h["video_id"], h["label"], h["metadata"]) for h in a["similar_cases"]] == [(h["video_id"], h["label"], h["metadata"]) for h in b["similar_cases"]]
        assert a["neighbor_evidence"] == b["neighbor_evidence"]
        worst = max(abs(x["score"] - y["score"]) for x, y in zip(a["similar_cases"], b["similar_cases"]))
        assert worst <= TOL, worst
        assert {k: v for k, v in a.items() if k != "similar_cases"} == {k: v for k, v in b.items() if k != "similar_cases"}
    assert stores["dev"].count() == len(stores["mem"].points) == 24 + 16
    assert {json.load(open(tmp_path / "dev" / f"clip{i}_dinov3.json"))["neighbor_evidence"] for i in range(16)} != {0.5}
    # upsert by an existing id replaces that slot
    stores["dev"].upsert("clip0", (-history[0][1]).tolist(), {"video_id": "clip0", "label": 1})
    assert stores["dev"].count() == 40 and stores["dev"].search(-history[0][1], 1)[0] == {"video_id": "clip0", "score": pytest.approx(1, abs=TOL), "label": 1, "metadata": {}}


def test_reid_matcher_agrees_with_the_memory_store(cuda):
    """CowReIDMatcher.match_or_create over 20 clips of 4 synthetic cows: the same identities, the same is_new sequence"""
    rng = np.random.default_rng(22)
    cows = rng.standard_normal((4, D))
    clips = [(c, cows[c] + 0.25 * rng.standard_normal(D)) for c in rng.permutation(np.repeat(np.arange(4), 5))]
    out = {}
    for name, store in (("mem", TR.MemoryIdentityStore()), ("dev", vstore.DeviceIdentityStore(cuda))):
        ids = (f"00000000-0000-0000-0000-{i:012d}" for i in itertools.count())
        m = TR.CowReIDMatcher(store, embedding_dim=D, new_uuid=lambda ids=ids: next(ids))
        m.connect()
        out[name] = [m.match_or_create(v, f"video{i}", i) for i, (_, v) in enumerate(clips)]
        assert store.count() == 4
    assert [r["identity_id"] for r in out["mem"]] == [r["identity_id"] for r in out["dev"]]
    assert [r["is_new_identity"] for r in out["mem"]] == [r["is_new_identity"] for r in out["dev"]]
    assert [r["cow_id"] for r in out["mem"]] == [r["cow_id"] for r in out["dev"]] and [r["confidence"] for r in out["mem"]] == [r["confidence"] for r in out["dev"]]
    assert sum(r["is_new_identity"] for r in out["dev"]) == 4
    first = {}
    for (c, _), r in zip(clips, out["dev"]):
        assert first.setdefault(c, r["identity_id"]) == r["identity_id"]  # a cow keeps its identity
    # the stored vectors drift apart by f32 roundings of the momentum update only: 16 updates, each within the unit rows' rounding
    assert max(abs(a["similarity"] - b["similarity"]) for a, b in zip(out["mem"], out["dev"])) <= 16 * TOL
