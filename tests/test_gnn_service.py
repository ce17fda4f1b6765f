"""GNNPipeline, the mirror of services/gnn-pipeline/app/main.py, on a synthetic results tree without a GPU: the keys of `{id}_gnn.json`
as the reference writes them, the values against the scorer and the restatement on the mirror's own graph, a backlog that scores to the
same bytes, and the videos the reference writes nothing for."""
import asyncio
import json

import numpy as np
import pytest
import torch

import gnnref
from lmx import gnn
from lmx import kernels as K


@pytest.fixture(scope="module")
def host():
    cfg, w = gnnref.shared()[0]["shipped"]
    return cfg, w, gnn.GnnScorer(cfg, w, backend="host")


def test_service_mirror_on_a_results_tree(host, tmp_path):
    from lmx.services import GNNPipeline
    from lmx.services.runtime import InProcessBus

    cfg, w, scorer = host
    rng = np.random.default_rng(3)
    videos = [(f"a{i}", "cow_A", "2024-05-%02dT10:00:00Z" % (i + 1)) for i in range(6)] + [(f"b{i}", "cow_B", 1.7e9 + 3600.0 * i + 0.25) for i in range(3)]
    videos += [("loose", None, None), ("a_bad_time", "cow_A", "yesterday"), ("alone", "cow_C", 1.7e9)]
    gnnref.results_tree(tmp_path, videos, rng)
    bus, got = InProcessBus(), []

    async def run():
        await bus.subscribe("pipeline.gnn", lambda m: got.append(m))
        svc = GNNPipeline(scorer, bus, config={}, data_dir=tmp_path)
        await svc.process_video({"video_id": "a3"})
        await svc.process_video({})
        await svc.process_video({"video_id": "alone"})  # one node: torch raises in the reference, nothing is written
        await svc.process_videos([{"video_id": "b1"}, {"video_id": "loose"}, {"video_id": "alone"}, {"video_id": "a3"}, {"video_id": "new_video"}])
        return svc

    svc = asyncio.run(run())
    assert [m["video_id"] for m in got] == ["a3", "b1", "loose", "a3", "new_video"]
    assert not (tmp_path / "gnn" / "alone_gnn.json").exists()
    res = json.loads((tmp_path / "gnn" / "a3_gnn.json").read_text())
    assert list(res) == ["video_id", "cow_id", "pipeline", "model", "severity_score", "cow_severity_score", "uncertainty", "prediction",
                         "cow_prediction", "confidence", "graph_info", "neighbor_influence", "videos_in_graph"]
    assert list(res["graph_info"]) == ["num_nodes", "num_edges", "k_neighbors", "has_edge_features", "has_temporal_edges", "num_heads",
                                       "hierarchical_pooling", "per_cow_graph"]
    assert res["cow_id"] == "cow_A" and res["model"] == "EnhancedGraphGPS" and res["pipeline"] == "gnn"
    assert sorted(res["videos_in_graph"]) == sorted([f"a{i}" for i in range(6)] + ["a_bad_time"])
    assert res["graph_info"] == {"num_nodes": 7, "num_edges": 7 * 5 + 2 * 6, "k_neighbors": 5, "has_edge_features": True, "has_temporal_edges": True,
                                 "num_heads": 8, "hierarchical_pooling": True, "per_cow_graph": True}
    assert res["confidence"] == 1.0 - res["uncertainty"] and res["prediction"] == int(res["severity_score"] > 0.5)
    assert got[0] == {"video_id": "a3", "cow_id": "cow_A", "pipeline": "gnn", "results_path": str(tmp_path / "gnn" / "a3_gnn.json"),
                      "severity_score": res["severity_score"], "cow_severity_score": res["cow_severity_score"], "uncertainty": res["uncertainty"],
                      "model": "EnhancedGraphGPS"}
    assert got[3] == got[0]  # in a backlog a graph scores to the same bytes
    # the features, the graph and the scores are those of the scorer and of the restatement on the mirror's own inputs
    item = svc._graph("a3")
    t = item["target"]
    assert item["video_ids"][t] == "a3"
    x = item["graph"]["x"]
    assert x.shape == (7, 50) and (x[:, 47:] == np.array([0.5, 1.0, 0.5], np.float32)).all() and (x[:, 12] == 1.0).all()  # meta; aspect ratio's default
    emb = x[:, 15:47]  # the first 32 values of the embedding, zero-padded where it has 20
    ts = np.array([svc.video_timestamps[v] for v in item["video_ids"]], np.float64)
    assert svc.video_timestamps["a_bad_time"] == 0.0 and svc.video_timestamps["b2"] == 1.7e9 + 7200.25
    want = gnnref.build_graph(cfg, x, emb, ts)
    for key in ("edges", "csr_ptr", "csr_edge", "deg"):
        assert np.array_equal(item["graph"][key], want[key]), key
    assert (np.abs(item["graph"]["edge_attr"] - want["edge_attr"]) <= np.spacing(np.abs(want["edge_attr"]))).all()
    (mean, std), = scorer.score([item["graph"]], [gnn.graph_seed("a3")], 10)
    gp, _, _ = scorer.evaluate([item["graph"]])
    assert res["severity_score"] == float(mean[t]) and res["uncertainty"] == float(std[t]) and res["cow_severity_score"] == float(gp[0])
    into = [int(s) for s, d in item["graph"]["edges"] if int(d) == t][:5]  # the first five edges into the target, in edge order
    assert len(into) == 5 and res["neighbor_influence"] == [{"video_id": item["video_ids"][s], "score": float(mean[s])} for s in into]
    ref = gnnref.forward(cfg, w, item["graph"], None, torch.float64)
    assert abs(res["cow_severity_score"] - float(ref["graph_pred"])) <= 1e-5
    keeps = [gnnref.keep_arrays(cfg, 7, gnn.graph_seed("a3"), s) for s in range(10)]
    mc = torch.stack([gnnref.forward(cfg, w, item["graph"], k, torch.float64)["node_pred"] for k in keeps])
    assert abs(res["severity_score"] - float(mc.mean(0)[t])) <= 1e-4 and abs(res["uncertainty"] - float(mc.std(0)[t])) <= 1e-4
    # a video without a cow: the global graph over every analysed video, no temporal edges; an unknown video joins with the defaults
    loose = json.loads((tmp_path / "gnn" / "loose_gnn.json").read_text())
    assert loose["cow_id"] is None and loose["graph_info"]["num_nodes"] == 12 and not loose["graph_info"]["has_temporal_edges"]
    assert loose["graph_info"]["num_edges"] == 12 * 5
    new = json.loads((tmp_path / "gnn" / "new_video_gnn.json").read_text())
    assert new["graph_info"]["num_nodes"] == 13 and new["videos_in_graph"][-1] == "new_video"


def test_service_mirror_refuses_a_graph_above_the_limit_and_a_single_node(host, tmp_path):
    from lmx.services import GNNPipeline
    from lmx.services.runtime import InProcessBus

    n = gnn.MAX_NODES + 1
    gnnref.results_tree(tmp_path, [(f"v{i}", "cow_A", 1.7e9 + i) for i in range(n)] + [("alone", "cow_B", 1.7e9)], np.random.default_rng(1))
    svc = GNNPipeline(host[2], InProcessBus(), config={}, data_dir=tmp_path)
    with pytest.raises(K.LmxError, match=f"{n} nodes.*{gnn.MAX_NODES}"):
        svc._graph("v0")
    with pytest.raises(K.LmxError, match="one node: BatchNorm has no batch statistics"):
        svc._graph("alone")
    asyncio.run(svc.process_video({"video_id": "v0"}))
    asyncio.run(svc.process_videos([{"video_id": "v1"}, {"video_id": "alone"}]))
    assert not list((tmp_path / "gnn").glob("*.json"))
