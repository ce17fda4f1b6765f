"""GNNPipeline — mirror of services/gnn-pipeline/app/main.py, the graph transformer's twin on `pipeline.dinov3`.  It reads the same four
result files and the same tracking results as ``GraphTransformerPipeline``, whose results-tree reader it inherits unchanged (the cow of
a video, the timestamps, the 50 node features with the reference's truncation of the embedding to its first 32 values and its three
constant meta features), builds the per-cow graph by the rules of GraphBuilder (``lmx.gnn.build_graph``: the raw cosine as kNN weight,
temporal edges with tanh(|dt| / 86400) only where the cow is known) and scores it: `model.predict_with_uncertainty(graph, 10)` and the
eval-mode `model(graph)` — eleven forwards, each with an eigensolver and 16 dense matrix powers on the host — are TWO calls of
``lmx.gnn.GnnScorer``, and ``process_videos`` scores a backlog in the same two.  The result goes to `{id}_gnn.json` with the reference's
keys and is published on `pipeline.gnn`.  A graph of one node has no batch statistics: torch raises in the reference, which then writes
no result, and nothing is written here either.  A graph of more than ``lmx.gnn.MAX_NODES`` nodes is refused with both numbers.  The
dropout bits are the library's, seeded per graph by ``lmx.gnn.graph_seed(video_id)``; BatchNorm's running statistics do not drift
("Graph model: GraphGPS")."""
import json
import traceback

import numpy as np

from .. import gnn
from .graph_transformer_pipeline import GraphTransformerPipeline


class GNNPipeline(GraphTransformerPipeline):
    MODEL_NAME = "EnhancedGraphGPS"

    def __init__(self, scorer, bus, config=None, data_dir="/app/data/results", results_dir=None):
        from pathlib import Path

        super().__init__(scorer, bus, config, data_dir, results_dir if results_dir is not None else Path(data_dir) / "gnn")

    # ---- main.py:1432-1491: everything up to the model ---------------------------------------------------------------------------------
    def _graph(self, video_id):
        cow = self.get_cow_for_video(video_id)
        node_features, embeddings, video_ids, cow_ids, timestamps = self.collect_graph_data(filter_cow_id=cow) if cow else self.collect_graph_data()
        if node_features is None or len(video_ids) == 0:
            print("  No video features available for graph construction")
            return None
        if video_id not in video_ids:
            features = self.extract_node_features(video_id)
            node_features, embeddings = np.vstack([node_features, self._node(features)]), np.vstack([embeddings, features["embedding"]])
            video_ids.append(video_id), cow_ids.append(cow), timestamps.append(self.video_timestamps.get(video_id, 0.0))
        if len(video_ids) > gnn.MAX_NODES:
            raise gnn.LmxError(f"GNNPipeline: the graph of {video_id} has {len(video_ids)} nodes; one workgroup holds at most {gnn.MAX_NODES}")
        if len(video_ids) < 2:
            raise gnn.LmxError(f"GNNPipeline: the graph of {video_id} has one node: BatchNorm has no batch statistics (torch raises in the reference)")
        ts = np.asarray(timestamps, np.float64) if cow else None  # Python floats in the reference
        graph = gnn.build_graph(self.model.cfg, node_features.astype(np.float32), embeddings.astype(np.float32), ts, self.K_NEIGHBORS)
        return {"graph": graph, "target": video_ids.index(video_id), "cow": cow, "video_ids": video_ids}

    def _score(self, video_ids, items):
        """Two launches for all graphs: S = 10, then eval mode for the cow score"""
        batch = self.model.batch([it["graph"] for it in items])
        stats = self.model.score(batch, [gnn.graph_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        graph_pred = self.model.evaluate(batch)[0].cpu().numpy()
        return [(m.cpu().numpy(), s.cpu().numpy(), float(graph_pred[i])) for i, (m, s) in enumerate(stats)]

    def _results(self, video_id, item, mean_pred, std_pred, cow_severity_score):
        target_idx, video_ids, cow = item["target"], item["video_ids"], item["cow"]
        node_severity_score, node_uncertainty = float(mean_pred[target_idx]), float(std_pred[target_idx])
        edges = item["graph"]["edges"]
        neighbor_scores = [{"video_id": video_ids[int(s)], "score": float(mean_pred[int(s)])} for s, d in edges if int(d) == target_idx]
        return {"video_id": video_id, "cow_id": cow, "pipeline": "gnn", "model": self.MODEL_NAME, "severity_score": node_severity_score,
                "cow_severity_score": cow_severity_score, "uncertainty": node_uncertainty, "prediction": int(node_severity_score > 0.5),
                "cow_prediction": int(cow_severity_score > 0.5), "confidence": 1.0 - node_uncertainty,
                "graph_info": {"num_nodes": len(video_ids), "num_edges": int(len(edges)), "k_neighbors": self.K_NEIGHBORS, "has_edge_features": True,
                               "has_temporal_edges": cow is not None, "num_heads": 8, "hierarchical_pooling": True,  # as the reference prints them
                               "per_cow_graph": cow is not None},
                "neighbor_influence": neighbor_scores[:5], "videos_in_graph": video_ids}

    async def _finish(self, video_id, item, scores):
        results = self._results(video_id, item, *scores)
        results_file = self.results_dir / f"{video_id}_gnn.json"
        with open(results_file, "w") as f:
            json.dump(results, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_gnn", "pipeline.gnn")
        await self.nats_client.publish(subject, {"video_id": video_id, "cow_id": item["cow"], "pipeline": "gnn", "results_path": str(results_file),
                                                 "severity_score": results["severity_score"], "cow_severity_score": results["cow_severity_score"],
                                                 "uncertainty": results["uncertainty"], "model": self.MODEL_NAME})

    async def _process(self, ready):
        if not ready:
            return
        scores = self._score([v for v, _ in ready], [it for _, it in ready])
        for (video_id, item), sc in zip(ready, scores):
            await self._finish(video_id, item, sc)

    async def process_video(self, video_data):
        video_id = video_data.get("video_id")
        if not video_id:
            return
        try:
            item = self._graph(video_id)
            await self._process([(video_id, item)] if item is not None else [])
        except Exception as e:  # noqa: BLE001 — the reference prints and writes nothing
            print(f"  Error in GNN pipeline for {video_id}: {e}")
            traceback.print_exc()

    async def process_videos(self, videos):
        """A backlog of graphs in the same two launches: each graph's file and message are those of process_video, bit for bit.  A graph
        above the node limit or of one node is refused on its own."""
        ready = []
        for video_data in videos:
            video_id = video_data.get("video_id")
            if not video_id:
                continue
            try:
                item = self._graph(video_id)
                if item is not None:
                    ready.append((video_id, item))
            except Exception as e:  # noqa: BLE001
                print(f"  Error in GNN pipeline for {video_id}: {e}")
        try:
            await self._process(ready)
        except Exception as e:  # noqa: BLE001
            print(f"  Error in GNN pipeline: {e}")
            traceback.print_exc()
