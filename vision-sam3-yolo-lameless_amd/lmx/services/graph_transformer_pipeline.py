"""GraphTransformerPipeline — mirror of services/graph-transformer-pipeline/app/main.py, the consumer of `pipeline.dinov3`.  For the
video of a message it looks up the cow in the tracking results (`{id}_tracking.json`: the first `reid_results` entry with a `cow_id`,
and the video's timestamp), collects one node per analysed video of that cow (every video where the cow is unknown) — 50 features from
`{id}_tleap.json`, `{id}_sam3.json`, `{id}_yolo.json` and `{id}_dinov3.json` with the reference's defaults —, builds the graph
(kNN over the DINO embeddings, k = 5; temporal edges and the temporal encoding only for a per-cow graph) and scores it:
`model.predict_with_uncertainty(graph, n_samples=10)` and the eval-mode `model(graph, return_attention=True)` (eleven forwards of
several hundred launches, each with networkx shortest paths) are TWO calls of ``lmx.gfm.GfmScorer`` — S = 10, then eval mode for the
target's node score and the attention towards it — and ``process_videos`` scores a backlog of graphs in the same two calls.  The result
goes to `{id}_graph_transformer.json` with the reference's keys and is published on `pipeline.graph_transformer`.  The dropout bits are
the library's (include/lmx.h), seeded per graph by ``lmx.gfm.graph_seed(video_id)``; parity with torch's generator is statistical.  A
graph of more than ``lmx.gfm.MAX_NODES`` nodes does not fit one workgroup: it is refused with both numbers, and nothing is written.
NATS and the config file stay with the caller (``lmx.services.runtime``)."""
import json
import traceback
from datetime import datetime
from pathlib import Path

import numpy as np

from .. import gfm
from . import runtime as R


class GraphTransformerPipeline:
    POSE_FEATURES, SILHOUETTE_FEATURES, EMBEDDING_DIM, META_FEATURES = 10, 5, 32, 3
    K_NEIGHBORS = 5
    N_SAMPLES = 10

    def __init__(self, scorer, bus, config=None, data_dir="/app/data/results", results_dir=None):
        self.config = config or R.load_config()
        self.nats_client = bus
        self.model = scorer
        self.data_dir = Path(data_dir)
        self.results_dir = Path(results_dir if results_dir is not None else self.data_dir / "graph_transformer")
        self.results_dir.mkdir(parents=True, exist_ok=True)
        self.cow_id_mapping, self.video_timestamps = {}, {}

    # ---- main.py:106-170 -----------------------------------------------------------------------------------------------------------
    def load_cow_id_mapping(self):
        """video_id -> cow_id from the tracking results, and each video's timestamp: the file's `timestamp` (ISO text or a number; 0.0
        where it cannot be read), else the file's modification time."""
        mapping, timestamps = {}, {}
        tracking_dir = self.data_dir / "tracking"
        if not tracking_dir.exists():
            return mapping
        for tracking_file in tracking_dir.glob("*_tracking.json"):
            try:
                with open(tracking_file) as f:
                    data = json.load(f)
                video_id = data.get("video_id")
                if not video_id:
                    continue
                for reid in data.get("reid_results", []):
                    if reid.get("cow_id"):
                        mapping[video_id] = reid["cow_id"]
                        break
                timestamp = data.get("timestamp")
                if timestamp:
                    try:
                        timestamps[video_id] = (datetime.fromisoformat(timestamp.replace("Z", "+00:00")).timestamp() if isinstance(timestamp, str)
                                                else float(timestamp))
                    except Exception:  # noqa: BLE001 — the reference's bare except
                        timestamps[video_id] = 0.0
                else:
                    timestamps[video_id] = tracking_file.stat().st_mtime
            except Exception as e:  # noqa: BLE001
                print(f"  Error reading tracking file {tracking_file}: {e}")
        self.cow_id_mapping, self.video_timestamps = mapping, timestamps
        return mapping

    def get_cow_for_video(self, video_id):
        self.load_cow_id_mapping()
        return self.cow_id_mapping.get(video_id)

    # ---- main.py:172-243 -----------------------------------------------------------------------------------------------------------
    def _json(self, kind, video_id):
        path = self.data_dir / kind / f"{video_id}_{kind}.json"
        if not path.exists():
            return None
        with open(path) as f:
            return json.load(f)

    def extract_node_features(self, video_id):
        """{"pose" [10], "silhouette" [5], "embedding" [32], "meta" [3]}, float32, with the reference's defaults for what is missing"""
        features = {}
        tleap = self._json("tleap", video_id)
        if tleap is not None:
            loco = tleap.get("locomotion_features", {})
            features["pose"] = np.array([loco.get("back_arch_mean", 0), loco.get("back_arch_std", 0), loco.get("head_bob_magnitude", 0),
                                         loco.get("head_bob_frequency", 0), loco.get("front_leg_asymmetry", 0), loco.get("rear_leg_asymmetry", 0),
                                         loco.get("lameness_score", 0.5), loco.get("stride_fl_mean", 0), loco.get("stride_fr_mean", 0),
                                         loco.get("steadiness_score", 0.5)], dtype=np.float32)
        else:
            features["pose"] = np.zeros(self.POSE_FEATURES, dtype=np.float32)
        silhouette = np.zeros(self.SILHOUETTE_FEATURES, dtype=np.float32)
        sam3, yolo = self._json("sam3", video_id), self._json("yolo", video_id)
        if sam3 is not None:
            feats = sam3.get("features", {})
            silhouette[0], silhouette[1], silhouette[2] = feats.get("avg_area_ratio", 0), feats.get("avg_circularity", 0), feats.get("avg_aspect_ratio", 1)
        if yolo is not None:
            feats = yolo.get("features", {})
            silhouette[3], silhouette[4] = feats.get("avg_confidence", 0.5), feats.get("position_stability", 0.5)
        features["silhouette"] = silhouette
        embedding = np.zeros(self.EMBEDDING_DIM, dtype=np.float32)
        dinov3 = self._json("dinov3", video_id)
        if dinov3 is not None and len(dinov3.get("embedding", [])) > 0:
            e = np.array(dinov3["embedding"], dtype=np.float32)[:self.EMBEDDING_DIM]
            embedding[:len(e)] = e
        features["embedding"] = embedding
        features["meta"] = np.array([0.5, 1.0, 0.5], dtype=np.float32)
        return features

    def _node(self, features):
        return np.concatenate([features["pose"], features["silhouette"], features["embedding"], features["meta"]])

    # ---- main.py:245-299 -----------------------------------------------------------------------------------------------------------
    def collect_graph_data(self, filter_cow_id=None):
        """(node_features [N, 50], embeddings [N, 32], video_ids, cow_ids, timestamps) over the analysed videos (those with T-LEAP
        results, in the directory's order), of one cow where filter_cow_id is given; (None, None, [], [], []) where there are none."""
        self.load_cow_id_mapping()
        nodes, embeddings, video_ids, cow_ids, timestamps = [], [], [], [], []
        tleap_dir = self.data_dir / "tleap"
        if tleap_dir.exists():
            for result_file in tleap_dir.glob("*_tleap.json"):
                video_id = result_file.stem.replace("_tleap", "")
                cow_id = self.cow_id_mapping.get(video_id)
                if filter_cow_id is not None and cow_id != filter_cow_id:
                    continue
                features = self.extract_node_features(video_id)
                nodes.append(self._node(features)), embeddings.append(features["embedding"]), video_ids.append(video_id)
                cow_ids.append(cow_id), timestamps.append(self.video_timestamps.get(video_id, 0.0))
        if not nodes:
            return None, None, [], [], []
        return np.stack(nodes), np.stack(embeddings), video_ids, cow_ids, timestamps

    # ---- main.py:301-358: everything up to the model ---------------------------------------------------------------------------------
    def _graph(self, video_id):
        """The graph of one message: a dict with the prepared graph, the target index, the cow and the videos; None where the reference
        returns without writing; LmxError above the node limit."""
        cow = self.get_cow_for_video(video_id)
        node_features, embeddings, video_ids, cow_ids, timestamps = self.collect_graph_data(filter_cow_id=cow) if cow else self.collect_graph_data()
        if node_features is None:  # main.py:324-326: no analysed video at all
            print("  No video features available")
            return None
        if video_id not in video_ids:  # the message's video has no T-LEAP result yet: it joins the graph with the defaults
            features = self.extract_node_features(video_id)
            node_features, embeddings = np.vstack([node_features, self._node(features)]), np.vstack([embeddings, features["embedding"]])
            video_ids.append(video_id), cow_ids.append(cow), timestamps.append(self.video_timestamps.get(video_id, 0.0))
        if len(video_ids) > gfm.MAX_NODES:
            raise gfm.LmxError(f"GraphTransformerPipeline: the graph of {video_id} has {len(video_ids)} nodes; one workgroup holds at most "
                               f"{gfm.MAX_NODES}")
        ts = np.asarray(timestamps, np.float32) if cow else None  # torch.tensor(timestamps, dtype=torch.float32): float32 seconds
        graph = gfm.build_graph(self.model.cfg, node_features.astype(np.float32), embeddings.astype(np.float32), ts, self.K_NEIGHBORS)
        return {"graph": graph, "target": video_ids.index(video_id), "cow": cow, "video_ids": video_ids}

    def _score(self, video_ids, items):
        """Two calls for all graphs: S = 10, then eval mode for node scores and the attention towards each target"""
        graphs, targets = [it["graph"] for it in items], [it["target"] for it in items]
        mean, std, _ = self.model.score(graphs, [gfm.graph_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        _, nodes, attn = self.model.node_scores(graphs, targets)
        return mean.cpu().numpy(), std.cpu().numpy(), [n.cpu().numpy() for n in nodes], [a.cpu().numpy() for a in attn]

    def _results(self, video_id, item, cow_severity_score, uncertainty, node_preds, attn_to_target):
        target_idx, video_ids, cow, cfg = item["target"], item["video_ids"], item["cow"], self.model.cfg
        target_node_score = float(node_preds[target_idx])
        top_attending = np.argsort(attn_to_target)[-5:][::-1]
        return {"video_id": video_id, "cow_id": cow, "pipeline": "graph_transformer", "model": "CowLamenessGraphormer",
                "graph_prediction": cow_severity_score, "node_prediction": target_node_score, "cow_severity_score": cow_severity_score,
                "uncertainty": uncertainty, "prediction": int(target_node_score > 0.5), "cow_prediction": int(cow_severity_score > 0.5),
                "confidence": 1.0 - uncertainty,
                "graph_info": {"num_nodes": len(video_ids), "num_edges": int(len(item["graph"]["edges"])), "num_layers": cfg.n_layers,
                               "num_heads": cfg.n_heads, "hidden_dim": cfg.d_model, "has_temporal_edges": cow is not None,
                               "per_cow_graph": cow is not None},
                "attention_info": {"top_attending_nodes": [{"video_id": video_ids[i], "attention": float(attn_to_target[i])}
                                                           for i in top_attending if i != target_idx]},
                "videos_in_graph": video_ids}

    async def _finish(self, video_id, item, scores):
        results = self._results(video_id, item, *scores)
        results_file = self.results_dir / f"{video_id}_graph_transformer.json"
        with open(results_file, "w") as f:
            json.dump(results, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_graph_transformer", "pipeline.graph_transformer")
        await self.nats_client.publish(subject, {"video_id": video_id, "cow_id": item["cow"], "pipeline": "graph_transformer",
                                                 "results_path": str(results_file), "severity_score": results["node_prediction"],
                                                 "cow_severity_score": results["cow_severity_score"], "uncertainty": results["uncertainty"]})

    async def _process(self, ready):
        if not ready:
            return
        mean, std, nodes, attn = self._score([v for v, _ in ready], [it for _, it in ready])
        for i, (video_id, item) in enumerate(ready):
            await self._finish(video_id, item, (float(mean[i]), float(std[i]), nodes[i], attn[i]))

    async def process_video(self, video_data):
        video_id = video_data.get("video_id")
        if not video_id:
            return
        try:
            item = self._graph(video_id)
            await self._process([(video_id, item)] if item is not None else [])
        except Exception as e:  # noqa: BLE001 — the reference prints and writes nothing
            print(f"  Error in Graph Transformer for {video_id}: {e}")
            traceback.print_exc()

    async def process_videos(self, videos):
        """A backlog of graphs in the same two calls: each graph's file and message are those of process_video, bit for bit — a graph's
        bits depend on its own arrays and seed, never on the batch it rides in.  A graph above the node limit is refused on its own."""
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
                print(f"  Error in Graph Transformer for {video_id}: {e}")
        try:
            await self._process(ready)
        except Exception as e:  # noqa: BLE001
            print(f"  Error in Graph Transformer: {e}")
            traceback.print_exc()

    async def start(self):
        await self.nats_client.connect()
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_dinov3", "pipeline.dinov3")
        await self.nats_client.subscribe(subject, self.process_video)
