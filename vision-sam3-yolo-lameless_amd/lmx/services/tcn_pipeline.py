"""TCNPipeline — mirror of services/tcn-pipeline/app/main.py: the first consumer of `pipeline.tleap`.  The pose series of
`{id}_tleap.json` becomes 44 features per frame (20 keypoints relative to the bounding box, centroid, box area, centroid velocity),
centre-cropped or centre-padded to 125 steps; the TCN turns it into a severity score and an MC-dropout uncertainty, written to
`{id}_tcn.json` and published on `pipeline.tcn`.  `model.predict_with_uncertainty(x, n_samples=10)` (main.py:361: ten train-mode
forwards of about 45 launches each) is ONE launch of ``lmx.tcn.TcnScorer.score``, and ``process_videos`` scores a whole backlog of clips
in one launch.  The dropout bits are the library's (include/lmx.h), seeded per clip by ``lmx.tcn.clip_seed(video_id)`` — the first 8
bytes of the id's SHA-256, little-endian — so scoring a clip again gives the same bytes; parity with torch's generator is statistical."""
import json
import traceback
from pathlib import Path

import numpy as np
import torch

from .. import tcn
from . import runtime as R


class TCNPipeline:
    NUM_KEYPOINTS = 20          # from T-LEAP
    FEATURES_PER_KEYPOINT = 2   # x, y relative to the bounding box
    EXTRA_FEATURES = 4          # centroid_x, centroid_y, bbox_area, velocity
    TARGET_LENGTH = 125         # 5 s at 25 frames/s
    N_SAMPLES = 10

    def __init__(self, scorer, bus, config=None, tleap_dir="/app/data/results/tleap", results_dir="/app/data/results/tcn"):
        self.config = config or R.load_config()
        self.nats_client = bus
        self.model = scorer
        self.tleap_dir = Path(tleap_dir)
        self.results_dir = Path(results_dir)
        self.results_dir.mkdir(parents=True, exist_ok=True)

    def extract_features_from_tleap(self, tleap_data):
        """main.py:255-314: float32 [frames, 44], or None without pose_sequences.  The arithmetic is Python's (doubles) up to the cast;
        the velocity is the difference of the float32 centroid-x column."""
        pose_sequences = tleap_data.get("pose_sequences", [])
        if not pose_sequences:
            return None
        width = self.NUM_KEYPOINTS * self.FEATURES_PER_KEYPOINT
        rows = []
        for frame in pose_sequences:
            bbox = frame.get("bbox", [0, 0, 100, 100])
            bbox_w = bbox[2] - bbox[0] if len(bbox) > 2 else 100
            bbox_h = bbox[3] - bbox[1] if len(bbox) > 3 else 100
            row = []
            for kp in frame.get("keypoints", [])[:self.NUM_KEYPOINTS]:
                row += [(kp.get("x", 0) - bbox[0]) / max(bbox_w, 1), (kp.get("y", 0) - bbox[1]) / max(bbox_h, 1)]
            row += [0.0] * (width - len(row))
            centroid_x = (bbox[0] + bbox[2]) / 2 if len(bbox) > 2 else 0
            centroid_y = (bbox[1] + bbox[3]) / 2 if len(bbox) > 3 else 0
            rows.append(row + [centroid_x / 1280, centroid_y / 720, bbox_w * bbox_h / (1280 * 720), 0.0])
        features = np.array(rows, dtype=np.float32)
        if len(features) > 1:
            features[1:, -1] = np.diff(features[:, -4])
        return features

    def pad_or_truncate(self, features, target_length=125):
        """main.py:316-328: centre crop, or zero padding on both sides with the shorter half in front."""
        n = features.shape[0]
        if n >= target_length:
            start = (n - target_length) // 2
            return features[start:start + target_length]
        before = (target_length - n) // 2
        return np.pad(features, ((before, target_length - n - before), (0, 0)), mode="constant")

    def _features(self, video_id):
        """The padded series of one clip, or None where the reference returns without writing (no file, no features)."""
        path = self.tleap_dir / f"{video_id}_tleap.json"
        if not path.exists():
            print(f"  No T-LEAP results found for {video_id}")
            return None
        with open(path) as f:
            features = self.extract_features_from_tleap(json.load(f))
        if features is None or len(features) == 0:
            print(f"  No features extracted for {video_id}")
            return None
        return self.pad_or_truncate(features, target_length=self.TARGET_LENGTH)

    def _score(self, series, video_ids):
        """(severity, uncertainty) per clip from ONE launch over the stacked series."""
        x = torch.from_numpy(np.ascontiguousarray(np.stack(series, 0), np.float32)).to(self.model.device)
        mean, std, _ = self.model.score(x, [tcn.clip_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        return mean.cpu().numpy(), std.cpu().numpy()

    async def _finish(self, video_id, features, severity_score, uncertainty):
        results = {"video_id": video_id, "pipeline": "tcn", "severity_score": severity_score, "uncertainty": uncertainty,
                   "prediction": int(severity_score > 0.5), "confidence": 1.0 - uncertainty, "input_frames": features.shape[0],
                   "input_features": features.shape[1], "model_receptive_field": self.model.cfg.receptive_field}
        results_file = self.results_dir / f"{video_id}_tcn.json"
        with open(results_file, "w") as f:
            json.dump(results, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_tcn", "pipeline.tcn")
        await self.nats_client.publish(subject, {"video_id": video_id, "pipeline": "tcn", "results_path": str(results_file),
                                                 "severity_score": severity_score, "uncertainty": uncertainty})

    async def process_video(self, video_data):
        video_id = video_data.get("video_id")
        if not video_id:
            return
        try:
            features = self._features(video_id)
            if features is None:
                return
            mean, std = self._score([features], [video_id])
            await self._finish(video_id, features, float(mean[0]), float(std[0]))
        except Exception as e:  # noqa: BLE001 — main.py:397-400 prints and writes nothing
            print(f"  Error in TCN pipeline for {video_id}: {e}")
            traceback.print_exc()

    async def process_videos(self, videos):
        """Many clips in one launch (re-scoring a backlog): each clip's file and message are those of process_video, bit for bit — a
        clip's bits depend on its own series and seed, never on the batch it rides in."""
        try:
            ready = []
            for video_data in videos:
                video_id = video_data.get("video_id")
                features = self._features(video_id) if video_id else None
                if features is not None:
                    ready.append((video_id, features))
            if not ready:
                return
            mean, std = self._score([f for _, f in ready], [v for v, _ in ready])
            for (video_id, features), m, s in zip(ready, mean, std):
                await self._finish(video_id, features, float(m), float(s))
        except Exception as e:  # noqa: BLE001
            print(f"  Error in TCN pipeline: {e}")
            traceback.print_exc()

    async def start(self):
        await self.nats_client.connect()
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_tleap", "pipeline.tleap")
        await self.nats_client.subscribe(subject, self.process_video)
