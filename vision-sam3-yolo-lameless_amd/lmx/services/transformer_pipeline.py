"""TransformerPipeline — mirror of services/transformer-pipeline/app/main.py:240-508, the TCN's twin on `pipeline.tleap`.  The pose
series of `{id}_tleap.json` becomes the TCN's 44 features per frame and a key-padding mask (a frame whose mean keypoint confidence times
its detection confidence is below 0.3 is masked), centre-cropped or centre-padded to 125 steps (padding is masked); the gait transformer
turns it into a severity score, an MC-dropout uncertainty and a temporal saliency, written to `{id}_transformer.json` and published on
`pipeline.transformer`.  `model.predict_with_uncertainty(x, mask, n_samples=10)` and `model.get_attention_weights(x)` (main.py:426-441:
eleven forwards of a few hundred launches each) are TWO launches of ``lmx.xfm.XfmScorer`` — S = 10 with the mask, eval mode without it
for the saliency, as main.py:435 passes none — and ``process_videos`` scores a whole backlog of clips in the same two launches.  The
dropout bits are the library's (include/lmx.h), seeded per clip by ``lmx.xfm.clip_seed(video_id)``; parity with torch's generator is
statistical.  A clip whose every step is masked has no defined score (torch gives NaN): it is refused and nothing is written."""
import json
import traceback
from pathlib import Path

import numpy as np
import torch

from .. import xfm
from . import runtime as R


class TransformerPipeline:
    NUM_KEYPOINTS = 20          # from T-LEAP
    FEATURES_PER_KEYPOINT = 2   # x, y relative to the bounding box
    EXTRA_FEATURES = 4          # centroid_x, centroid_y, bbox_area, velocity
    TARGET_LENGTH = 125         # 5 s at 25 frames/s
    N_SAMPLES = 10
    MASK_BELOW = 0.3            # mean keypoint confidence x detection confidence
    SALIENCY_SHOWN = 20

    def __init__(self, scorer, bus, config=None, tleap_dir="/app/data/results/tleap", results_dir="/app/data/results/transformer"):
        self.config = config or R.load_config()
        self.nats_client = bus
        self.model = scorer
        self.tleap_dir = Path(tleap_dir)
        self.results_dir = Path(results_dir)
        self.results_dir.mkdir(parents=True, exist_ok=True)

    def extract_features_from_tleap(self, tleap_data):
        """main.py:303-372: (float32 [frames, 44], bool [frames], True = masked), or (None, None) without pose_sequences.  The
        features are the TCN's; the confidence of a frame is np.mean over its 20 keypoint confidences (0.5 where a keypoint has none, 0
        for a missing keypoint) times the detection confidence, cast to float32."""
        pose_sequences = tleap_data.get("pose_sequences", [])
        if not pose_sequences:
            return None, None
        width = self.NUM_KEYPOINTS * self.FEATURES_PER_KEYPOINT
        rows, confidences = [], []
        for frame in pose_sequences:
            bbox = frame.get("bbox", [0, 0, 100, 100])
            bbox_w = bbox[2] - bbox[0] if len(bbox) > 2 else 100
            bbox_h = bbox[3] - bbox[1] if len(bbox) > 3 else 100
            row, conf = [], []
            for kp in frame.get("keypoints", [])[:self.NUM_KEYPOINTS]:
                row += [(kp.get("x", 0) - bbox[0]) / max(bbox_w, 1), (kp.get("y", 0) - bbox[1]) / max(bbox_h, 1)]
                conf.append(kp.get("confidence", 0.5))
            conf += [0.0] * ((width - len(row)) // 2)
            row += [0.0] * (width - len(row))
            centroid_x = (bbox[0] + bbox[2]) / 2 if len(bbox) > 2 else 0
            centroid_y = (bbox[1] + bbox[3]) / 2 if len(bbox) > 3 else 0
            rows.append(row + [centroid_x / 1280, centroid_y / 720, bbox_w * bbox_h / (1280 * 720), 0.0])
            confidences.append(np.mean(conf) * frame.get("detection_confidence", 1.0))
        features = np.array(rows, dtype=np.float32)
        if len(features) > 1:
            features[1:, -1] = np.diff(features[:, -4])
        return features, np.array(confidences, dtype=np.float32) < np.float32(self.MASK_BELOW)

    def pad_or_truncate(self, features, mask, target_length=125):
        """main.py:374-392: centre crop, or padding on both sides with the shorter half in front: zeros for the features, True for the mask."""
        n = features.shape[0]
        if n >= target_length:
            start = (n - target_length) // 2
            return features[start:start + target_length], mask[start:start + target_length]
        before = (target_length - n) // 2
        after = target_length - n - before
        return (np.pad(features, ((before, after), (0, 0)), mode="constant"), np.pad(mask, (before, after), mode="constant", constant_values=True))

    def _features(self, video_id):
        """(padded series, padded mask) of one clip, or None where the reference returns without writing (no file, no features) and
        where every step is masked"""
        path = self.tleap_dir / f"{video_id}_tleap.json"
        if not path.exists():
            print(f"  No T-LEAP results found for {video_id}")
            return None
        with open(path) as f:
            features, mask = self.extract_features_from_tleap(json.load(f))
        if features is None or len(features) == 0:
            print(f"  No features extracted for {video_id}")
            return None
        features, mask = self.pad_or_truncate(features, mask, target_length=self.TARGET_LENGTH)
        if mask.all():
            print(f"  Every step of {video_id} is masked (low confidence): no score")
            return None
        return features, mask

    def _score(self, series, masks, video_ids):
        """(severity, uncertainty, saliency) per clip from TWO launches over the stacked series"""
        x = torch.from_numpy(np.ascontiguousarray(np.stack(series, 0), np.float32)).to(self.model.device)
        m = torch.from_numpy(np.ascontiguousarray(np.stack(masks, 0)).astype(np.uint8)).to(self.model.device)
        mean, std, _ = self.model.score(x, m, [xfm.clip_seed(v) for v in video_ids], n_samples=self.N_SAMPLES)
        return mean.cpu().numpy(), std.cpu().numpy(), self.model.saliency(x).cpu().numpy()

    async def _finish(self, video_id, features, mask, severity_score, uncertainty, saliency):
        temporal_saliency = [float(v) for v in saliency]
        cfg = self.model.cfg
        results = {"video_id": video_id, "pipeline": "transformer", "severity_score": severity_score, "uncertainty": uncertainty,
                   "prediction": int(severity_score > 0.5), "confidence": 1.0 - uncertainty, "input_frames": features.shape[0],
                   "input_features": features.shape[1], "masked_frames": int(mask.sum()),
                   "temporal_saliency": temporal_saliency[:self.SALIENCY_SHOWN] if len(temporal_saliency) > self.SALIENCY_SHOWN else temporal_saliency,
                   "model_info": {"d_model": cfg.d_model, "num_layers": cfg.n_layers, "nhead": cfg.n_heads}}
        results_file = self.results_dir / f"{video_id}_transformer.json"
        with open(results_file, "w") as f:
            json.dump(results, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_transformer", "pipeline.transformer")
        await self.nats_client.publish(subject, {"video_id": video_id, "pipeline": "transformer", "results_path": str(results_file),
                                                 "severity_score": severity_score, "uncertainty": uncertainty})

    async def process_video(self, video_data):
        video_id = video_data.get("video_id")
        if not video_id:
            return
        try:
            ready = self._features(video_id)
            if ready is None:
                return
            mean, std, sal = self._score([ready[0]], [ready[1]], [video_id])
            await self._finish(video_id, ready[0], ready[1], float(mean[0]), float(std[0]), sal[0])
        except Exception as e:  # noqa: BLE001 — main.py:482-485 prints and writes nothing
            print(f"  Error in Transformer pipeline for {video_id}: {e}")
            traceback.print_exc()

    async def process_videos(self, videos):
        """Many clips in two launches (re-scoring a backlog): each clip's file and message are those of process_video, bit for bit — a
        clip's bits depend on its own series, mask and seed, never on the batch it rides in."""
        try:
            ready = []
            for video_data in videos:
                video_id = video_data.get("video_id")
                got = self._features(video_id) if video_id else None
                if got is not None:
                    ready.append((video_id,) + got)
            if not ready:
                return
            mean, std, sal = self._score([f for _, f, _ in ready], [m for _, _, m in ready], [v for v, _, _ in ready])
            for (video_id, features, mask), m, s, a in zip(ready, mean, std, sal):
                await self._finish(video_id, features, mask, float(m), float(s), a)
        except Exception as e:  # noqa: BLE001
            print(f"  Error in Transformer pipeline: {e}")
            traceback.print_exc()

    async def start(self):
        await self.nats_client.connect()
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_tleap", "pipeline.tleap")
        await self.nats_client.subscribe(subject, self.process_video)
