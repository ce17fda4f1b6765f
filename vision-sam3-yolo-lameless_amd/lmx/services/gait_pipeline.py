"""GaitPipeline — what the two consumers of `pipeline.tleap` that score a pose series (``TCNPipeline``, ``TransformerPipeline``) do
alike: 44 features per frame from `{id}_tleap.json` (20 keypoints relative to the bounding box, centroid, box area, centroid
velocity), centre-cropped or centre-padded to 125 steps; one clip per message or a whole backlog in one batch; the result written to
`{id}_{NAME}.json` and published on `pipeline.{NAME}`.  A clip is the tuple of its padded arrays (`_clip`), scored by `_score` and turned
into the result dictionary by `_results`: those three are the subclass's.

A consumer is EITHER subscribed to the bus (`start`: it reads `{id}_tleap.json` per message) OR handed clips by a ``TLEAPPipeline`` that
lists it among its `consumers` (`process_clip` / `process_clips`: the arrays come from the device, no file is read) — not both, or every
clip is scored and published twice."""
import json
import traceback
from pathlib import Path

import numpy as np

from . import runtime as R


class GaitPipeline:
    NUM_KEYPOINTS = 20          # from T-LEAP
    FEATURES_PER_KEYPOINT = 2   # x, y relative to the bounding box
    EXTRA_FEATURES = 4          # centroid_x, centroid_y, bbox_area, velocity
    TARGET_LENGTH = 125         # 5 s at 25 frames/s
    N_SAMPLES = 10
    NAME = None                 # "tcn": the results' directory, file suffix, `pipeline` field and subject
    LABEL = None                # "TCN": the name in printed messages
    USES_MASK = False           # the clip tuple is (series,) or, with the key-padding mask, (series, mask)

    def __init__(self, scorer, bus, config=None, tleap_dir="/app/data/results/tleap", results_dir=None):
        self.config = config or R.load_config()
        self.nats_client = bus
        self.model = scorer
        self.tleap_dir = Path(tleap_dir)
        self.results_dir = Path(results_dir if results_dir is not None else f"/app/data/results/{self.NAME}")
        self.results_dir.mkdir(parents=True, exist_ok=True)

    def _frame_row(self, frame):
        """The 44 features of one frame (tcn-pipeline main.py:255-314, transformer-pipeline main.py:303-372) in Python's doubles; the
        velocity stays 0 until _feature_matrix has the float32 column to difference."""
        width = self.NUM_KEYPOINTS * self.FEATURES_PER_KEYPOINT
        bbox = frame.get("bbox", [0, 0, 100, 100])
        bbox_w = bbox[2] - bbox[0] if len(bbox) > 2 else 100
        bbox_h = bbox[3] - bbox[1] if len(bbox) > 3 else 100
        row = []
        for kp in frame.get("keypoints", [])[:self.NUM_KEYPOINTS]:
            row += [(kp.get("x", 0) - bbox[0]) / max(bbox_w, 1), (kp.get("y", 0) - bbox[1]) / max(bbox_h, 1)]
        row += [0.0] * (width - len(row))
        centroid_x = (bbox[0] + bbox[2]) / 2 if len(bbox) > 2 else 0
        centroid_y = (bbox[1] + bbox[3]) / 2 if len(bbox) > 3 else 0
        return row + [centroid_x / 1280, centroid_y / 720, bbox_w * bbox_h / (1280 * 720), 0.0]

    def _feature_matrix(self, pose_sequences):
        """float32 [frames, 44]; the velocity is the difference of the float32 centroid-x column"""
        features = np.array([self._frame_row(frame) for frame in pose_sequences], dtype=np.float32)
        if len(features) > 1:
            features[1:, -1] = np.diff(features[:, -4])
        return features

    @staticmethod
    def _centre(a, target_length, fill):
        """Centre crop of `a` along its first axis, or `fill` on both sides with the shorter half in front."""
        n = a.shape[0]
        if n >= target_length:
            start = (n - target_length) // 2
            return a[start:start + target_length]
        before = (target_length - n) // 2
        return np.pad(a, ((before, target_length - n - before),) + ((0, 0),) * (a.ndim - 1), mode="constant", constant_values=fill)

    def _features(self, video_id):
        """The clip of one video, or None where the reference returns without writing (no file, no features)."""
        path = self.tleap_dir / f"{video_id}_tleap.json"
        if not path.exists():
            print(f"  No T-LEAP results found for {video_id}")
            return None
        with open(path) as f:
            clip = self._clip(json.load(f))
        if clip is None:
            print(f"  No features extracted for {video_id}")
        return clip

    async def _finish(self, video_id, clip, scores):
        results = self._results(video_id, *clip, *scores)
        results_file = self.results_dir / f"{video_id}_{self.NAME}.json"
        with open(results_file, "w") as f:
            json.dump(results, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get(f"pipeline_{self.NAME}", f"pipeline.{self.NAME}")
        await self.nats_client.publish(subject, {"video_id": video_id, "pipeline": self.NAME, "results_path": str(results_file),
                                                 "severity_score": results["severity_score"], "uncertainty": results["uncertainty"]})

    async def _process(self, ready):
        """Score the (video_id, clip) pairs in one batch and finish each: (severity, uncertainty) as Python floats, then what else
        _score returns per clip."""
        if not ready:
            return
        scores = self._score([v for v, _ in ready], *[list(arrays) for arrays in zip(*[clip for _, clip in ready])])
        for i, (video_id, clip) in enumerate(ready):
            await self._finish(video_id, clip, (float(scores[0][i]), float(scores[1][i])) + tuple(s[i] for s in scores[2:]))

    async def process_video(self, video_data):
        video_id = video_data.get("video_id")
        if not video_id:
            return
        try:
            clip = self._features(video_id)
            await self._process([(video_id, clip)] if clip is not None else [])
        except Exception as e:  # noqa: BLE001 — the reference prints and writes nothing
            print(f"  Error in {self.LABEL} pipeline for {video_id}: {e}")
            traceback.print_exc()

    async def process_videos(self, videos):
        """Many clips in one batch (re-scoring a backlog): each clip's file and message are those of process_video, bit for bit — a
        clip's bits depend on its own arrays and seed, never on the batch it rides in."""
        try:
            ready = []
            for video_data in videos:
                video_id = video_data.get("video_id")
                clip = self._features(video_id) if video_id else None
                if clip is not None:
                    ready.append((video_id, clip))
            await self._process(ready)
        except Exception as e:  # noqa: BLE001
            print(f"  Error in {self.LABEL} pipeline: {e}")
            traceback.print_exc()

    def _accept(self, video_id, clip):
        """The clip tuple of a handed-over (series, mask), or None where _features would have returned None for its file."""
        return tuple(clip[:2 if self.USES_MASK else 1])

    async def process_clips(self, clips):
        """(video_id, (series f32 [125, 44], mask bool [125])) pairs from ``TLEAPPipeline``: the same `_process` as for clips read from
        `{id}_tleap.json` — same file, same message, bit for bit — without the JSON read.  Never raises, like process_video."""
        try:
            ready = [(video_id, self._accept(video_id, clip)) for video_id, clip in clips]
            await self._process([(v, c) for v, c in ready if c is not None])
        except Exception as e:  # noqa: BLE001
            print(f"  Error in {self.LABEL} pipeline: {e}")
            traceback.print_exc()

    async def process_clip(self, video_id, clip):
        await self.process_clips([(video_id, clip)])

    async def start(self):
        await self.nats_client.connect()
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_tleap", "pipeline.tleap")
        await self.nats_client.subscribe(subject, self.process_video)
