"""TLEAPPipeline — mirror of services/tleap-pipeline/app/main.py:316-541, the link between the detector and the two gait consumers: every
max(1, int(fps // 5))-th frame of a clip goes through the pose model (``trained``: a detector with a Pose head) or the plain detector
(``heuristic``: cow boxes, keypoints estimated from each box) at confidence 0.3, and ONE launch of ``lmx.tleap.PoseSeries`` turns the
detector's outputs, where they lie in HBM, into tleap's pose records, the 125 x 44 series and the key-padding mask.  The records are
downloaded once and written as `{id}_tleap.json` with the reference's keys and key order; `pipeline.tleap` is published; then each of
`consumers` (``TCNPipeline`` / ``TransformerPipeline``) is handed the clip's series and mask from the device, so frames become scores
without host arithmetic and without the JSON round trip.  ``process_videos`` handles a backlog in one series launch and one launch per
consumer stage.  The kernel is small; the pose model is where a clip's time goes.

Kept quirks: pose_sequences holds one row per DETECTION (main.py:479-486), so two cows in a frame are two steps of the series; the
locomotion features look keypoints up by the heuristic names, so a trained clip has none; a heuristic frame without a cow gets one
assumed box; fps stays a float here (`time`, the sampling interval) where the other services truncate it."""
import json
import traceback
from pathlib import Path

import numpy as np
import torch

from .. import tleap
from . import runtime as R
from .pose import KEYPOINT_NAMES

# main.py:66-94 — the skeleton the reference writes into every result (indices into ITS docstring's keypoint order) and its colours (BGR)
COW_SKELETON = [(0, 1), (0, 2), (1, 2), (0, 3), (1, 4), (2, 17), (17, 18), (18, 19), (5, 9), (6, 10), (7, 11), (8, 12), (9, 13), (10, 14),
                (11, 15), (12, 16)]
SKELETON_COLORS = {"face": (0, 255, 255), "spine": (0, 255, 0), "front_left": (255, 0, 0), "front_right": (0, 165, 255),
                   "back_left": (255, 0, 255), "back_right": (0, 255, 255)}
MAX_ROWS = 1 << 24  # frames x max_det of one series launch (include/lmx.h)


def compute_locomotion_features(pose_sequences):
    """main.py:338-436, numpy float64 like the reference (so the JSON carries numpy's bits); ``lmx_h_tleap_locomotion`` is the same
    over the records for a C caller, with sequential sums."""
    if not pose_sequences or len(pose_sequences) < 2:
        return {}
    features = {}
    head_positions, spine_angles = [], []
    hoof_positions = {"fl": [], "fr": [], "rl": [], "rr": []}
    for frame_data in pose_sequences:
        keypoints = frame_data.get("keypoints", [])
        if len(keypoints) < 20:
            continue
        kp_dict = {kp["name"]: kp for kp in keypoints}
        nose = kp_dict.get("nose", {})
        if nose.get("confidence", 0) > 0.3:
            head_positions.append(nose.get("y", 0))
        throat, withers, tailbase = kp_dict.get("throat", {}), kp_dict.get("withers", {}), kp_dict.get("tailbase", {})
        if all(k.get("confidence", 0) > 0.3 for k in (throat, withers, tailbase)):
            v1 = np.array([throat["x"] - withers["x"], throat["y"] - withers["y"]])
            v2 = np.array([tailbase["x"] - withers["x"], tailbase["y"] - withers["y"]])
            cos_angle = np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2) + 1e-6)
            spine_angles.append(np.degrees(np.arccos(np.clip(cos_angle, -1, 1))))
        for leg, name in (("fl", "left_front_paw"), ("fr", "right_front_paw"), ("rl", "left_back_paw"), ("rr", "right_back_paw")):
            kp = kp_dict.get(name, {})
            if kp.get("confidence", 0) > 0.3:
                hoof_positions[leg].append(kp.get("x", 0))
    if spine_angles:
        features["back_arch_mean"] = float(np.mean(spine_angles))
        features["back_arch_std"] = float(np.std(spine_angles))
        features["back_arch_score"] = float(1.0 - (np.mean(spine_angles) / 180.0))
    if len(head_positions) > 1:
        features["head_bob_magnitude"] = float(np.std(head_positions))
        head_diff = np.diff(head_positions)
        features["head_bob_frequency"] = float(np.sum(np.abs(np.diff(np.sign(head_diff)))) / 2)
        features["head_bob_score"] = float(min(1.0, features["head_bob_magnitude"] / 50.0))
    for leg, positions in hoof_positions.items():
        if len(positions) > 1:
            strides = np.diff(positions)
            features[f"stride_{leg}_mean"] = float(np.mean(np.abs(strides)))
            features[f"stride_{leg}_std"] = float(np.std(strides))
    for key, a, b in (("front_leg_asymmetry", "stride_fl_mean", "stride_fr_mean"), ("rear_leg_asymmetry", "stride_rl_mean", "stride_rr_mean")):
        if a in features and b in features:
            features[key] = float(abs(features[a] - features[b]) / (features[a] + features[b] + 1e-6))
    components = [features[k] for k in ("back_arch_score", "head_bob_score", "front_leg_asymmetry", "rear_leg_asymmetry") if k in features]
    if components:
        features["lameness_score"] = float(np.mean(components))
    return features


def pose_sequences_from_records(records, frame_ids, fps, trained):
    """A clip's records (numpy, lmx.tleap.RECORD) -> the reference's pose_sequences (main.py:479-486): `frame` is the decoded frame's
    number, keypoint dicts are name, x, y, confidence in both modes (main.py:166 and :221); the trained withers fallback keeps its name."""
    names = KEYPOINT_NAMES if trained else tleap.HEURISTIC_NAMES
    out = []
    for r in records:
        fid = frame_ids[int(r["frame"])]
        kps = [{"name": names[i], "x": float(k[0]), "y": float(k[1]), "confidence": float(k[2])} for i, k in enumerate(r["keypoints"][:int(r["n_kp"])])]
        out.append({"frame": fid, "time": fid / fps if fps > 0 else 0, "bbox": [float(v) for v in r["bbox"]], "keypoints": kps,
                    "detection_confidence": float(r["confidence"])})
    return out


class TLEAPPipeline:
    CONF = 0.3  # main.py:150, :273

    def __init__(self, detector, bus, config=None, results_dir="/app/data/results/tleap", consumers=(), videos_dir="/app/data/videos", batch=32,
                 conf=None, backend="device"):
        """detector: lmx.yolo.YoloDetector (a Pose head makes the model type `trained`); consumers: GaitPipeline instances that are handed
        each clip after its message (they must not also be subscribed to the bus); backend "host" runs the series through
        lmx_h_tleap_series on a detector that returns CPU tensors (no GPU)."""
        self.config = config or R.load_config()
        self.nats_client = bus
        self.detector = detector
        self.use_trained_model = detector.cfg.kpt_shape is not None
        names = getattr(detector, "names", {}) or {}
        self.cow_classes = sorted({19} | {int(i) for i, n in names.items() if "cow" in str(n).lower()})  # main.py:282
        self.series = tleap.PoseSeries("trained" if self.use_trained_model else "heuristic", self.cow_classes, backend=backend)
        self.results_dir = Path(results_dir)
        self.results_dir.mkdir(parents=True, exist_ok=True)
        self.videos_dir = Path(videos_dir)
        self.consumers = list(consumers)
        self.batch, self.conf = batch, self.CONF if conf is None else conf

    @property
    def model_type(self):
        return "trained" if self.use_trained_model else "heuristic"

    def _video_path(self, video_data):
        """main.py:441-454"""
        video_id = video_data.get("video_id")
        processed_path = Path(video_data.get("processed_path", ""))
        if processed_path.is_file():
            return processed_path
        found = sorted(self.videos_dir.glob(f"{video_id}.*")) if self.videos_dir.is_dir() else []
        if found:
            return found[0]
        print(f"Video not found: {video_id}")
        return None

    def _detect(self, path):
        """The sampled frames of one clip through the detector, `batch` at a time: (clip facts, the detector's tensors on its device)."""
        clip = R.Clip.open(path)
        fps = clip.fps_exact
        interval = max(1, int(fps // 5))  # main.py:469, on the unrounded fps
        ids, parts = [], []
        dev = self.detector.device
        for chunk, host in clip.batches(interval, self.batch):
            frames = torch.from_numpy(host).to(dev)
            if self.use_trained_model:
                b, s, c, _, n, k = self.detector.detect_pose(frames, conf=self.conf)
            else:
                (b, s, c, _, n), k = self.detector.detect(frames, conf=self.conf), None
            ids += chunk
            parts.append((b, s, c, n, k))
        return {"fps": fps, "total_frames": clip.total_frames, "frame_ids": ids, "hw": clip.frame_hw}, parts

    def _launches(self, clips):
        """Group the clips that share a frame size and a max_det into series launches (one, for a backlog from one camera)."""
        groups = {}
        for i, (facts, parts) in enumerate(clips):
            if parts:
                groups.setdefault((tuple(facts["hw"]), int(parts[0][0].shape[1])), []).append(i)
        for (hw, max_det), members in groups.items():
            cap, cur, frames = MAX_ROWS // max_det, [], 0
            for i in members:
                nf = len(clips[i][0]["frame_ids"])
                if cur and frames + nf > cap:
                    yield hw, max_det, cur
                    cur, frames = [], 0
                cur.append(i)
                frames += nf
            yield hw, max_det, cur

    def pose_series(self, clips):
        """clips: [(facts, parts)] of _detect -> per clip (records numpy or None, series f32 [125, 44] numpy, mask bool [125] numpy): ONE
        series launch and ONE download of the records per group of _launches."""
        out = [None] * len(clips)
        for hw, max_det, members in self._launches(clips):
            cat = [torch.cat([p[j] for i in members for p in clips[i][1]], 0).contiguous() for j in range(4)]
            kpts = torch.cat([p[4] for i in members for p in clips[i][1]], 0).contiguous() if self.use_trained_model else None
            first = np.cumsum([0] + [len(clips[i][0]["frame_ids"]) for i in members])
            rows, records, series, mask = self.series(*cat, kpts, hw, first)
            counts = rows.cpu().numpy()
            index = np.concatenate([np.arange(int(first[c]) * max_det, int(first[c]) * max_det + int(counts[c])) for c in range(len(members))])
            taken = records.index_select(0, torch.from_numpy(index).to(records.device)).cpu().numpy().view(tleap.RECORD).reshape(-1)
            series, mask = series.cpu().numpy(), mask.cpu().numpy().astype(bool)
            at = np.cumsum([0] + [int(v) for v in counts])
            for c, i in enumerate(members):
                out[i] = (taken[at[c]:at[c + 1]], series[c], mask[c])
        return out

    def results(self, video_id, facts, records):
        """The dictionary of main.py:499-513, keys in its order."""
        seq = pose_sequences_from_records(records, facts["frame_ids"], facts["fps"], self.use_trained_model) if records is not None else []
        return {"video_id": video_id, "pipeline": "tleap", "total_frames": facts["total_frames"], "fps": facts["fps"],
                "frames_processed": len(seq), "pose_sequences": seq, "locomotion_features": compute_locomotion_features(seq),
                "model_type": self.model_type,
                "skeleton_definition": {"keypoint_names": KEYPOINT_NAMES, "skeleton_connections": COW_SKELETON,
                                        "colors": {k: list(v) for k, v in SKELETON_COLORS.items()}}}

    async def write_and_publish(self, video_id, result):
        """main.py:515-530: `{id}_tleap.json` (indent 2) and the `pipeline.tleap` message."""
        results_file = self.results_dir / f"{video_id}_tleap.json"
        with open(results_file, "w") as f:
            json.dump(result, f, indent=2)
        subject = self.config.get("nats", {}).get("subjects", {}).get("pipeline_tleap", "pipeline.tleap")
        await self.nats_client.publish(subject, {"video_id": video_id, "pipeline": "tleap", "results_path": str(results_file),
                                                 "features": result["locomotion_features"], "frames_processed": result["frames_processed"],
                                                 "model_type": result["model_type"]})

    async def process_videos(self, videos):
        """A backlog: every clip through the detector, ONE series launch, then per clip its file and message, then each consumer scores
        all clips in one batch.  Each clip's file and message are those of process_video, bit for bit."""
        try:
            ready = []
            for video_data in videos:
                video_id = video_data.get("video_id")
                try:
                    path = self._video_path(video_data)
                    if path is not None:
                        ready.append((video_id, self._detect(path)))
                except Exception as e:  # noqa: BLE001 — one unreadable clip does not stop the backlog
                    print(f"Error in T-LEAP pipeline for {video_id}: {e}")
                    traceback.print_exc()
            outs = self.pose_series([clip for _, clip in ready])
            handed = []
            for (video_id, (facts, _)), out in zip(ready, outs):
                records, series, mask = out if out is not None else (None, None, None)
                await self.write_and_publish(video_id, self.results(video_id, facts, records))
                if records is not None and len(records):  # without rows the consumers find no features in the file either
                    handed.append((video_id, (series, mask)))
            for consumer in self.consumers:
                await consumer.process_clips(handed)
        except Exception as e:  # noqa: BLE001 — the reference never raises out of the handler (main.py:538-541)
            print(f"Error in T-LEAP pipeline: {e}")
            traceback.print_exc()

    async def process_video(self, video_data):
        await self.process_videos([video_data])

    async def start(self):
        await self.nats_client.connect()
        await self.nats_client.subscribe(self.config["nats"]["subjects"]["video_preprocessed"], self.process_video)
