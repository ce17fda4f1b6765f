"""TLEAPPipeline with backend="host" and a fake detector that returns the fixture's tensors: the written `{id}_tleap.json` and the
`pipeline.tleap` message carry what the reference's own functions returned (tests/golden/tleap_reference.json).  No GPU."""
import asyncio
import json
import os

import numpy as np
import pytest
import torch

import tleapref as R
from lmx.services import TLEAPPipeline
from lmx.services import runtime as RT

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tleap_reference.json")))
LOOSE = ("back_arch_mean", "back_arch_std", "back_arch_score", "lameness_score")  # arccos and the 2-norm go through libm / SVML


class FakeDetector:
    """Hands out the fixture's per-frame arrays in the order the frames arrive (the service samples in ascending order)."""
    device = torch.device("cpu")

    def __init__(self, case):
        self.arrays = R.case_arrays(case)
        self.cfg = type("Cfg", (), {"kpt_shape": (case["K"], case["ndim"]) if case.get("K") else None})()
        self.names = {int(k): v for k, v in case.get("names", {}).items()}
        self.at, self.confs = 0, []

    def _next(self, frames, conf):
        a, b = self.at, self.at + frames.shape[0]
        self.at = b
        self.confs.append(conf)
        boxes, scores, cls, counts, kpts = (torch.from_numpy(np.ascontiguousarray(x[a:b])) if x is not None else None for x in self.arrays)
        return boxes, scores, cls, torch.zeros_like(cls), counts, kpts

    def detect(self, frames, conf=0.25):
        return self._next(frames, conf)[:5]

    def detect_pose(self, frames, conf=0.25):
        return self._next(frames, conf)


def serve(case, tmp_path, monkeypatch, video_id="cow_7"):
    n = case["frame_ids"][-1] + 3  # a few frames beyond the last sampled one
    frames = np.broadcast_to(np.zeros((1, case["h"], case["w"], 3), np.uint8), (n, case["h"], case["w"], 3))
    monkeypatch.setattr(RT.Clip, "open", staticmethod(lambda path: RT.Clip(path, frames, case["fps"])))
    video = tmp_path / f"{video_id}.npz"
    video.write_bytes(b"stand-in")
    bus, det = RT.InProcessBus(), FakeDetector(case)
    svc = TLEAPPipeline(det, bus, config=RT.load_config(str(tmp_path / "none.yaml")), results_dir=tmp_path / "tleap", batch=4, backend="host")
    asyncio.run(svc.process_video({"video_id": video_id, "processed_path": str(video)}))
    return svc, det, bus, n


@pytest.mark.parametrize("name", sorted(FIXTURE["cases"]))
def test_service_writes_the_reference_records(name, tmp_path, monkeypatch):
    case = FIXTURE["cases"][name]
    svc, det, bus, n = serve(case, tmp_path, monkeypatch)
    assert det.at == len(case["frames"]) and set(det.confs) == {0.3}
    doc = json.load(open(tmp_path / "tleap" / "cow_7_tleap.json"))
    assert list(doc) == ["video_id", "pipeline", "total_frames", "fps", "frames_processed", "pose_sequences", "locomotion_features", "model_type",
                         "skeleton_definition"]
    want = R.pose_sequences(case["detections"], case["frame_ids"], case["fps"])
    assert doc["pose_sequences"] == want and doc["frames_processed"] == len(want)
    assert all(list(row) == ["frame", "time", "bbox", "keypoints", "detection_confidence"] for row in doc["pose_sequences"])
    assert all(list(kp) == ["name", "x", "y", "confidence"] for row in doc["pose_sequences"] for kp in row["keypoints"])
    assert (doc["video_id"], doc["pipeline"], doc["total_frames"], doc["fps"], doc["model_type"]) == ("cow_7", "tleap", n, case["fps"], case["mode"])
    assert doc["skeleton_definition"] == {"keypoint_names": FIXTURE["keypoint_names"], "skeleton_connections": FIXTURE["skeleton"], "colors": FIXTURE["colors"]}
    features = next(e["features"] for e in FIXTURE["locomotion"] if e["case"] == name and e["rows"] == len(want))
    assert list(doc["locomotion_features"]) == list(features)
    for k, v in features.items():
        assert doc["locomotion_features"][k] == (pytest.approx(v, rel=1e-12, abs=0) if k in LOOSE else v), k
    (subject, msg), = bus.published
    assert subject == "pipeline.tleap" and list(msg) == ["video_id", "pipeline", "results_path", "features", "frames_processed", "model_type"]
    assert msg["features"] == doc["locomotion_features"] and msg["results_path"] == str(tmp_path / "tleap" / "cow_7_tleap.json")
    text = open(tmp_path / "tleap" / "cow_7_tleap.json").read()
    assert text == json.dumps(doc, indent=2)


def test_sampling_uses_the_unrounded_fps(tmp_path, monkeypatch):
    """29.97 frames/s: every int(29.97 // 5) = 5th frame, time = frame / 29.97; Clip keeps int(fps) for the other services"""
    case = FIXTURE["cases"]["heuristic_walk"]
    assert case["fps"] == 29.97 and case["frame_ids"] == list(range(0, 60, 5))
    serve(case, tmp_path, monkeypatch)
    doc = json.load(open(tmp_path / "tleap" / "cow_7_tleap.json"))
    assert [r["frame"] for r in doc["pose_sequences"]] == case["frame_ids"] and doc["pose_sequences"][3]["time"] == 15 / 29.97
    clip = RT.Clip(None, np.zeros((2, 4, 4, 3), np.uint8), 29.97)
    assert clip.fps == 29 and clip.fps_exact == 29.97


def test_handler_never_raises(tmp_path, capsys):
    case = FIXTURE["cases"]["heuristic_walk"]
    bus = RT.InProcessBus()
    svc = TLEAPPipeline(FakeDetector(case), bus, config=RT.load_config(str(tmp_path / "none.yaml")), results_dir=tmp_path / "tleap",
                        videos_dir=tmp_path / "videos", backend="host")
    asyncio.run(svc.process_video({"video_id": "absent", "processed_path": str(tmp_path / "absent.mp4")}))
    assert "Video not found: absent" in capsys.readouterr().out and bus.published == []
    bad = tmp_path / "broken.npz"
    bad.write_bytes(b"not a clip")
    asyncio.run(svc.process_video({"video_id": "broken", "processed_path": str(bad)}))
    assert "Error in T-LEAP pipeline for broken" in capsys.readouterr().out and bus.published == []


def test_handed_clips_and_file_clips_give_the_same_bytes(tmp_path, monkeypatch):
    """consumers handed (series, mask) write what the same consumers write from `{id}_tleap.json`; the bus sees tleap first"""
    import tcnref
    import xfmref
    from lmx import checkpoints, tcn, xfm
    from lmx.services import TCNPipeline, TransformerPipeline

    _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(tcnref.SHIPPED, 3), tcnref.SHIPPED.dropout)
    _, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(xfmref.WIDE, 3), n_heads=xfmref.WIDE.n_heads, dropout=xfmref.WIDE.dropout)
    scorers = (tcn.TcnScorer(tcnref.SHIPPED, folded, backend="host"), xfm.XfmScorer(xfmref.WIDE, w, backend="host"))

    def consumers(bus, tleap_dir, out):
        cfg = {"nats": {"subjects": {}}}
        return [TCNPipeline(scorers[0], bus, config=cfg, tleap_dir=tleap_dir, results_dir=out / "tcn"),
                TransformerPipeline(scorers[1], bus, config=cfg, tleap_dir=tleap_dir, results_dir=out / "transformer")]

    case = FIXTURE["cases"]["heuristic_mixed"]
    frames = np.broadcast_to(np.zeros((1, case["h"], case["w"], 3), np.uint8), (21, case["h"], case["w"], 3))
    monkeypatch.setattr(RT.Clip, "open", staticmethod(lambda path: RT.Clip(path, frames, case["fps"])))
    video = tmp_path / "cow_7.npz"
    video.write_bytes(b"stand-in")
    bus = RT.InProcessBus()
    svc = TLEAPPipeline(FakeDetector(case), bus, config=RT.load_config(str(tmp_path / "none.yaml")), results_dir=tmp_path / "tleap",
                        consumers=consumers(bus, tmp_path / "unused", tmp_path / "handed"), backend="host")
    asyncio.run(svc.process_video({"video_id": "cow_7", "processed_path": str(video)}))
    assert [s for s, _ in bus.published] == ["pipeline.tleap", "pipeline.tcn", "pipeline.transformer"]

    async def from_files():
        for c in consumers(RT.InProcessBus(), tmp_path / "tleap", tmp_path / "filed"):
            await c.process_video({"video_id": "cow_7"})

    asyncio.run(from_files())
    for sub, name in (("tcn", "cow_7_tcn.json"), ("transformer", "cow_7_transformer.json")):
        assert (tmp_path / "handed" / sub / name).read_bytes() == (tmp_path / "filed" / sub / name).read_bytes()
