"""clip-curation's per-frame YOLO consumer on liblmx: `detect_cow_in_frame`
(services/clip-curation/app/main.py:103-131) and the per-frame records of `track_cow_through_video` (:154-165), batched
over the frames of a clip.  The detector runs on every frame of 30 s uploads — the densest YOLO consumer of the product —
so the frames go through YoloDetector.detect in batches and only the [n, max_det] box / score / class tables (7 kB per frame)
come back to the host, where the reference's selection rule is applied unchanged.

Behind the records, the rest of the service (`ClipCurator`): walking passes (:175-274), the sliding 5 s window scores (:291-395), the
best window of a pass (:397-432), the frames of the canonical 125-frame clip (:434-483) and the quality report (:507-565).  The one piece
of per-pixel arithmetic in there that is no network — cv2.cvtColor(BGR2GRAY), cv2.Laplacian(gray, CV_64F).var() and np.mean(gray) on
five decoded frames per candidate window (:276-289, :350-365) — is ONE pass over every frame where CowTracker.track already has them,
in HBM (lmx.kernels.frame_quality -> four integer sums per frame); `score_window` is host arithmetic on that table and no frame is
decoded or touched twice.  The canonical clip's cv2.resize(frame, (1280, 720)) is lmx.kernels.letterbox without padding and without the
channel swap.  Writing mp4 files, the ffmpeg re-encode, NATS and the report file stay with the caller: `canonical_frames` is what it
would encode."""
from dataclasses import asdict, dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

TARGET_FPS = 25
TARGET_RESOLUTION = (1280, 720)  # width, height
CANONICAL_DURATION = 5.0  # seconds
MIN_PASS_FRAMES = 30  # detections of a valid walking pass
PROGRESS_BAND = (0.25, 0.85)

COCO_COW = 19  # "Class 19 is cow in COCO" (main.py:114)


def best_detection(boxes, scores, cls, count, frame_h, frame_w):
    """main.py:106-131 on one frame's NMS output: the largest box that is a cow or covers more than 10 % of the frame."""
    best, best_area = None, 0
    frame_area = frame_h * frame_w
    for j in range(int(count)):
        x1, y1, x2, y2 = (np.float32(v) for v in boxes[j])
        area = (x2 - x1) * (y2 - y1)
        if (int(cls[j]) == COCO_COW or area > frame_area * 0.1) and area > best_area:
            best_area = area
            best = {"bbox": [float(x1), float(y1), float(x2), float(y2)], "confidence": float(scores[j]),
                    "centroid": ((x1 + x2) / 2, (y1 + y2) / 2), "area": area}
    return best


class CowTracker:
    def __init__(self, detector, conf=0.3, batch=64):
        self.detector, self.conf, self.batch = detector, conf, batch

    def track(self, frames, fps, first_frame=0):
        """frames: u8 BGR [n,h,w,3] on the detector's device -> the `detections` list of track_cow_through_video:
        [{"frame", "time", "detection": best_detection | None}] (main.py:154-165)."""
        n, h, w, _ = frames.shape
        out = []
        for i in range(0, n, self.batch):
            boxes, scores, cls, _, counts = (t.cpu().numpy() for t in self.detector.detect(frames[i:i + self.batch], conf=self.conf))
            for b in range(boxes.shape[0]):
                idx = first_frame + i + b
                out.append({"frame": idx, "time": idx / fps if fps > 0 else 0,
                            "detection": best_detection(boxes[b], scores[b], cls[b], counts[b], h, w)})
        return out


# ---- behind the records: passes, windows, the canonical clip, the report ------------------------------------------------------------
@dataclass
class QualityMetrics:
    framing_score: float
    steadiness_score: float
    straightness_score: float
    visual_quality_score: float
    occlusion_score: float
    overall_score: float

    def to_dict(self) -> Dict[str, float]:
        return asdict(self)


@dataclass
class WalkingPass:
    start_frame: int
    end_frame: int
    direction: str  # "left_to_right" | "right_to_left"
    centroids: List[Tuple[float, float]]
    bboxes: List[List[float]]
    confidences: List[float]
    normalized_progress: List[float]


@dataclass
class ClipCandidate:
    start_frame: int
    end_frame: int
    start_time: float
    end_time: float
    metrics: QualityMetrics
    needs_flip: bool


def visual_scores(stats):
    """int64 [n,4] rows (Σ g, Σ lap, Σ lap², N) of lmx.kernels.frame_quality -> (blur, brightness), float64 [n] each: main.py:276-289.
    brightness = max(0, 1 - |Σ g / N - 128| / 128): bit-equal to the reference's np.mean on the u8 gray image (an integer sum below 2^53
    is exact in float64, then one division).  blur = min(1, var / 500) with the population variance var = (N Σ lap² - (Σ lap)²) / N² from
    Python integers and one true division, i.e. correctly rounded (N Σ lap² passes 2^63 above some 8.8 M pixels; numpy's two-pass float
    .var() of the reference is matched to a tolerance, not bit for bit)."""
    rows = np.asarray(stats).reshape(-1, 4).tolist()
    blur, bright = np.empty(len(rows), np.float64), np.empty(len(rows), np.float64)
    for i, (s0, s1, s2, cnt) in enumerate(rows):
        s0, s1, s2, cnt = int(s0), int(s1), int(s2), int(cnt)
        var = (cnt * s2 - s1 * s1) / (cnt * cnt)
        blur[i] = min(1.0, var / 500.0)
        bright[i] = max(0.0, 1.0 - abs(s0 / cnt - 128) / 128)
    return blur, bright


def _walking_pass(start_frame, end_frame, direction, centroids, bboxes, confidences):
    """main.py:251-274: progress 0 .. 1 along x in the direction of the walk (a pass without x extent divides by 1)"""
    xs = [c[0] for c in centroids]
    lo, hi = min(xs), max(xs)
    span = hi - lo if hi > lo else 1
    progress = [(x - lo) / span for x in xs] if direction == "left_to_right" else [(hi - x) / span for x in xs]
    return WalkingPass(start_frame, end_frame, direction, centroids, bboxes, confidences, progress)


def identify_walking_passes(detections, video_info):
    """main.py:175-249 on CowTracker.track's records, quirks included: a frame without a detection ends the pass at frame - 1 and
    forgets everything but the direction; from the sixth detection of a pass on, the x movement against the FIRST of the last five
    centroids (taken before the new one is appended) sets the direction once and later splits the pass where it is opposite and larger
    than 5 % of the width — the splitting detection opens the next pass; passes with fewer than MIN_PASS_FRAMES detections are
    dropped; the last pass ends at the last record's frame and is left_to_right if no direction was ever set."""
    passes = []
    start, direction = None, None
    cents, boxes, confs = [], [], []
    width = video_info["width"]

    def close(end_frame, dflt=None):
        if start is not None and len(cents) >= MIN_PASS_FRAMES:
            passes.append(_walking_pass(start, end_frame, direction or dflt, cents, boxes, confs))

    for det in detections:
        d = det["detection"]
        if d is None:
            close(det["frame"] - 1)
            start, cents, boxes, confs = None, [], [], []
            continue
        if start is None:
            start, cents, boxes, confs = det["frame"], [d["centroid"]], [d["bbox"]], [d["confidence"]]
            continue
        if len(cents) >= 5:
            dx = d["centroid"][0] - cents[-5][0]
            seen = "left_to_right" if dx > 0 else "right_to_left"
            if direction is None:
                direction = seen
            elif seen != direction and abs(dx) > width * 0.05:
                close(det["frame"] - 1)
                start, direction = det["frame"], seen
                cents, boxes, confs = [d["centroid"]], [d["bbox"]], [d["confidence"]]
                continue
        cents.append(d["centroid"])
        boxes.append(d["bbox"])
        confs.append(d["confidence"])
    if detections:
        close(detections[-1]["frame"], "left_to_right")
    return passes


def score_window(walking_pass, start_idx, window_frames, video_info, visual):
    """main.py:291-395.  `visual`: the per-frame (blur + brightness) / 2 table indexed by absolute frame number, in place of the
    reference's seek, decode and score of up to five sampled frames; a sample outside the table is a failed cap.read() — skipped, and
    no sample at all gives 0.5."""
    end_idx = min(start_idx + window_frames, len(walking_pass.centroids))
    length = end_idx - start_idx
    if length < window_frames * 0.8:
        return QualityMetrics(0, 0, 0, 0, 0, 0)
    cents = walking_pass.centroids[start_idx:end_idx]
    boxes = walking_pass.bboxes[start_idx:end_idx]
    fw, fh = video_info["width"], video_info["height"]

    # framing: box size (best at 30 % of the frame) and distance from the edges (penalised below 5 %)
    rel = np.mean([(b[2] - b[0]) * (b[3] - b[1]) for b in boxes]) / (fw * fh)
    size_score = min(1.0, rel / 0.3)
    edge = [min(1.0, min(b[0] / fw, (fw - b[2]) / fw, b[1] / fh, (fh - b[3]) / fh) / 0.05) for b in boxes]
    framing = size_score * 0.6 + np.mean(edge) * 0.4

    # steadiness: coefficient of variation of the x velocity
    vx = np.diff([c[0] for c in cents])
    speed_mean, speed_std = np.abs(np.mean(vx)), np.std(vx)
    steadiness = max(0, 1.0 - speed_std / speed_mean) if speed_mean > 0 else 0.0

    # straightness: y range against the frame height
    ys = [c[1] for c in cents]
    straightness = max(0, 1.0 - ((max(ys) - min(ys)) / fh) * 10)

    # visual quality: up to five frames of the window
    first = walking_pass.start_frame + start_idx
    samples = [first + i for i in range(0, length, max(1, length // 5))][:5]
    seen = [float(visual[f]) for f in samples if 0 <= f < len(visual)]
    visual_quality = np.mean(seen) if seen else 0.5

    occlusion = np.mean(walking_pass.confidences[start_idx:end_idx])

    progress = np.mean(walking_pass.normalized_progress[start_idx:end_idx])
    band = 1.0
    if progress < PROGRESS_BAND[0]:
        band = progress / PROGRESS_BAND[0]
    elif progress > PROGRESS_BAND[1]:
        band = (1.0 - progress) / (1.0 - PROGRESS_BAND[1])

    overall = framing * 0.25 + steadiness * 0.25 + straightness * 0.15 + visual_quality * 0.15 + occlusion * 0.1 + band * 0.1
    return QualityMetrics(float(framing), float(steadiness), float(straightness), float(visual_quality), float(occlusion), float(overall))


def find_best_window(walking_pass, video_info, visual):
    """main.py:397-432: 5 s windows sliding by a quarter of their length; the first window of the highest score wins (a later one needs
    a strictly greater score, starting from -1); None for a pass shorter than one window."""
    fps = video_info["fps"]
    window_frames = int(CANONICAL_DURATION * fps)
    if len(walking_pass.centroids) < window_frames:
        return None
    best, best_score = None, -1
    for start_idx in range(0, len(walking_pass.centroids) - window_frames + 1, max(1, window_frames // 4)):
        metrics = score_window(walking_pass, start_idx, window_frames, video_info, visual)
        if metrics.overall_score > best_score:
            best_score = metrics.overall_score
            first = walking_pass.start_frame + start_idx
            best = ClipCandidate(first, first + window_frames, first / fps, (first + window_frames) / fps, metrics,
                                 walking_pass.direction == "right_to_left")
    return best


def canonical_frame_indices(start_frame, n_frames, fps):
    """main.py:456-481: the source frames of the canonical clip — frame k behind start_frame is written when k >= written * (fps / 25),
    until int(5.0 * 25) frames are written or the clip of n_frames frames ends."""
    target, ratio = int(CANONICAL_DURATION * TARGET_FPS), fps / TARGET_FPS
    out, k = [], 0
    while len(out) < target and start_frame + k < n_frames:
        if k >= len(out) * ratio:
            out.append(start_frame + k)
        k += 1
    return out


def canonical_frames(frames, candidate, fps):
    """main.py:456-481 without the writer: frames u8 BGR [n,h,w,3] on the device -> u8 [m,720,1280,3] on the device, the frames
    canonical_frame_indices names, resized as cv2.resize(frame, (1280, 720)) does (INTER_LINEAR on 8U: lmx.kernels.letterbox with no
    padding and no channel swap; a 720 x 1280 source is copied) and mirrored along x where the pass walks right to left (cv2.flip(frame, 1));
    the gather and the mirror are plain copies."""
    import torch

    from .. import kernels as K
    from .. import letterbox as LB

    n, sh, sw, _ = frames.shape
    ow, oh = TARGET_RESOLUTION
    idx = canonical_frame_indices(candidate.start_frame, n, fps)
    if not idx:
        return torch.empty((0, oh, ow, 3), dtype=torch.uint8, device=frames.device)
    out = frames.index_select(0, torch.tensor(idx, dtype=torch.int64, device=frames.device))
    if (sh, sw) != (oh, ow):
        geo = LB.LetterboxGeo(sh, sw, oh, ow, 0, 0, oh, ow, min(oh / sh, ow / sw), 0.0, 0.0)
        tables = tuple(torch.from_numpy(t).to(frames.device) for t in LB.resize_tables(sh, sw, oh, ow))
        out = K.letterbox(out, geo, tables, swap_rb=False)
    return out.flip(2).contiguous() if candidate.needs_flip else out


def _window_record(c):
    return {"start_frame": c.start_frame, "end_frame": c.end_frame, "start_time": c.start_time, "end_time": c.end_time,
            "needs_flip": c.needs_flip, "metrics": c.metrics.to_dict()}


def generate_quality_report(video_id, video_info, passes, selected, backup):
    """main.py:507-565, key for key"""
    return {
        "video_id": video_id,
        "source_video": {k: video_info[k] for k in ("fps", "width", "height", "total_frames", "duration")},
        "canonical_clip": {"target_fps": TARGET_FPS, "target_resolution": list(TARGET_RESOLUTION), "target_duration": CANONICAL_DURATION},
        "walking_passes_detected": len(passes),
        "passes": [{"start_frame": p.start_frame, "end_frame": p.end_frame, "direction": p.direction,
                    "duration": (p.end_frame - p.start_frame) / video_info["fps"]} for p in passes],
        "selected_window": _window_record(selected) if selected else None,
        "backup_window": _window_record(backup) if backup else None,
        "status": "success" if selected else "failed",
        "rejection_reason": None if selected else "No valid walking pass found with sufficient quality",
    }


def select_windows(passes, video_info, visual):
    """main.py:601-613: the best window of every pass, then the two best of those by overall score -> (selected, backup)"""
    candidates = [c for c in (find_best_window(p, video_info, visual) for p in passes) if c]
    candidates.sort(key=lambda c: c.metrics.overall_score, reverse=True)
    return (candidates[0] if candidates else None), (candidates[1] if len(candidates) > 1 else None)


class ClipCurator:
    """curate_video of the reference (main.py:567-634) from frames in HBM to the chosen windows; the caller owns decode, encode and I/O."""

    def __init__(self, detector, conf=0.3, batch=64):
        self.tracker = CowTracker(detector, conf, batch)
        self.batch = batch

    def curate(self, video_id, frames, fps):
        """frames: u8 BGR [n,h,w,3] on the detector's device -> {"report": generate_quality_report's dict, "selected" / "backup":
        ClipCandidate | None (what canonical_frames takes), "visual": float64 [n], the per-frame (blur + brightness) / 2}."""
        import torch

        from .. import kernels as K

        n, h, w, _ = frames.shape
        video_info = {"fps": fps, "width": w, "height": h, "total_frames": n, "duration": n / fps if fps > 0 else 0}
        detections = self.tracker.track(frames, fps)
        stats = torch.empty((n, 4), dtype=torch.int64, device=frames.device)
        for i in range(0, n, self.batch):
            K.frame_quality(frames[i:i + self.batch], out=stats[i:i + self.batch])
        blur, bright = visual_scores(stats.cpu().numpy())  # the one host copy: 32 bytes per frame
        visual = (blur + bright) / 2
        passes = identify_walking_passes(detections, video_info)
        selected, backup = select_windows(passes, video_info, visual)
        return {"report": generate_quality_report(video_id, video_info, passes, selected, backup), "selected": selected, "backup": backup,
                "visual": visual}
