"""The host half of clip-curation behind the per-frame records (lmx/services/curation.py; reference services/clip-curation/app/main.py
:175-565) on authored tracks whose expectations are derived by hand in the comments: walking passes and their quirks, window scores,
the best window's tie rule, the canonical clip's frame sampling, the report, and the selection following the per-frame visual table."""
import numpy as np
import pytest

from lmx.services import curation as C

INFO = {"fps": 10.0, "width": 1000, "height": 500, "total_frames": 0, "duration": 0.0}  # window_frames = 50, step 12


def det(frame, cx, cy=250.0, bw=300.0, bh=250.0, conf=0.8):
    if cx is None:
        return {"frame": frame, "time": frame / 10.0, "detection": None}
    return {"frame": frame, "time": frame / 10.0,
            "detection": {"bbox": [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], "confidence": conf, "centroid": (cx, cy), "area": bw * bh}}


def track(xs, first=0):
    """records for consecutive frames; None = no detection"""
    return [det(first + i, x) for i, x in enumerate(xs)]


def test_left_to_right_gap_right_to_left():
    """frames 0..39 walk right by 10; frame 40 has no detection: pass 1 ends at 39.  Frames 41..80 walk left by 15 from 900.  The
    direction SURVIVES the gap, so the second stretch starts as left_to_right; its sixth detection (frame 46, x = 825) is compared with
    the first of the last five (frame 42, x = 885): -60, opposite and above 5 % of 1000 — the five detections so far are dropped as too
    short and frame 46 opens the right_to_left pass, which runs to the last record (35 detections)."""
    xs = [100.0 + 10 * i for i in range(40)] + [None] + [900.0 - 15 * i for i in range(40)]
    passes = C.identify_walking_passes(track(xs), INFO)
    assert [(p.start_frame, p.end_frame, p.direction, len(p.centroids)) for p in passes] == [(0, 39, "left_to_right", 40), (46, 80, "right_to_left", 35)]
    assert passes[0].normalized_progress[0] == 0.0 and passes[0].normalized_progress[-1] == 1.0
    assert passes[0].normalized_progress[10] == (200.0 - 100.0) / 390.0
    assert passes[1].centroids[0] == (825.0, 250.0)
    assert passes[1].normalized_progress[0] == 0.0 and passes[1].normalized_progress[-1] == 1.0  # progress runs along the walk
    assert passes[1].bboxes[0] == [675.0, 125.0, 975.0, 375.0] and passes[1].confidences == [0.8] * 35


def test_a_slow_reversal_after_a_gap_keeps_the_old_direction():
    """the same, walking left by 10: |dx| against the first of the last five is 40, never above 50, so no split: one pass from frame 41,
    still called left_to_right, progress computed for that direction (it FALLS from 1 to 0)"""
    xs = [100.0 + 10 * i for i in range(40)] + [None] + [900.0 - 10 * i for i in range(40)]
    passes = C.identify_walking_passes(track(xs), INFO)
    assert [(p.start_frame, p.end_frame, p.direction, len(p.centroids)) for p in passes] == [(0, 39, "left_to_right", 40), (41, 80, "left_to_right", 40)]
    assert passes[1].normalized_progress[0] == 1.0 and passes[1].normalized_progress[-1] == 0.0


@pytest.mark.parametrize("count,kept", [(29, 0), (30, 1)])
def test_passes_shorter_than_30_detections_are_dropped(count, kept):
    xs = [100.0 + 10 * i for i in range(count)] + [None] * 3
    passes = C.identify_walking_passes(track(xs), INFO)
    assert len(passes) == kept
    if kept:
        assert (passes[0].start_frame, passes[0].end_frame) == (0, 29)  # the gap's frame - 1, not the last record's
    # the same stretch as the clip's end: the last pass ends at the last record
    passes = C.identify_walking_passes(track(xs[:count]), INFO)
    assert len(passes) == kept and (not kept or passes[0].end_frame == 29)


def test_reversal_above_the_threshold_splits_and_below_it_does_not():
    """frames 0..34: x = 100 + 10 f (up to 440); then back by 12 per frame.  Against the first of the last five centroids: frame 35 (428 vs
    x30 = 400) +28, frame 36 (416 vs 410) +6, frame 37 (404 vs 420) -16, frame 38 (392 vs 430) -38: opposite but within 50, appended;
    frame 39 (380 vs 440) -60: split.  Pass 1 = frames 0..38, pass 2 = frames 39..74 right_to_left (36 detections).
    Back by 2 per frame instead: the movement never passes -10, one pass."""
    up = [100.0 + 10 * f for f in range(35)]
    passes = C.identify_walking_passes(track(up + [440.0 - 12 * k for k in range(1, 41)]), INFO)
    assert [(p.start_frame, p.end_frame, p.direction, len(p.centroids)) for p in passes] == [(0, 38, "left_to_right", 39), (39, 74, "right_to_left", 36)]
    passes = C.identify_walking_passes(track(up + [440.0 - 2 * k for k in range(1, 41)]), INFO)
    assert [(p.start_frame, p.end_frame, p.direction, len(p.centroids)) for p in passes] == [(0, 74, "left_to_right", 75)]


def test_no_direction_defaults_and_nothing_detected():
    assert C.identify_walking_passes([], INFO) == []
    assert C.identify_walking_passes(track([None] * 40), INFO) == []
    # a standing cow: dx = 0 is "not > 0", so the direction is right_to_left — the left_to_right default only serves a pass that never
    # reached its sixth detection, which the 30-detection rule drops anyway
    passes = C.identify_walking_passes(track([500.0] * 40), INFO)
    assert [(p.direction, p.normalized_progress[3]) for p in passes] == [("right_to_left", 0.0)]


def steady_pass(first=0, count=50, x0=255.0, step=10.0):
    """box 300 x 250 at y = 250 in a 1000 x 500 frame, moving right by `step`: margins stay above 5 % for x in 255 .. 745"""
    return C.identify_walking_passes(track([x0 + step * i for i in range(count)], first), INFO)[0]


def test_score_of_a_steady_centred_window():
    """size: 75 000 / 500 000 = 0.15 -> 0.15 / 0.3 = 0.5; margins at least 0.105 -> edge 1: framing 0.5 * 0.6 + 0.4 = 0.7.  Constant
    velocity: steadiness 1; constant y: straightness 1; confidence 0.8; progress runs 0 .. 1, mean 0.5, inside the band: 1.
    overall = 0.7 / 4 + 1 / 4 + 0.15 + 0.15 v + 0.08 + 0.1 = 0.755 + 0.15 v with v the mean of the table at frames 0, 10, 20, 30, 40"""
    p = steady_pass()
    visual = np.linspace(0.0, 0.49, 50)  # table[f] = f / 100
    m = C.score_window(p, 0, 50, INFO, visual)
    assert m.framing_score == pytest.approx(0.7, abs=1e-12) and m.steadiness_score == pytest.approx(1.0, abs=1e-12)
    assert m.straightness_score == 1.0 and m.occlusion_score == pytest.approx(0.8, abs=1e-12)
    assert m.visual_quality_score == pytest.approx(0.2, abs=1e-12)
    assert m.overall_score == pytest.approx(0.755 + 0.15 * 0.2, abs=1e-12)
    assert all(isinstance(v, float) for v in m.to_dict().values())
    assert list(m.to_dict()) == ["framing_score", "steadiness_score", "straightness_score", "visual_quality_score", "occlusion_score", "overall_score"]


def test_edges_wobble_and_progress_band():
    """a box that touches the left edge (margin 0) scores edge 0 on that frame; a y range of 5 % of the height costs half the straightness;
    a window at the start of a long pass is scaled by progress / 0.25"""
    p = steady_pass(x0=150.0, step=10.0)  # x1 = 0 on frame 0, then 10, 20, 30, 40: edge = 0, .2, .4, .6, .8 (sum 2), then 45 times 1 -> mean 47 / 50
    m = C.score_window(p, 0, 50, INFO, np.ones(50))
    assert m.framing_score == pytest.approx(0.5 * 0.6 + (47 / 50) * 0.4, abs=1e-12)
    recs = track([255.0 + 10 * i for i in range(50)])
    recs[7]["detection"]["centroid"] = (325.0, 275.0)  # 25 px of 500: 1 - 0.05 * 10 = 0.5
    m = C.score_window(C.identify_walking_passes(recs, INFO)[0], 0, 50, INFO, np.ones(50))
    assert m.straightness_score == pytest.approx(0.5, abs=1e-12)
    long = steady_pass(count=200, x0=255.0, step=2.0)  # progress of detection i = i / 199
    m = C.score_window(long, 0, 50, INFO, np.ones(200))
    band = (24.5 / 199) / 0.25
    assert m.overall_score == pytest.approx(0.7 * 0.25 + 0.25 + 0.15 + 0.15 + 0.08 + 0.1 * band, abs=1e-12)
    m = C.score_window(long, 150, 50, INFO, np.ones(200))  # mean progress 174.5 / 199 = 0.877 > 0.85
    band = (1 - 174.5 / 199) / 0.15
    assert m.overall_score == pytest.approx(0.7 * 0.25 + 0.25 + 0.15 + 0.15 + 0.08 + 0.1 * band, abs=1e-12)


def test_window_shorter_than_four_fifths_scores_zero():
    p = steady_pass(count=100, step=4.0)
    assert C.score_window(p, 61, 50, INFO, np.ones(100)) == C.QualityMetrics(0, 0, 0, 0, 0, 0)  # 39 detections < 40
    m = C.score_window(p, 60, 50, INFO, np.ones(100))  # exactly 40: scored, sampled at 60, 68, .. 92
    assert m.overall_score > 0 and m.visual_quality_score == 1.0
    table = np.zeros(100)
    table[[60, 68, 76, 84, 92]] = 1.0
    assert C.score_window(p, 60, 50, INFO, table).visual_quality_score == 1.0


def test_samples_beyond_the_table_are_failed_reads():
    """the pass starts at frame 100: samples 100, 110, 120, 130, 140.  A table of 10 frames holds none: 0.5.  A table of 125 holds the
    first three; a window of 52 detections yields six sample positions, of which five are used"""
    p = steady_pass(first=100, count=52, step=9.0)
    assert C.score_window(p, 0, 50, INFO, np.ones(10)).visual_quality_score == 0.5
    assert C.score_window(p, 0, 50, INFO, np.zeros(0)).visual_quality_score == 0.5
    table = np.zeros(125)
    table[[100, 110, 120]] = (0.3, 0.6, 0.9)
    assert C.score_window(p, 0, 50, INFO, table).visual_quality_score == pytest.approx(0.6, abs=1e-12)
    table = np.zeros(160)
    table[[100, 110, 120, 130, 140, 150]] = (1, 1, 1, 1, 1, 100)
    assert C.score_window(p, 0, 52, INFO, table).visual_quality_score == 1.0


def test_best_window_needs_a_strictly_greater_score():
    """a standing cow: steadiness 0 and progress 0 for every window, so all windows of the pass tie and the FIRST is kept; a table that
    favours a later window moves the choice there.  window_frames = int(5.0 * 10) = 50, step 12: starts 0, 12, 24, 36, 48"""
    p = C.identify_walking_passes(track([500.0] * 100), INFO)[0]
    c = C.find_best_window(p, INFO, np.ones(100))
    assert (c.start_frame, c.end_frame, c.start_time, c.end_time, c.needs_flip) == (0, 50, 0.0, 5.0, True)
    table = np.zeros(100)
    table[[36, 46, 56, 66, 76]] = 1.0
    c = C.find_best_window(p, INFO, table)
    assert (c.start_frame, c.end_frame) == (36, 86) and c.metrics.visual_quality_score == 1.0
    assert C.find_best_window(steady_pass(count=49), INFO, np.ones(49)) is None  # shorter than one window
    info = dict(INFO, fps=29.97)
    assert C.find_best_window(steady_pass(count=149, step=3.0), info, np.ones(149)).end_frame == 149  # int(5.0 * 29.97) = 149


def test_canonical_frame_indices():
    assert C.canonical_frame_indices(40, 1000, 25.0) == list(range(40, 165))
    assert C.canonical_frame_indices(40, 1000, 50.0) == list(range(40, 290, 2))
    got = C.canonical_frame_indices(0, 1000, 30.0)  # frame k when k >= 1.2 * written: 0, 2 (>= 1.2), 3 (>= 2.4), 4 (>= 3.6), 5 (>= 4.8), 6, 8, ..
    assert got[:11] == [0, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12] and len(got) == 125 and got[-1] == 149
    assert C.canonical_frame_indices(100, 110, 25.0) == list(range(100, 110))  # the clip ends: 10 frames
    assert C.canonical_frame_indices(100, 110, 50.0) == [100, 102, 104, 106, 108]
    assert C.canonical_frame_indices(100, 100, 25.0) == []
    assert C.canonical_frame_indices(7, 1000, 12.5)[:4] == [7, 8, 9, 10] and len(C.canonical_frame_indices(7, 1000, 12.5)) == 125


def two_equal_passes():
    """frames 0..49 and 51..100 hold the same walk; frame 50 has no detection.  One window each, equal but for the frames they sample"""
    xs = [255.0 + 10 * i for i in range(50)]
    info = dict(INFO, total_frames=101, duration=10.1)
    return C.identify_walking_passes(track(xs + [None] + xs), info), info


def test_selection_follows_the_visual_table():
    passes, info = two_equal_passes()
    assert [(p.start_frame, p.end_frame, p.direction) for p in passes] == [(0, 49, "left_to_right"), (51, 100, "left_to_right")]
    sharp_first = np.where(np.arange(101) <= 50, 0.9, 0.3)
    selected, backup = C.select_windows(passes, info, sharp_first)
    assert (selected.start_frame, backup.start_frame) == (0, 51)
    assert selected.metrics.overall_score == pytest.approx(0.755 + 0.15 * 0.9, abs=1e-12)
    assert backup.metrics.overall_score == pytest.approx(0.755 + 0.15 * 0.3, abs=1e-12)
    selected, backup = C.select_windows(passes, info, sharp_first[::-1].copy())
    assert (selected.start_frame, backup.start_frame) == (51, 0)
    selected, backup = C.select_windows(passes, info, np.full(101, 0.5))  # a tie keeps the order of the passes
    assert (selected.start_frame, backup.start_frame) == (0, 51)
    assert C.select_windows([], info, sharp_first) == (None, None)
    assert C.select_windows(passes[:1], info, sharp_first)[1] is None


def test_quality_report_keys_and_values():
    passes, info = two_equal_passes()
    selected, backup = C.select_windows(passes, info, np.where(np.arange(101) <= 50, 0.9, 0.3))
    rep = C.generate_quality_report("vid7", info, passes, selected, backup)
    assert list(rep) == ["video_id", "source_video", "canonical_clip", "walking_passes_detected", "passes", "selected_window", "backup_window", "status",
                         "rejection_reason"]
    assert rep["video_id"] == "vid7" and rep["status"] == "success" and rep["rejection_reason"] is None
    assert rep["source_video"] == {"fps": 10.0, "width": 1000, "height": 500, "total_frames": 101, "duration": 10.1}
    assert rep["canonical_clip"] == {"target_fps": 25, "target_resolution": [1280, 720], "target_duration": 5.0}
    assert rep["walking_passes_detected"] == 2
    assert rep["passes"] == [{"start_frame": 0, "end_frame": 49, "direction": "left_to_right", "duration": 4.9},
                             {"start_frame": 51, "end_frame": 100, "direction": "left_to_right", "duration": 4.9}]
    assert rep["selected_window"] == {"start_frame": 0, "end_frame": 50, "start_time": 0.0, "end_time": 5.0, "needs_flip": False,
                                      "metrics": selected.metrics.to_dict()}
    assert rep["backup_window"]["start_frame"] == 51 and rep["backup_window"]["end_time"] == 10.1 and rep["backup_window"]["metrics"] == backup.metrics.to_dict()
    failed = C.generate_quality_report("vid8", info, [], None, None)
    assert list(failed) == list(rep) and failed["status"] == "failed" and failed["selected_window"] is None and failed["backup_window"] is None
    assert failed["rejection_reason"] == "No valid walking pass found with sufficient quality" and failed["passes"] == []
