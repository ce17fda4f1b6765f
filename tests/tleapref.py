"""The arithmetic of services/tleap-pipeline/app/main.py restated in plain Python floats, as the oracle of the tleap tests: the keypoints
estimated from a box (main.py:210-263), the blend of a trained model's keypoints with them (:156-195), the detector-only mode
(:267-306), the flattened pose_sequences (:479-486) and the locomotion features (:338-436, numpy as there).  Inputs are the detector's
arrays of one frame: boxes f32 [max_det, 4], scores f32 [max_det], cls i32 [max_det], count, kpts f32 [max_det, K, ndim] or None.
tests/golden/tleap_reference.json holds what the reference's own functions returned for the same inputs (tests/golden/record_tleap.py)."""
import numpy as np

KEYPOINT_NAMES = [
    "left_ear_base", "neck", "withers", "mid_back", "right_hind_hip", "right_hind_mid_leg", "right_hind_fetlock", "left_hind_shoulder",
    "left_hind_mid_leg", "left_hind_fetlock", "right_front_shoulder", "right_front_mid_leg", "right_front_lower_leg", "left_front_shoulder",
    "left_front_mid_leg", "left_front_lower_leg", "right_front_hoof", "left_front_hoof", "right_hind_hoof", "left_hind_hoof",
]
HEURISTIC_NAMES = [
    "left_eye", "right_eye", "nose", "left_ear", "right_ear", "left_front_elbow", "right_front_elbow", "left_back_elbow",
    "right_back_elbow", "left_front_knee", "right_front_knee", "left_back_knee", "right_back_knee", "left_front_paw", "right_front_paw",
    "left_back_paw", "right_back_paw", "throat", "withers", "tailbase",
]


def estimate_pose_from_bbox(bbox):
    x1, y1, x2, y2 = [int(c) for c in bbox]
    w, h = x2 - x1, y2 - y1
    head_x, head_y = x1 + w * 0.1, y1 + h * 0.3
    front_x, back_x = x1 + w * 0.25, x1 + w * 0.75
    ground_y = y2 - h * 0.05
    rows = [
        (head_x - w * 0.02, head_y - h * 0.05, 0.7), (head_x + w * 0.02, head_y - h * 0.05, 0.7), (head_x, head_y + h * 0.05, 0.8),
        (head_x - w * 0.05, head_y - h * 0.1, 0.6), (head_x + w * 0.05, head_y - h * 0.1, 0.6),
        (front_x - w * 0.05, y1 + h * 0.4, 0.7), (front_x + w * 0.05, y1 + h * 0.4, 0.7),
        (back_x - w * 0.05, y1 + h * 0.4, 0.7), (back_x + w * 0.05, y1 + h * 0.4, 0.7),
        (front_x - w * 0.03, y1 + h * 0.6, 0.7), (front_x + w * 0.07, y1 + h * 0.6, 0.7),
        (back_x - w * 0.07, y1 + h * 0.6, 0.7), (back_x + w * 0.03, y1 + h * 0.6, 0.7),
        (front_x - w * 0.02, ground_y, 0.7), (front_x + w * 0.08, ground_y, 0.7), (back_x - w * 0.08, ground_y, 0.7), (back_x + w * 0.02, ground_y, 0.7),
        (x1 + w * 0.15, y1 + h * 0.25, 0.8), (x1 + w * 0.3, y1 + h * 0.15, 0.8), (x1 + w * 0.9, y1 + h * 0.25, 0.7),
    ]
    return [{"name": n, "x": x, "y": y, "confidence": c} for n, (x, y, c) in zip(HEURISTIC_NAMES, rows)]


def detect_with_trained_model(boxes, scores, count, kpts):
    """One frame's detections; the keypoint list has min(K, 20) entries."""
    out = []
    for j in range(int(count)):
        bbox = [float(v) for v in boxes[j]]
        model = {}
        for i, kp in enumerate(kpts[j]):
            name = KEYPOINT_NAMES[i] if i < len(KEYPOINT_NAMES) else f"kp_{i}"
            model[name] = {"name": name, "x": float(kp[0]), "y": float(kp[1]), "confidence": float(kp[2]) if len(kp) > 2 else 1.0}
        heuristic = {kp["name"]: kp for kp in estimate_pose_from_bbox(bbox)}
        final = []
        for name in KEYPOINT_NAMES:
            if name in model and model[name]["confidence"] > 0.3:
                final.append(model[name])
            elif name in heuristic:
                final.append(heuristic[name])
            elif name in model:
                final.append(model[name])
        out.append({"bbox": bbox, "confidence": float(scores[j]), "class": "cow", "keypoints": final})
    return out


def detect_with_heuristic(boxes, scores, cls, count, names, h, w):
    """names: {class id: class name}"""
    out = []
    for j in range(int(count)):
        c = int(cls[j])
        class_name = names[c]
        if c == 19 or "cow" in class_name.lower():
            bbox = [float(v) for v in boxes[j]]
            out.append({"bbox": bbox, "confidence": float(scores[j]), "class": class_name, "keypoints": estimate_pose_from_bbox(bbox)})
    if not out and h > 0 and w > 0:
        margin = 0.1
        bbox = [w * margin, h * margin, w * (1 - margin), h * (1 - margin)]
        out.append({"bbox": bbox, "confidence": 0.5, "class": "cow_assumed", "keypoints": estimate_pose_from_bbox(bbox)})
    return out


def cow_classes(names):
    """The ids detect_with_heuristic accepts, as the service hands them to the kernel."""
    return sorted({19} | {i for i, n in names.items() if "cow" in str(n).lower()})


def pose_sequences(per_frame, frame_ids, fps):
    """main.py:479-486: one row per detection, flattened over the sampled frames."""
    seq = []
    for fid, dets in zip(frame_ids, per_frame):
        for det in dets:
            seq.append({"frame": fid, "time": fid / fps if fps > 0 else 0, "bbox": det["bbox"], "keypoints": det["keypoints"],
                        "detection_confidence": det["confidence"]})
    return seq


def locomotion(seq):
    if not seq or len(seq) < 2:
        return {}
    f, head, angles = {}, [], []
    hoofs = {"fl": [], "fr": [], "rl": [], "rr": []}
    for row in seq:
        kps = row.get("keypoints", [])
        if len(kps) < 20:
            continue
        d = {kp["name"]: kp for kp in kps}
        nose = d.get("nose", {})
        if nose.get("confidence", 0) > 0.3:
            head.append(nose.get("y", 0))
        t, w, b = d.get("throat", {}), d.get("withers", {}), d.get("tailbase", {})
        if all(k.get("confidence", 0) > 0.3 for k in (t, w, b)):
            v1 = np.array([t["x"] - w["x"], t["y"] - w["y"]])
            v2 = np.array([b["x"] - w["x"], b["y"] - w["y"]])
            cos = np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2) + 1e-6)
            angles.append(np.degrees(np.arccos(np.clip(cos, -1, 1))))
        for leg, name in (("fl", "left_front_paw"), ("fr", "right_front_paw"), ("rl", "left_back_paw"), ("rr", "right_back_paw")):
            kp = d.get(name, {})
            if kp.get("confidence", 0) > 0.3:
                hoofs[leg].append(kp.get("x", 0))
    if angles:
        f["back_arch_mean"] = float(np.mean(angles))
        f["back_arch_std"] = float(np.std(angles))
        f["back_arch_score"] = float(1.0 - (np.mean(angles) / 180.0))
    if len(head) > 1:
        f["head_bob_magnitude"] = float(np.std(head))
        f["head_bob_frequency"] = float(np.sum(np.abs(np.diff(np.sign(np.diff(head))))) / 2)
        f["head_bob_score"] = float(min(1.0, f["head_bob_magnitude"] / 50.0))
    for leg, xs in hoofs.items():
        if len(xs) > 1:
            strides = np.diff(xs)
            f[f"stride_{leg}_mean"] = float(np.mean(np.abs(strides)))
            f[f"stride_{leg}_std"] = float(np.std(strides))
    for key, a, b in (("front_leg_asymmetry", "stride_fl_mean", "stride_fr_mean"), ("rear_leg_asymmetry", "stride_rl_mean", "stride_rr_mean")):
        if a in f and b in f:
            f[key] = float(abs(f[a] - f[b]) / (f[a] + f[b] + 1e-6))
    parts = [f[k] for k in ("back_arch_score", "head_bob_score", "front_leg_asymmetry", "rear_leg_asymmetry") if k in f]
    if parts:
        f["lameness_score"] = float(np.mean(parts))
    return f


# ---- the fixture's cases as the detector's arrays -------------------------------------------------------------------------------------
def case_arrays(case):
    """A fixture case -> (boxes f32 [F, max_det, 4], scores f32 [F, max_det], cls i32 [F, max_det], counts i32 [F], kpts or None):
    max_det is the case's largest count (at least 1), unused slots are 0."""
    frames = case["frames"]
    md = max(1, max(len(fr["boxes"]) for fr in frames))
    F = len(frames)
    boxes, scores = np.zeros((F, md, 4), np.float32), np.zeros((F, md), np.float32)
    cls, counts = np.zeros((F, md), np.int32), np.zeros((F,), np.int32)
    kpts = np.zeros((F, md, case["K"], case["ndim"]), np.float32) if case.get("K") else None
    for i, fr in enumerate(frames):
        k = len(fr["boxes"])
        counts[i] = k
        if k:
            boxes[i, :k], scores[i, :k], cls[i, :k] = fr["boxes"], fr["scores"], fr["cls"]
            if kpts is not None:
                kpts[i, :k] = fr["kpts"]
    return boxes, scores, cls, counts, kpts


def case_detections(case):
    """This module's restatement over a fixture case: per frame, the detections."""
    boxes, scores, cls, counts, kpts = case_arrays(case)
    names = {int(k): v for k, v in case.get("names", {}).items()}
    out = []
    for i in range(len(counts)):
        if kpts is not None:
            out.append(detect_with_trained_model(boxes[i], scores[i], counts[i], kpts[i]))
        else:
            out.append(detect_with_heuristic(boxes[i], scores[i], cls[i], counts[i], names, case["h"], case["w"]))
    return out


def records_as_detections(rec, trained, names=None):
    """A clip's records (numpy, lmx.kernels.tleap_record_dtype) -> per row (frame, {"bbox", "confidence", "keypoints"}) with the slot
    names of the mode, to compare with the fixture."""
    names = names or (KEYPOINT_NAMES if trained else HEURISTIC_NAMES)
    out = []
    for r in rec:
        kps = []
        for i in range(int(r["n_kp"])):
            name = "withers" if trained and i == 2 else names[i]
            kps.append({"name": name, "x": float(r["keypoints"][i][0]), "y": float(r["keypoints"][i][1]), "confidence": float(r["keypoints"][i][2])})
        out.append((int(r["frame"]), {"bbox": [float(v) for v in r["bbox"]], "confidence": float(r["confidence"]), "keypoints": kps}))
    return out
