"""Records tests/golden/tleap_reference.json: what the reference's OWN tleap-pipeline functions return for a handful of inputs.

    python tests/golden/record_tleap.py PATH_TO_REFERENCE_CHECKOUT

services/tleap-pipeline/app/main.py is imported with stand-ins for cv2, yaml and shared in sys.modules (none is used by the functions
recorded); its CowPoseEstimator gets a fake `model` whose results are built from torch tensors, so `.cpu().numpy()` works as on the
real one.  Only data goes into the fixture: the inputs (float32 values written as Python floats, which repr round-trips) and the returned
dictionaries.  The tests read the fixture, never the reference."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 720, 1280


def load_reference(root):
    for name in ("cv2", "yaml", "shared", "shared.utils", "shared.utils.nats_client"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["shared.utils.nats_client"].NATSClient = object
    spec = importlib.util.spec_from_file_location("tleap_reference_main", os.path.join(root, "services", "tleap-pipeline", "app", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Box:
    def __init__(self, xyxy, conf, cls):
        self.xyxy, self.conf, self.cls = torch.tensor([xyxy], dtype=torch.float32), torch.tensor([conf], dtype=torch.float32), torch.tensor([float(cls)])


class Keypoints:
    def __init__(self, data):
        self.data = data  # [n, K, ndim]

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, j):
        return Keypoints(self.data[j:j + 1])


class Result:
    def __init__(self, frame, pose):
        self.boxes = [Box(b, s, c) for b, s, c in zip(frame["boxes"], frame["scores"], frame["cls"])]
        self.keypoints = Keypoints(torch.tensor(frame["kpts"], dtype=torch.float32)) if pose and frame["boxes"] else None


class Model:
    def __init__(self, names, pose):
        self.names, self.pose, self.frame = names, pose, None

    def __call__(self, image, verbose=False, conf=0.3):
        return [Result(self.frame, self.pose)]


def f32(a):
    return np.asarray(a, np.float32).tolist()  # Python floats that hold float32 values exactly


def trained_case(K, ndim, rng):
    below = float(np.nextafter(np.float32(0.3), np.float32(0)))
    frames = []
    for n_det, withers in ((3, (float(np.float32(0.3)), below, 0.0)), (0, ()), (1, (0.9,))):
        boxes = rng.uniform(0, 600, (n_det, 4)).astype(np.float32)
        boxes[:, 2:] += boxes[:, :2] + 5
        kpts = rng.uniform(0, 1200, (n_det, K, ndim)).astype(np.float32)
        if ndim == 3:
            kpts[:, :, 2] = rng.uniform(0, 1, (n_det, K)).astype(np.float32)
            kpts[:, 2, 2] = withers
        frames.append({"boxes": f32(boxes), "scores": f32(rng.uniform(0.3, 1, n_det)), "cls": [0] * n_det, "kpts": f32(kpts)})
    return {"mode": "trained", "K": K, "ndim": ndim, "h": H, "w": W, "fps": 25.0, "frame_ids": [0, 5, 10], "frames": frames}


def heuristic_cases(rng):
    def frame(classes):
        n = len(classes)
        boxes = rng.uniform(0, 600, (n, 4)).astype(np.float32)
        boxes[:, 2:] += boxes[:, :2] + 5
        return {"boxes": f32(boxes), "scores": f32(rng.uniform(0.3, 1, n)), "cls": list(classes)}

    names = {0: "person", 3: "Dairy Cow", 7: "truck", 19: "sheep"}
    mixed = {"mode": "heuristic", "h": H, "w": W, "fps": 25.0, "names": {str(k): v for k, v in names.items()}, "frame_ids": [0, 5, 10, 15, 20],
             "frames": [frame([19, 0, 19]), frame([3]), frame([0, 7]), frame([]), frame([7, 3, 19])]}
    walk_frames = []
    for i in range(12):  # one cow walking left to right, its box breathing: the clip the locomotion features are recorded on
        x, y = 100 + 37.3 * i + rng.uniform(-6, 6), 200 + 9 * np.sin(1.1 * i) + rng.uniform(-3, 3)
        bw, bh = 420 + rng.uniform(-25, 25), 260 + rng.uniform(-20, 20)
        walk_frames.append({"boxes": f32([[x, y, x + bw, y + bh]]), "scores": f32([rng.uniform(0.5, 0.95)]), "cls": [19]})
    walk = {"mode": "heuristic", "h": H, "w": W, "fps": 29.97, "names": {"19": "cow"}, "frame_ids": [5 * i for i in range(12)], "frames": walk_frames}
    return {"heuristic_mixed": mixed, "heuristic_walk": walk}


def main(root):
    ref = load_reference(root)
    est = ref.CowPoseEstimator()
    pipe = ref.TLEAPPipeline.__new__(ref.TLEAPPipeline)
    image = np.zeros((H, W, 3), np.uint8)
    rng = np.random.default_rng(20240611)

    boxes = [[10.99, 20.5, 210.01, 140.75], [0.0, 0.0, 0.9, 0.5], [100.2, 50.7, 100.9, 300.1], [1279.4, 700.6, 1280.0, 720.0],
             [-3.7, -0.2, 55.5, 41.9], [300.0, 200.0, 900.0, 650.0], [640.5, 10.25, 1279.99, 719.99], [12.0, 500.0, 13.0, 501.0]]
    out = {"keypoint_names": ref.KEYPOINT_NAMES, "skeleton": [list(p) for p in ref.COW_SKELETON],
           "colors": {k: list(v) for k, v in ref.SKELETON_COLORS.items()},
           "bbox": [{"bbox": f32(b), "keypoints": est.estimate_pose_from_bbox(image, f32(b), H, W)} for b in boxes], "cases": {}, "locomotion": []}

    cases = {"trained_20_3": trained_case(20, 3, rng), "trained_20_2": trained_case(20, 2, rng), "trained_17_3": trained_case(17, 3, rng)}
    cases.update(heuristic_cases(rng))
    for name, case in cases.items():
        pose = case["mode"] == "trained"
        est.use_trained_model = pose
        est.model = Model({int(k): v for k, v in case.get("names", {}).items()}, pose)
        detections = []
        for fr in case["frames"]:
            est.model.frame = fr
            detections.append(est.detect_and_estimate(image))
        case["detections"] = detections
        out["cases"][name] = case

    def sequences(case):
        seq = []
        for fid, dets in zip(case["frame_ids"], case["detections"]):
            for det in dets:
                seq.append({"frame": fid, "time": fid / case["fps"], "bbox": det["bbox"], "keypoints": det["keypoints"],
                            "detection_confidence": det["confidence"]})
        return seq

    for name, rows in (("heuristic_walk", None), ("heuristic_walk", 0), ("heuristic_walk", 1), ("heuristic_walk", 2), ("heuristic_walk", 7),
                       ("heuristic_mixed", None), ("trained_20_3", None), ("trained_20_2", None), ("trained_17_3", None)):
        seq = sequences(out["cases"][name])
        seq = seq if rows is None else seq[:rows]
        out["locomotion"].append({"case": name, "rows": len(seq), "features": pipe.compute_locomotion_features(seq)})

    path = os.path.join(HERE, "tleap_reference.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
