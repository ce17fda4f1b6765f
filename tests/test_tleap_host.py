"""The pose series on the host: lmx_h_tleap_series (csrc/host_tleap.cpp, the twin of the kernel), lmx.tleap.PoseSeries(backend="host"),
the restatement tests/tleapref.py and lmx_h_tleap_locomotion against what the reference's own functions returned
(tests/golden/tleap_reference.json, recorded by tests/golden/record_tleap.py).  No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import tleapref as R
from lmx import _lib, tleap
from lmx import kernels as K
from lmx.services.tcn_pipeline import TCNPipeline
from lmx.services.tleap_pipeline import compute_locomotion_features
from lmx.services.transformer_pipeline import TransformerPipeline

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tleap_reference.json")))
CASES = sorted(FIXTURE["cases"])
LOOSE = ("back_arch_mean", "back_arch_std", "back_arch_score", "lameness_score")  # arccos and the 2-norm go through libm / SVML


def host_series(case, target=125, via="kernels"):
    boxes, scores, cls, counts, kpts = (torch.from_numpy(a) if a is not None else None for a in R.case_arrays(case))
    names = {int(k): v for k, v in case.get("names", {}).items()}
    first = [0, len(counts)]
    if via == "PoseSeries":
        ps = tleap.PoseSeries(case["mode"], R.cow_classes(names), target=target, backend="host")
        rows, rec, series, mask = ps(boxes, scores, cls, counts, kpts, (case["h"], case["w"]), first)
    else:
        rows, rec, series, mask = K.tleap_series(boxes, scores, cls, counts, kpts, (case["h"], case["w"]), first, target, R.cow_classes(names), host=True)
    records = tleap.PoseSeries.records(rows, rec, first, boxes.shape[1])[0]
    return records, series[0].numpy(), mask[0].numpy()


def fixture_rows(case):
    return [(i, {k: d[k] for k in ("bbox", "confidence", "keypoints")}) for i, dets in enumerate(case["detections"]) for d in dets]


def test_restatement_equals_the_reference():
    assert R.KEYPOINT_NAMES == FIXTURE["keypoint_names"]
    for b in FIXTURE["bbox"]:
        assert R.estimate_pose_from_bbox(b["bbox"]) == b["keypoints"]
    for name in CASES:
        assert R.case_detections(FIXTURE["cases"][name]) == FIXTURE["cases"][name]["detections"], name


@pytest.mark.parametrize("via", ["kernels", "PoseSeries"])
@pytest.mark.parametrize("name", CASES)
def test_records_equal_the_reference(name, via):
    case = FIXTURE["cases"][name]
    records, _, _ = host_series(case, via=via)
    assert R.records_as_detections(records, case["mode"] == "trained") == fixture_rows(case)
    assert not records["reserved"].any()
    if case["mode"] == "heuristic":  # the assumed rows carry detection index -1
        want = [-1 if d["class"] == "cow_assumed" else None for dets in case["detections"] for d in dets]
        assert all(w is None or g == w for g, w in zip(records["det"], want)) and sum(w == -1 for w in want) == int((records["det"] == -1).sum())


def test_heuristic_keypoints_of_single_boxes_equal_the_reference():
    """estimate_pose_from_bbox on the fixture's boxes (fractional corners, width below 1, the frame's edge) through the twin"""
    for b in FIXTURE["bbox"]:
        case = {"mode": "heuristic", "h": 720, "w": 1280, "names": {"19": "cow"}, "frames": [{"boxes": [b["bbox"]], "scores": [0.5], "cls": [19]}]}
        records, _, _ = host_series(case)
        assert R.records_as_detections(records, False)[0][1]["keypoints"] == b["keypoints"]


@pytest.mark.parametrize("target", [125, 3])
@pytest.mark.parametrize("name", CASES)
def test_series_and_mask_are_the_gait_features_of_the_records(name, target):
    case = FIXTURE["cases"][name]
    records, series, mask = host_series(case, target)
    kp = np.ascontiguousarray(records["keypoints"][:, :, :2])
    assert np.array_equal(series, K.tcn_features(kp, records["n_kp"], records["bbox"], target))
    assert np.array_equal(mask, K.xfm_mask(np.ascontiguousarray(records["keypoints"][:, :, 2]), records["n_kp"], records["confidence"], target))
    # and what the consumers compute from the JSON
    doc = json.loads(json.dumps({"pose_sequences": R.pose_sequences(case["detections"], list(range(len(case["detections"]))), 5.0)}))
    tcn, xfm = object.__new__(TCNPipeline), object.__new__(TransformerPipeline)
    tcn.TARGET_LENGTH = xfm.TARGET_LENGTH = target
    assert np.array_equal(series, tcn._clip(doc)[0])
    s, m = xfm._clip(doc)
    assert np.array_equal(series, s) and np.array_equal(mask.astype(bool), m)


def test_clip_without_rows_is_zero_and_fully_masked():
    case = dict(FIXTURE["cases"]["trained_17_3"])
    case["frames"] = [case["frames"][1]] * 3  # the frame without a detection
    records, series, mask = host_series(case)
    assert len(records) == 0 and not series.any() and mask.all() and series.shape == (125, 44)


def sequences(entry):
    case = FIXTURE["cases"][entry["case"]]
    return case, R.pose_sequences(case["detections"], case["frame_ids"], case["fps"])[:entry["rows"]]


@pytest.mark.parametrize("i", range(len(FIXTURE["locomotion"])))
def test_python_locomotion_equals_the_reference(i):
    entry = FIXTURE["locomotion"][i]
    got = compute_locomotion_features(sequences(entry)[1])
    assert list(got) == list(entry["features"])
    for k, v in entry["features"].items():
        assert got[k] == (pytest.approx(v, rel=1e-12, abs=0) if k in LOOSE else v), k
    assert R.locomotion(sequences(entry)[1]).keys() == got.keys()


@pytest.mark.parametrize("i", range(len(FIXTURE["locomotion"])))
def test_c_locomotion_is_within_its_bound_of_the_reference(i):
    """rel 1e-11: at most about 1500 sequential terms x 2^-53 x a condition number of at most 10 is about 1.7e-12, a margin of about 6.
    The bound needs |cos| <= 0.99 and std >= 1e-6 |mean| on the inputs: both asserted here."""
    entry = FIXTURE["locomotion"][i]
    case, seq = sequences(entry)
    records, _, _ = host_series(case)
    records = records[:entry["rows"]]
    trained = case["mode"] == "trained"
    names = R.KEYPOINT_NAMES if trained else R.HEURISTIC_NAMES
    got = K.tleap_locomotion(records, names)
    want = entry["features"]
    assert list(got) == list(want)  # the presence mask, in the reference's key order
    if trained:
        assert want == {} and len(records) >= 2  # the quirk: a trained model's names match `withers` only
    for row in seq:
        d = {kp["name"]: kp for kp in row["keypoints"]}
        if {"throat", "withers", "tailbase"} <= d.keys():
            v1 = (d["throat"]["x"] - d["withers"]["x"], d["throat"]["y"] - d["withers"]["y"])
            v2 = (d["tailbase"]["x"] - d["withers"]["x"], d["tailbase"]["y"] - d["withers"]["y"])
            assert abs((v1[0] * v2[0] + v1[1] * v2[1]) / (math.hypot(*v1) * math.hypot(*v2))) <= 0.99
    for k in want:
        if k.endswith("_std") or k == "head_bob_magnitude":
            mean_key = {"back_arch_std": "back_arch_mean", "head_bob_magnitude": None}.get(k, k.replace("_std", "_mean"))
            if entry["rows"] == 2 and mean_key is not None and mean_key.startswith("stride"):
                assert want[k] == 0.0 and got[k] == 0.0  # two rows are ONE stride: its deviation is exactly 0 on both sides, no bound needed
            else:
                assert mean_key is None or want[k] >= 1e-6 * abs(want[mean_key])
    for k, v in want.items():
        assert got[k] == (v if k == "head_bob_frequency" else pytest.approx(v, rel=1e-11, abs=0)), k


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _call(fn="lmx_h_tleap_series", **over):
    F, md, Kk, nd, n, target = 4, 3, 17, 3, 2, 125
    a = {"boxes": np.zeros((F, md, 4), np.float32), "scores": np.zeros((F, md), np.float32), "cls": np.zeros((F, md), np.int32),
         "counts": np.zeros((F,), np.int32), "kpts": np.zeros((F, md, Kk, nd), np.float32), "K": Kk, "ndim": nd, "F": F, "max_det": md, "h": 720,
         "w": 1280, "clip_first": np.array([0, 1, 4], np.int32), "n": n, "target": target, "mode": K.TLEAP_TRAINED,
         "cow": np.array([19], np.int32), "n_cow": 1, "rows": np.zeros((n,), np.int32), "records": np.zeros((F * md, 536), np.uint8),
         "series": np.zeros((n, target, 44), np.float32), "mask": np.zeros((n, target), np.uint8)}
    a.update(over)

    def p(v):
        return C.c_void_p(v if isinstance(v, int) else (v.ctypes.data if v is not None else 0))

    lib = _lib.load()
    rc = getattr(lib, fn)(p(a["boxes"]), p(a["scores"]), p(a["cls"]), p(a["counts"]), p(a["kpts"]), a["K"], a["ndim"], a["F"], a["max_det"], a["h"],
                          a["w"], p(a["clip_first"]), a["n"], a["target"], a["mode"], p(a["cow"]), a["n_cow"], p(a["rows"]), p(a["records"]),
                          p(a["series"]), p(a["mask"]))
    return rc, lib.lmx_last_error().decode()


REFUSALS = [
    ({"boxes": None}, "boxes"), ({"scores": None}, "scores"), ({"cls": None}, "cls"), ({"counts": None}, "counts"), ({"rows": None}, "rows"),
    ({"records": None}, "records"), ({"series": None}, "series"), ({"mask": None}, "mask"), ({"clip_first": None}, "clip_first_host"),
    ({"kpts": None}, "kpts"), ({"mode": K.TLEAP_HEURISTIC}, "kpts"), ({"mode": 2}, "mode"), ({"ndim": 1}, "ndim"), ({"ndim": 4}, "ndim"),
    ({"K": 2}, "K"), ({"target": 0}, "target"), ({"target": 65537}, "target"), ({"clip_first": np.array([0, 2, 2], np.int32), "F": 2}, "clip_first_host"),
    ({"clip_first": np.array([0, 3, 2], np.int32), "F": 2}, "clip_first_host"), ({"clip_first": np.array([1, 2, 4], np.int32)}, "clip_first_host"),
    ({"clip_first": np.array([0, 2, 3], np.int32)}, "clip_first_host"), ({"F": 0}, "F"), ({"max_det": 0}, "max_det"), ({"h": 0}, "h"), ({"n": 0}, "n"),
    ({"mode": K.TLEAP_HEURISTIC, "kpts": None, "n_cow": 17}, "n_cow"), ({"mode": K.TLEAP_HEURISTIC, "kpts": None, "cow": None}, "cow_classes_host"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_name_the_argument(i):
    over, word = REFUSALS[i]
    rc, msg = _call(**over)
    assert rc == -1 and msg.startswith("lmx_h_tleap_series: ") and word in msg, (rc, msg)


@pytest.mark.parametrize("name", ["boxes", "scores", "cls", "counts", "kpts", "rows", "records", "series"])
def test_misaligned_pointers_are_refused(name):
    rc0, _ = _call()
    assert rc0 == 0
    buf = np.zeros((4096,), np.uint8)
    rc, msg = _call(**{name: buf.ctypes.data + (-buf.ctypes.data % 8) + 1})
    assert rc == -1 and name in msg and "aligned" in msg, (rc, msg)


def test_locomotion_refusals_and_workspace():
    lib = _lib.load()
    out = _lib.TleapLocomotion()
    names = (C.c_char_p * 20)(*[n.encode() for n in R.HEURISTIC_NAMES])
    rec = np.zeros((3,), K.tleap_record_dtype())
    assert lib.lmx_h_tleap_locomotion(None, 3, names, C.byref(out)) == -1 and "records_host" in lib.lmx_last_error().decode()
    assert lib.lmx_h_tleap_locomotion(C.c_void_p(rec.ctypes.data), 3, None, C.byref(out)) == -1 and "names_host" in lib.lmx_last_error().decode()
    assert lib.lmx_h_tleap_locomotion(C.c_void_p(rec.ctypes.data), 3, names, None) == -1 and "out_host" in lib.lmx_last_error().decode()
    assert lib.lmx_h_tleap_locomotion(C.c_void_p(rec.ctypes.data), -1, names, C.byref(out)) == -1 and "rows" in lib.lmx_last_error().decode()
    assert K.tleap_record_dtype().itemsize == 536
    assert lib.lmx_tleap_workspace_bytes(5, 300) == 8 * 3 + 5 * 300 * 8 and lib.lmx_tleap_workspace_bytes(0, 300) == 0
