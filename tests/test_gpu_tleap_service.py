"""TLEAPPipeline over the real HIP backends: the synthetic yolov8n-pose detector of test_gpu_services.py (model type `trained`) and a
synthetic yolov8n (`heuristic`) on short synthetic clips.  `{id}_tleap.json` is written, `pipeline.tleap` is published, and the two gait
consumers write the same bytes whether they read that file or are handed the clip from the device."""
import asyncio
import json

import numpy as np
import pytest
import torch

import tcnref
import xfmref
from lmx import checkpoints, synth, tcn, xfm, yolo
from lmx.services import TCNPipeline, TLEAPPipeline, TransformerPipeline
from lmx.services import runtime as R

pytestmark = pytest.mark.gpu
COW_NAMES = [f"cow_{i}" if i < 10 else f"class_{i}" for i in range(80)]  # ten classes the heuristic mode accepts by name, and id 19


@pytest.fixture(scope="module")
def backends(cuda):
    pcfg = yolo.YoloConfig("n", nc=1, kpt_shape=(17, 3))
    pose = yolo.YoloDetector(pcfg, yolo.synthetic_state_dict(pcfg, 7, yolo.bn_stats_path("n", pose=True)), cuda)
    dcfg = yolo.YoloConfig("n")
    det = yolo.YoloDetector(dcfg, yolo.synthetic_state_dict(dcfg, 7, yolo.bn_stats_path("n")), cuda, names=COW_NAMES)
    _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(tcnref.SHIPPED, 21), tcnref.SHIPPED.dropout)
    _, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(xfmref.SHIPPED, 21), n_heads=xfmref.SHIPPED.n_heads, dropout=xfmref.SHIPPED.dropout)
    return {"trained": pose, "heuristic": det, "tcn": tcn.TcnScorer(tcnref.SHIPPED, folded, device=cuda),
            "xfm": xfm.XfmScorer(xfmref.SHIPPED, w, device=cuda)}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("clips")
    frames = np.stack([synth.synth_frame(3, 40 + 3 * i) for i in range(12)], 0)
    R.save_npz_clip(d / "walk_a.npz", frames, 10.0)      # every 2nd frame: 6 sampled
    R.save_npz_clip(d / "walk_b.npz", frames[::-1], 29.97)  # every 5th frame: 0, 5, 10
    return {v: {"video_id": v, "processed_path": str(d / f"{v}.npz")} for v in ("walk_a", "walk_b")}


def consumers(backends, bus, tleap_dir, out):
    cfg = {"nats": {"subjects": {}}}
    return [TCNPipeline(backends["tcn"], bus, config=cfg, tleap_dir=tleap_dir, results_dir=out / "tcn"),
            TransformerPipeline(backends["xfm"], bus, config=cfg, tleap_dir=tleap_dir, results_dir=out / "transformer")]


def gait_files(out):
    return {p.name: p.read_bytes() for sub in ("tcn", "transformer") for p in sorted((out / sub).iterdir())}


@pytest.mark.parametrize("mode", ["trained", "heuristic"])
def test_frames_to_scores(backends, clips, tmp_path, mode):
    cfg = {"nats": {"subjects": dict(R.DEFAULT_SUBJECTS)}}
    bus = R.InProcessBus()
    handed = consumers(backends, bus, tmp_path / "unused", tmp_path / "handed")
    svc = TLEAPPipeline(backends[mode], bus, cfg, results_dir=tmp_path / "tleap", consumers=handed, conf=0.05 if mode == "trained" else None)
    assert svc.model_type == mode and (mode == "trained" or svc.cow_classes == list(range(10)) + [19])

    async def one_at_a_time():
        await svc.process_video(clips["walk_a"])
        await svc.process_video(clips["walk_b"])

    asyncio.run(one_at_a_time())
    docs = {v: json.load(open(tmp_path / "tleap" / f"{v}_tleap.json")) for v in clips}
    a, b = docs["walk_a"], docs["walk_b"]
    assert a["frames_processed"] >= 6 and a["model_type"] == mode and a["fps"] == 10.0 and a["total_frames"] == 12
    assert sorted({r["frame"] for r in a["pose_sequences"]}) <= [0, 2, 4, 6, 8, 10] and all(r["time"] == r["frame"] / 10.0 for r in a["pose_sequences"])
    assert b["fps"] == 29.97 and {r["frame"] for r in b["pose_sequences"]} <= {0, 5, 10} and all(r["time"] == r["frame"] / 29.97 for r in b["pose_sequences"])
    assert b["frames_processed"] >= 1
    n_kp = 17 if mode == "trained" else 20
    for doc in docs.values():
        for r in doc["pose_sequences"]:
            assert len(r["keypoints"]) == n_kp and all(list(k) == ["name", "x", "y", "confidence"] for k in r["keypoints"])
            conf = sum(k["confidence"] for k in r["keypoints"]) / 20 * r["detection_confidence"]
            assert abs(conf - 0.3) > 1e-6  # np.mean and the index-order sum may differ in the last place: keep the data off the threshold
    if mode == "heuristic":
        assert a["locomotion_features"] and "lameness_score" in a["locomotion_features"]
    else:
        assert a["locomotion_features"] == {}  # a trained model's names match `withers` only

    # the messages: tleap, then the consumers it hands the clip to
    subjects = [s for s, m in bus.published if m["video_id"] == "walk_a"]
    assert subjects[0] == "pipeline.tleap" and subjects[1:2] == ["pipeline.tcn"] and set(subjects[2:]) <= {"pipeline.transformer"}
    msg = bus.published[0][1]
    assert msg == {"video_id": "walk_a", "pipeline": "tleap", "results_path": str(tmp_path / "tleap" / "walk_a_tleap.json"),
                   "features": a["locomotion_features"], "frames_processed": a["frames_processed"], "model_type": mode}

    # the same two consumers fed from the file write the same bytes
    bus2 = R.InProcessBus()
    filed = consumers(backends, bus2, tmp_path / "tleap", tmp_path / "filed")

    async def from_files():
        for c in filed:
            for v in clips:
                await c.process_video({"video_id": v})

    asyncio.run(from_files())
    got, want = gait_files(tmp_path / "handed"), gait_files(tmp_path / "filed")
    assert got == want and {"walk_a_tcn.json", "walk_b_tcn.json"} <= set(got)
    if mode == "heuristic":
        assert "walk_a_transformer.json" in got  # an assumed box has confidence 0.705 x 0.5: its step is not masked

    # the backlog in one series launch: the same files
    singles = {v: (tmp_path / "tleap" / f"{v}_tleap.json").read_bytes() for v in clips}
    bus3 = R.InProcessBus()
    batch = TLEAPPipeline(backends[mode], bus3, cfg, results_dir=tmp_path / "tleap_batch", consumers=consumers(backends, bus3, tmp_path / "unused", tmp_path / "batch"),
                          conf=0.05 if mode == "trained" else None)
    asyncio.run(batch.process_videos([clips["walk_a"], {"video_id": "absent", "processed_path": str(tmp_path / "absent.npz")}, clips["walk_b"]]))
    assert {v: (tmp_path / "tleap_batch" / f"{v}_tleap.json").read_bytes() for v in clips} == singles
    assert gait_files(tmp_path / "batch") == got
    assert [s for s, _ in bus3.published][:2] == ["pipeline.tleap", "pipeline.tleap"]


@pytest.mark.parametrize("mode", ["trained", "heuristic"])
def test_c_example_chains_the_same_launches(backends, cuda, tmp_path, mode):
    """examples/tleap_gait.c, compiled with cc against include/lmx.h and liblmx.so and run as a child process on exported images: its
    rows, masked steps and the two scores' bits are those of the Python path over the same frames."""
    import os
    import shutil
    import subprocess

    from lmx import _lib, native, tleap

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cc = shutil.which("cc")
    assert cc, "no C compiler named cc"
    det, conf, seed = backends[mode], 0.05 if mode == "trained" else 0.3, 2 ** 63 + 77
    frames = torch.from_numpy(np.stack([synth.synth_frame(3, 40 + 6 * i) for i in range(4)], 0)).to(cuda)
    n, h, w = frames.shape[:3]
    if mode == "trained":
        b, s, c, _, k, kp = det.detect_pose(frames, conf=conf)
    else:
        (b, s, c, _, k), kp = det.detect(frames, conf=conf), None
    series_fn = tleap.PoseSeries(mode, sorted({19} | {i for i, name in det.names.items() if "cow" in name}))
    rows, _, series, mask = series_fn(b, s, c, k, kp, (h, w), [0, n])
    want = [f"model_type {mode}", f"frames {n}", f"rows {int(rows[0])}", f"masked_steps {int(mask[0].sum())}"]
    mean, std, _ = backends["tcn"].score(series, [seed], n_samples=10)
    want.append(f"tcn bits {float(mean[0]).hex()} {float(std[0]).hex()}")
    if not bool(mask[0].all()):
        mean, std, _ = backends["xfm"].score(series, mask, [seed], n_samples=10)
        want.append(f"transformer bits {float(mean[0]).hex()} {float(std[0]).hex()}")
    assert int(rows[0]) >= 1

    images = {name: tmp_path / f"{name}.lmx" for name in ("yolo", "tcn", "xfm")}
    native.write_yolo_image(det, images["yolo"])
    native.write_tcn_image(backends["tcn"].cfg, checkpoints.tcn_from_state_dict(tcnref.state_dict(tcnref.SHIPPED, 21), tcnref.SHIPPED.dropout)[1], images["tcn"])
    native.write_xfm_image(backends["xfm"].cfg, checkpoints.xfm_from_state_dict(xfmref.state_dict(xfmref.SHIPPED, 21), n_heads=xfmref.SHIPPED.n_heads,
                                                                                 dropout=xfmref.SHIPPED.dropout)[1], images["xfm"])
    raw = tmp_path / "frames.raw"
    raw.write_bytes(np.array([n, h, w], np.int32).tobytes() + frames.cpu().numpy().tobytes())
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "tleap_gait"
    subprocess.run([cc, "-O1", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "tleap_gait.c"), "-o", str(exe), "-L", libdir, "-llmx", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    f"-Wl,-rpath,{libdir}"], check=True, timeout=120)
    # the HIP runtime this process loaded, first on the child's search path (as tests/test_gpu_native_yolo.py does)
    hip = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(hip) == 1, hip
    hipdir, soname, search = os.path.dirname(hip[0]), "libamdhip64.so.7", [os.path.dirname(hip[0])]
    if not os.path.exists(os.path.join(hipdir, soname)):
        rt = tmp_path / "rt"
        rt.mkdir()
        os.symlink(hip[0], rt / soname)
        search.append(str(rt))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join(search + [p for p in env.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p])
    r = subprocess.run([str(exe), str(images["yolo"]), str(images["tcn"]), str(images["xfm"]), str(raw), str(seed), repr(conf)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    got = lines[:4] + [" ".join([ln.split()[0], "bits", *(float.fromhex(v).hex() for v in ln.split()[-2:])]) for ln in lines[4:] if " bits " in ln]
    assert got == want, (got, want)
    loco = [ln for ln in lines if ln.split()[0] in _lib.TleapLocomotion.KEYS]
    assert (len(loco) == 0) if mode == "trained" or int(rows[0]) < 2 else ("lameness_score" in loco[-1])
