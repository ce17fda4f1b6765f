"""Frames in HBM to the TCN and transformer scores on two routes, for one clip of 25 sampled 720p frames and for a backlog of 64:
  (a) the device route: detect_pose -> lmx_k_tleap_series -> TcnScorer / XfmScorer on the series and mask where they lie
      (a+) the same with what TLEAPPipeline adds for its file: ONE download of the records and json.dump of `{id}_tleap.json`;
  (b) the route assembled from the public pieces that existed before the kernel: PoseEstimator.detect_with_trained_model, tleap's blend
      restated in Python, json.dump, then TCNPipeline / TransformerPipeline reading the file (GaitPipeline._features) and scoring.
The routes alternate, three repeats each; a host clock around work that ends in a device synchronise.  The pose model's own time is
reported separately (it is inside both routes and dominates them), and the series kernel's own time (HIP events) beside the HBM bytes it
has to move.  Writes profiles/tleap_ab.txt.

    python tools/tleap_ab.py [--repeats 3] [--out profiles/tleap_ab.txt]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tcnref  # noqa: E402
import tleapref  # noqa: E402
import xfmref  # noqa: E402
from lmx import checkpoints, synth, tcn, tleap, xfm, yolo  # noqa: E402
from lmx.services import PoseEstimator, TCNPipeline, TransformerPipeline  # noqa: E402
from lmx.services.runtime import InProcessBus  # noqa: E402
from lmx.services.tleap_pipeline import pose_sequences_from_records  # noqa: E402

FRAMES, H, W, BATCH, CONF, KPT = 25, 720, 1280, 32, 0.05, (17, 3)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-det", type=int, default=300, help="detections kept per frame (a real clip shows a cow or two; synthetic weights fill any limit)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tleap_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tleap_ab needs a GPU"
    dev = torch.device("cuda:0")
    pcfg = yolo.YoloConfig("n", nc=1, kpt_shape=KPT)
    det = yolo.YoloDetector(pcfg, yolo.synthetic_state_dict(pcfg, 7, yolo.bn_stats_path("n", pose=True)), dev)
    _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(tcnref.SHIPPED, 21), tcnref.SHIPPED.dropout)
    _, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(xfmref.SHIPPED, 21), n_heads=xfmref.SHIPPED.n_heads, dropout=xfmref.SHIPPED.dropout)
    tcn_s, xfm_s = tcn.TcnScorer(tcnref.SHIPPED, folded, device=dev), xfm.XfmScorer(xfmref.SHIPPED, w, device=dev)

    class Capped:  # the detector with the run's max_det, for PoseEstimator (which passes none)
        cfg = det.cfg

        def detect_pose(self, frames, conf=0.25):
            return det.detect_pose(frames, conf=conf, max_det=args.max_det)

    series_fn, estimator = tleap.PoseSeries("trained"), PoseEstimator(Capped(), conf=CONF)
    tmp = tempfile.mkdtemp(prefix="tleap_ab_")
    cfg = {"nats": {"subjects": {}}}
    tcn_p = TCNPipeline(tcn_s, InProcessBus(), config=cfg, tleap_dir=tmp, results_dir=os.path.join(tmp, "tcn"))
    xfm_p = TransformerPipeline(xfm_s, InProcessBus(), config=cfg, tleap_dir=tmp, results_dir=os.path.join(tmp, "xfm"))
    clip = torch.from_numpy(np.stack([synth.synth_frame(3, 40 + 2 * i, H, W) for i in range(FRAMES)], 0)).to(dev)
    frame_ids = [5 * i for i in range(FRAMES)]
    lines = [f"{torch.cuda.get_device_properties(dev).name}; clips of {FRAMES} sampled {W} x {H} frames, synthetic yolov8n-pose (K = {KPT[0]}) at conf {CONF} and max_det {args.max_det} in batches of "
             f"{BATCH}, shipped TCN and gait transformer, S = 10; {args.repeats} alternating repeats, host clock around work that ends in a device synchronise, ms"]

    for n in (1, 64):
        ids = [f"clip_{i}" for i in range(n)]
        frames = clip.repeat(n, 1, 1, 1) if n > 1 else clip
        first = [FRAMES * c for c in range(n + 1)]

        def detect():
            parts = [det.detect_pose(frames[i:i + BATCH], conf=CONF, max_det=args.max_det) for i in range(0, len(frames), BATCH)]
            return [torch.cat([p[j] for p in parts], 0).contiguous() for j in (0, 1, 2, 4, 5)]

        def score(series, mask):
            a = tcn_s.score(series, [tcn.clip_seed(v) for v in ids], n_samples=10)
            b = xfm_s.score(series, mask, [xfm.clip_seed(v) for v in ids], n_samples=10)
            return a[0].cpu().numpy(), b[0].cpu().numpy(), xfm_s.saliency(series).cpu().numpy()

        def route_a(files=False):
            boxes, scores, cls, counts, kpts = detect()
            rows, records, series, mask = series_fn(boxes, scores, cls, counts, kpts, (H, W), first)
            if files:
                per_clip = tleap.PoseSeries.records(rows, records, first, boxes.shape[1])
                for v, rec in zip(ids, per_clip):
                    with open(os.path.join(tmp, f"{v}_tleap.json"), "w") as f:
                        json.dump({"video_id": v, "pose_sequences": pose_sequences_from_records(rec, frame_ids, 25.0, True)}, f, indent=2)
            return score(series, mask), rows

        def route_b():
            per_frame = []
            for i in range(0, len(frames), BATCH):
                for dets in estimator.detect_with_trained_model(frames[i:i + BATCH]):
                    out = []
                    for d in dets:  # tleap's blend (main.py:173-195), restated
                        heuristic = {kp["name"]: kp for kp in tleapref.estimate_pose_from_bbox(d["bbox"])}
                        final = []
                        for name in tleapref.KEYPOINT_NAMES:
                            mk = d["model_keypoints"].get(name)
                            if mk is not None and mk["confidence"] > 0.3:
                                final.append(mk)
                            elif name in heuristic:
                                final.append(heuristic[name])
                            elif mk is not None:
                                final.append(mk)
                        out.append({"bbox": d["bbox"], "confidence": d["confidence"], "keypoints": final})
                    per_frame.append(out)
            ready_t, ready_x = [], []
            for c, v in enumerate(ids):
                seq = tleapref.pose_sequences(per_frame[first[c]:first[c + 1]], frame_ids, 25.0)
                with open(os.path.join(tmp, f"{v}_tleap.json"), "w") as f:
                    json.dump({"video_id": v, "pose_sequences": seq}, f, indent=2)
                ct, cx = tcn_p._features(v), super(TransformerPipeline, xfm_p)._features(v)  # all-masked clips are scored too, as in (a)
                ready_t.append(ct)
                ready_x.append(cx)
            a = tcn_p._score(ids, *[list(x) for x in zip(*ready_t)])
            b = xfm_p._score(ids, *[list(x) for x in zip(*ready_x)])
            return (a[0], b[0], b[2]), None

        t_pose, t_a, t_af, t_b = [], [], [], []
        ra, rows = route_a()  # warm-up of every shape, and the outputs to compare
        route_a(True)
        rb = route_b()[0]
        same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ra, rb))
        for _ in range(args.repeats):
            t_pose.append(wall(detect)[0])
            t_a.append(wall(route_a)[0])
            t_b.append(wall(route_b)[0])
            t_af.append(wall(lambda: route_a(True))[0])
        # the series kernel alone, and the bytes it has to move
        boxes, scores, cls, counts, kpts = detect()
        e0, e1, iters = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), 20
        series_fn(boxes, scores, cls, counts, kpts, (H, W), first)
        e0.record()
        for _ in range(iters):
            series_fn(boxes, scores, cls, counts, kpts, (H, W), first)
        e1.record()
        e1.synchronize()
        t_kernel = e0.elapsed_time(e1) / iters
        T0 = int(rows.sum())
        moved = len(frames) * 4 + T0 * (16 + 4 + KPT[0] * KPT[1] * 4 + 8 + 8 + 536) + n * 125 * (44 * 4 + 1)

        def cell(v):
            return f"{statistics.median(v):9.2f} [{min(v):.2f} .. {max(v):.2f}]"

        lines += [f"--- {n} clip{'s' if n > 1 else ''}: {len(frames)} frames, {T0} rows; scores of (a) and (b) bit-identical: {same}",
                  f"pose model alone (detect_pose, inside both routes)      {cell(t_pose)}",
                  f"(a)  device route                                       {cell(t_a)}",
                  f"(a+) device route + records download + tleap.json       {cell(t_af)}",
                  f"(b)  host route (PoseEstimator, Python blend, json, GaitPipeline from the file) {cell(t_b)}",
                  f"spread of (b) over its repeats {max(t_b) - min(t_b):.2f} ms; median (a) - median (b) = {statistics.median(t_a) - statistics.median(t_b):+.2f} ms; "
                  f"median (a+) - median (b) = {statistics.median(t_af) - statistics.median(t_b):+.2f} ms",
                  f"lmx_k_tleap_series alone (allocations, the clip bounds' copy and the launch; HIP events, {iters} calls): {t_kernel * 1e3:.1f} us for "
                  f"{moved / 1e6:.3f} MB that have to move (row inputs, row map, records, series, mask) = {moved / 1e9 / (t_kernel / 1e3):.2f} GB/s"]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
