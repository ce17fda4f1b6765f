"""Latency of one 1080p frame through lmx_sam_segment (csrc/sam_model.hip) against the Python plan it restates — SamVitEncoder.encode +
MaskDecoder.predict on sam_vit_b(), or with --encoder hiera HieraEncoder(band="blocks").encode(outputs="embedding") +
MaskDecoder.predict on Hiera-B+ — with synthetic weights, per precision plan.  The device work is the same, launch for launch; what
the C path can save is host time per launch.  Each call is timed with a host clock between stream synchronisations; the two paths
alternate call by call; 5 warm-ups, then the median (and the quartiles) of `--calls` calls.

    python tools/native_sam_latency.py [--encoder vit|hiera] [--calls 25] [--h 1080 --w 1920]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lmx import native, sam, sam_decoder, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", choices=("vit", "hiera"), default="vit")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("native_sam_latency: needs a GPU")
    dev = torch.device("cuda:0")
    hiera = a.encoder == "hiera"
    if hiera:
        cfg = sam.hiera_b_plus()
        enc = sam.HieraEncoder(cfg, weights.synth_state_dict(sam.param_spec(cfg), 5), dev, band="blocks")
    else:
        cfg = sam.sam_vit_b()
        enc = sam.SamVitEncoder(cfg, weights.synth_state_dict(sam.vit_param_spec(cfg), 5), dev)
    model = "hiera_b_plus" if hiera else "sam_vit_b"
    py_name = ("HieraEncoder.encode(embedding)" if hiera else "SamVitEncoder.encode") + " + MaskDecoder.predict"
    dec = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), dev)
    h, w = a.h, a.w
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)).to(dev)
    boxes = torch.tensor([[0.25 * w, 0.25 * h, 0.75 * w, 0.7 * h]], dtype=torch.float32, device=dev)
    rhw = sam.resize_longest_side(h, w, cfg.image)
    print(f"{model}, one {h} x {w} frame, one box; {a.warmup} warm-ups, median [quartiles] of {a.calls} calls, host clock between stream synchronisations")
    with tempfile.TemporaryDirectory() as tmp:
        for plan in ("f16", "exact"):
            path = os.path.join(tmp, f"{model}_{plan}.lmx")
            native.write_sam_image(enc, dec, path, (plan,))
            with native.NativeSam(path, 1, dev) as ns:
                ns.prepare(h, w, plan)

                def python_plan():
                    emb = enc.encode(frames, plan, outputs="embedding")["fpn"][2]
                    return dec.predict(emb.view(-1, 256), boxes, (h, w), rhw, plan)

                def c_plan():
                    return ns.segment(frames, boxes, plan, outputs=("mask", "lowres"))

                ref, got = python_plan(), c_plan()
                same = all(torch.equal(got[k], ref[k]) for k in ("mask", "stats", "iou", "lowres"))
                times = {"python": [], "c": []}
                for i in range(a.warmup + a.calls):
                    for name, fn in (("python", python_plan), ("c", c_plan)):
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize(dev)
                        if i >= a.warmup:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                for name in ("python", "c"):
                    q = statistics.quantiles(times[name], n=4)
                    what = py_name if name == "python" else "lmx_sam_segment"
                    print(f"plan {plan:5s}  {what:52s} {statistics.median(times[name]):8.3f} ms  [{q[0]:.3f} .. {q[2]:.3f}]")
                print(f"plan {plan:5s}  outputs equal bit for bit: {same}")
            os.unlink(path)


if __name__ == "__main__":
    main()
