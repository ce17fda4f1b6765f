"""The SAM mask decoder at whatever commit is checked out: its bits, its launch order and its time, to be compared between two commits
(a refactor of MaskDecoder / struct Dec of csrc/sam_model.hip must leave the first two as they are).  Synthetic weights (encoder S64 of
tests/test_gpu_native_sam.py with seed 5, decoder seed 6 plus the mask-embedding weights of seed 7), both precision plans.

  1 bits    sha256 of lowres and iou of MaskDecoder on four prompt kinds (predict with a box; decode with points; with points, a box and
            a mask input; with points and multimask) and of every output of NativeSam.segment, n = 3, the 96x160 and 64x64 frames of
            tests/test_gpu_native_sam.py
  2 order   the (class, key) list lmx.kernels' launch trace collects around one predict and one decode(multimask, mask_input) per plan,
            with its sha256; and the kernel names of one lmx_sam_decode per plan in start order, from a rocprofv3 --kernel-trace run of
            a child process of its own (no counters)
  3 time    median of 50 calls after 10 warm-ups, device events: the four Python cases per plan at n = 8, and lmx_sam_decode at n = 8

    python tools/sam_decoder_ab.py [--label WORD] [--out FILE] [--skip-profiler]
"""
import argparse
import csv
import glob
import hashlib
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lmx import kernels as K  # noqa: E402
from lmx import native, sam, sam_decoder, weights  # noqa: E402

PLANS = ("f16", "exact")
SIZES = ((96, 160), (64, 64))
CASES = ("predict box", "decode points", "decode points+box+mask", "decode multimask")


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def models(dev):
    cfg = sam.SamVitConfig(hidden=192, heads=3, layers=2, mlp=384, global_idx=(1,))
    enc = sam.SamVitEncoder(cfg, weights.synth_state_dict(sam.vit_param_spec(cfg), 5), dev)
    sd = sam_decoder.synthetic_state_dict(6)
    sd.update(weights.synth_state_dict(sam_decoder.mask_embed_param_spec(), 7))
    return enc, sam_decoder.MaskDecoder(sd, dev)


def prompts(h, w, n, dev):
    """boxes f32 [n,4], points f32 [n,2,2], labels int32 [n,2], mask_input f32 [n,256,256]: seeded, inside the frame"""
    from test_gpu_native_sam import make_boxes

    rng = np.random.default_rng(100 * h + w)
    pts = (rng.random((n, 2, 2)) * np.array([w, h])).astype(np.float32)
    lab = np.tile(np.array([1, 0], np.int32), (n, 1))
    mk = rng.standard_normal((n, 256, 256)).astype(np.float32) * 4
    return tuple(torch.from_numpy(a).to(dev) for a in (make_boxes(h, w, n), pts, lab, mk))


def run_case(dec, case, emb, hw, rhw, plan, boxes, pts, lab, mk):
    if case == "predict box":
        return dec.predict(emb, boxes, hw, rhw, plan)
    if case == "decode points":
        return dec.decode(emb, hw, rhw, points=pts, labels=lab, precision=plan)
    if case == "decode points+box+mask":
        return dec.decode(emb, hw, rhw, points=pts, labels=lab, boxes=boxes, mask_input=mk, precision=plan)
    return dec.decode(emb, hw, rhw, points=pts, labels=lab, multimask=True, precision=plan)


def frames_of(h, w, n, dev):
    from test_gpu_native_sam import make_frames

    return torch.from_numpy(make_frames(h, w, n)).to(dev)


def native_decode_once(plan):
    """the child under the profiler: one lmx_sam_decode of 3 frames' embeddings, nothing else of this library on the device"""
    dev = torch.device("cuda:0")
    enc, dec = models("cpu")
    h, w = SIZES[0]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s64.lmx")
        native.write_sam_image(enc, dec, path, (plan,))
        with native.NativeSam(path, 3, dev) as ns:
            ns.prepare(h, w, plan)
            emb = torch.zeros((3, 64, 64, 256), dtype=torch.float32 if plan == "exact" else torch.float16, device=dev)
            boxes = prompts(h, w, 3, dev)[0]
            ns.decode(emb, boxes, (h, w), plan)
            torch.cuda.synchronize(dev)


def profiled_kernels(plan):
    """-> (kernel names of the child in start order, those of torch left out) or a string saying why there are none"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return "rocprofv3 is not on PATH"
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--native-decode", plan]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return f"rocprofv3 ended with {r.returncode} and {len(files)} trace files: {r.stdout[-300:]!r}"
        rows = []
        for f in files:
            with open(f, newline="") as fh:
                rows += list(csv.DictReader(fh))
        rows.sort(key=lambda r_: int(r_["Start_Timestamp"]))
        return [r_["Kernel_Name"] for r_ in rows if "at::native" not in r_["Kernel_Name"]]


def event_median(fn, dev, warmup=10, calls=50):
    ms = []
    for i in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--skip-profiler", action="store_true")
    ap.add_argument("--label", default="", help="a word for the report's first line, such as 'parent, run 1'")
    ap.add_argument("--native-decode", choices=PLANS, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sam_decoder_ab: needs a GPU")
    if a.native_decode:
        return native_decode_once(a.native_decode)
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    say(f"== sam_decoder_ab {a.label}: {head or 'an unversioned tree'} on {torch.cuda.get_device_name(dev)}")
    enc, dec = models(dev)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s64.lmx")
        native.write_sam_image(enc, dec, path, PLANS)
        say("-- 1 bits: sha256[:16] of lowres, iou (MaskDecoder) and of every output (NativeSam.segment), n = 3")
        all_bits = []
        with native.NativeSam(path, 3, dev) as ns:
            for plan in PLANS:
                for h, w in SIZES:
                    frames, rhw = frames_of(h, w, 3, dev), sam.resize_longest_side(h, w, 1024)
                    emb = enc.encode(frames, plan)["fpn"][2].view(-1, 256)
                    p = prompts(h, w, 3, dev)
                    for case in CASES:
                        d = run_case(dec, case, emb, (h, w), rhw, plan, *p)
                        all_bits.append((digest(d["lowres"]), digest(d["iou"])))
                        say(f"{plan:5s} {h}x{w:<4d} {case:24s} lowres {all_bits[-1][0]} iou {all_bits[-1][1]}")
                    got = ns.segment(frames, p[0], plan)
                    all_bits.append(tuple((k, digest(got[k])) for k in sorted(got)))
                    say(f"{plan:5s} {h}x{w:<4d} {'NativeSam.segment':24s} " + " ".join(f"{k} {v}" for k, v in all_bits[-1]))
        say(f"bits digest {hashlib.sha256(repr(all_bits).encode()).hexdigest()[:16]}")

        say("-- 3 time: median [quartiles] ms of 50 calls after 10 warm-ups, device events, n = 8, 96x160")
        n, (h, w) = 8, SIZES[0]
        rhw = sam.resize_longest_side(h, w, 1024)
        p = prompts(h, w, n, dev)
        frames = frames_of(h, w, n, dev)
        with native.NativeSam(path, n, dev) as ns:
            for plan in PLANS:
                emb4 = enc.encode(frames, plan)["fpn"][2]
                emb = emb4.view(-1, 256)
                for case in CASES:
                    m, lo, hi = event_median(lambda: run_case(dec, case, emb, (h, w), rhw, plan, *p), dev)
                    say(f"{plan:5s} {case:24s} {m:8.3f}  [{lo:.3f} .. {hi:.3f}]")
                ns.prepare(h, w, plan)
                m, lo, hi = event_median(lambda: ns.decode(emb4, p[0], (h, w), plan), dev)
                say(f"{plan:5s} {'lmx_sam_decode':24s} {m:8.3f}  [{lo:.3f} .. {hi:.3f}]")
        # (last: the launch trace leaves a proxy in front of every lmx_k_* call, which the timed calls above should not pay for)
        say("-- 2 launch order: (class, key) of lmx.kernels' launch trace around predict + decode(multimask, mask_input), n = 3, 96x160")
        h, w = SIZES[0]
        rhw, p = sam.resize_longest_side(h, w, 1024), prompts(h, w, 3, dev)
        for plan in PLANS:
            emb = enc.encode(frames_of(h, w, 3, dev), plan)["fpn"][2].view(-1, 256)
            K.start_launch_trace()
            dec.predict(emb, p[0], (h, w), rhw, plan)
            dec.decode(emb, (h, w), rhw, points=p[1], labels=p[2], mask_input=p[3], multimask=True, precision=plan)
            order = [(cls, key) for cls, key, *_ in K.LAUNCH_TRACE]
            K.stop_launch_trace()
            say(f"{plan:5s} python: {len(order)} launches, sha256 {hashlib.sha256(repr(order).encode()).hexdigest()[:16]}")
            for i, o in enumerate(order):
                say(f"    {i:3d} {o[0]} {o[1]}")
        for plan in PLANS:
            names = "skipped (--skip-profiler)" if a.skip_profiler else profiled_kernels(plan)
            if isinstance(names, str):
                say(f"{plan:5s} lmx_sam_decode kernel names: none, {names}; the torch.equal suites (tests/test_gpu_native_sam.py) stand in")
                continue
            say(f"{plan:5s} lmx_sam_decode (+ prepare): {len(names)} kernels, sha256 {hashlib.sha256(repr(names).encode()).hexdigest()[:16]}")
            for i, name in enumerate(names):
                say(f"    {i:3d} {name[:150]}")

    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
