"""Per-frame blur / brightness sums: lmx_k_frame_quality against a copy of the same traffic, one job, one MI355X
(profiles/frame_quality.txt).

  python tools/frame_quality_probe.py [--frames 150] [--launches 20] [--out profiles/frame_quality.txt]

Kernel: lmx_k_frame_quality on --frames frames of 1080 x 1920 from lmx.synth, HIP events around each of --launches launches after 3
warm-up launches; bytes/s over the algorithmic 3 B/px (read once; 32 bytes per frame written).  The yardstick is a torch device-to-device
copy_ of 1.5 n h w bytes — 1.5 B/px read and 1.5 written, the same total traffic — timed the same way, the two alternating launch by
launch.  The expectation to report against is the one profiles/yuv_ingest.txt used for its kernel: within 1.5 x of the copy."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_quality.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import qualityref
    from lmx import kernels as K
    from lmx import synth

    dev = torch.device("cuda:0")
    n = args.frames
    px = n * H * W
    clip = synth.synth_clip(100, n)
    frames = torch.from_numpy(clip).to(dev)
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    copy_src = torch.randint(0, 256, (px * 3 // 2,), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)

    legs = {
        "frame_quality 1080p": lambda: K.frame_quality(frames, out=out),
        "torch copy_ of 1.5 B/px": lambda: copy_dst.copy_(copy_src),
    }
    us = {k: [] for k in legs}
    for i in range(3 + args.launches):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            if i >= 3:
                us[name].append(a.elapsed_time(b) * 1e3)
    # the sums the timed launches left are the reference's, on the first and the last frame
    got = out.cpu().numpy()
    exact = bool(np.array_equal(got[[0, n - 1]], qualityref.sums(clip[[0, n - 1]])))

    med = {k: statistics.median(v) for k, v in us.items()}
    base = med["torch copy_ of 1.5 B/px"]
    lines = [
        f"# tools/frame_quality_probe.py: {n} frames of {H} x {W}; {torch.cuda.get_device_name(dev)}",
        f"# lmx_k_frame_quality (memset of out + one kernel), HIP events around each launch, legs alternating, {args.launches} launches after 3 warm-up; "
        f"GB/s over the algorithmic 3 B/px = {3 * px / 1e6:.1f} MB (the copy moves the same bytes: 1.5 B/px read, 1.5 written)",
        f"{'leg':28s} {'median us':>10s} {'min':>9s} {'max':>9s} {'GB/s':>8s} {'x copy':>7s}",
    ]
    for name in legs:
        lines.append(f"{name:28s} {med[name]:10.1f} {min(us[name]):9.1f} {max(us[name]):9.1f} {3 * px / med[name] / 1e3:8.1f} {med[name] / base:7.2f}")
    ratio = med["frame_quality 1080p"] / base
    lines.append(f"expectation to report against: within 1.5 x of the copy; measured {ratio:.2f} x: {'met' if ratio <= 1.5 else 'MISSED'}")
    lines.append(f"sums of frames 0 and {n - 1} equal tests/qualityref.py: {exact}")

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
