"""A/B of the fused step through the C API against the Python path, one job, one MI355X (profiles/native_fused_ab.txt).

  python tools/native_fused_ab.py [--frames 150] [--steps 20] [--warmup 5] [--sam-chunk 30] [--out profiles/native_fused_ab.txt]

The workload is bench.py's dense step: a synthetic 150-frame 1080p clip, YOLOv8-l, Hiera-B+ and DINOv3 ViT-L/16 with synthetic weights,
the f16 plans, SAM passes of 30 frames.  Python leg: FusedExtractor.step + lmx.dist.pack_records + the copy into pinned host memory.
C leg: NativeFused.step (lmx_fused_step, five lanes, seven streams) + the same copy.  The legs alternate step by step, each step ends
with a device synchronisation (the C handle allows one step in flight), and the figure is the median over --steps steps after --warmup.
The record kernel alone (lmx_k_pack_records) is timed against the torch packing it replaces on the same dict, with HIP events."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sam-chunk", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_fused_ab.txt"))
    args = ap.parse_args()

    import torch

    from lmx import dist, native, pipeline, synth
    from lmx import kernels as K

    dev = torch.device("cuda:0")
    fx = pipeline.FusedExtractor(dev)
    frames = torch.from_numpy(synth.synth_clip(100, args.frames)).to(dev)
    n_pass = -(-args.frames // args.sam_chunk)
    lanes = max(1, min(n_pass, fx.max_streams - 2))
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"{k}.lmx") for k in ("yolo", "sam", "dino")]
        native.write_yolo_image(fx.yolo, paths[0], ("f16",))
        native.write_sam_image(fx.sam, fx.decoder, paths[1], ("f16",))
        native.write_dino_image(fx.dino, paths[2])
        nf = native.NativeFused(*paths, args.frames, args.sam_chunk, sam_lanes=lanes, max_streams=fx.max_streams, device=dev)
    nf.prepare(1080, 1920, "f16")
    pinned = {}

    def to_host(buf):
        key = tuple(buf.shape)
        if key not in pinned:
            pinned[key] = torch.empty(buf.shape, dtype=torch.uint8).pin_memory()
        pinned[key].copy_(buf, non_blocking=True)
        return pinned[key]

    def python_step():
        out = fx.step(frames, sam_chunk=args.sam_chunk, precision="f16")
        out.pop("mask", None)
        buf, _ = dist.pack_records(out)
        return to_host(buf), out

    def c_step():
        buf, _ = nf.step(frames, "f16", conf=0.5)
        return to_host(buf), None

    times = {"python": [], "c": []}
    same = None
    for i in range(args.warmup + args.steps):
        host = {}
        for name, step in (("python", python_step), ("c", c_step)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            h, out = step()
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            host[name] = h.clone()
            if out is not None:
                last = out
        same = bool(torch.equal(host["python"], host["c"]))

    def event_ms(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b))
        return statistics.median(ms[2:])

    out_buf = torch.empty_like(dist.pack_records(last)[0])
    torch_ms = event_ms(lambda: dist.pack_records(last), args.steps + 2)
    kernel_ms = event_ms(lambda: K.pack_records(last, out=out_buf), args.steps + 2)
    kernel_same = bool(torch.equal(out_buf, dist.pack_records(last)[0]))
    nbytes = out_buf.numel()
    nf.close()

    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (min(v), max(v)) for k, v in times.items()}
    lines = [
        f"# tools/native_fused_ab.py: {args.frames} frames of 1080 x 1920, YOLOv8-l + Hiera-B+ + DINOv3 ViT-L/16, f16 plans, sam_chunk {args.sam_chunk}, "
        f"{lanes} lanes / {fx.max_streams} streams; {torch.cuda.get_device_name(dev)}",
        f"# per step: the step, the records, the copy into pinned host memory, a device synchronisation; legs alternate; median of {args.steps} after {args.warmup} warm-up steps",
        f"python  FusedExtractor.step + dist.pack_records + D2H : {med['python']:8.2f} ms/step  ({args.frames / med['python'] * 1e3:7.1f} frames/s)  min {spread['python'][0]:.2f} max {spread['python'][1]:.2f}",
        f"c       NativeFused.step (lmx_fused_step) + D2H       : {med['c']:8.2f} ms/step  ({args.frames / med['c'] * 1e3:7.1f} frames/s)  min {spread['c'][0]:.2f} max {spread['c'][1]:.2f}",
        f"records of the two legs equal byte for byte           : {same}",
        f"# the record matrix alone ({nbytes} bytes), HIP events, median of {args.steps}",
        f"torch   dist.pack_records (zeros + a strided copy per field) : {torch_ms * 1e3:8.1f} us",
        f"kernel  lmx_k_pack_records (one launch)                      : {kernel_ms * 1e3:8.1f} us  ({2 * nbytes / kernel_ms / 1e6:6.1f} GB/s read + written)  equal: {kernel_same}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
