"""Decoder frames in: the YUV 4:2:0 -> BGR kernel against a copy of the same traffic, and the fused step from rawvideo against the fused
step from BGR, one job, one MI355X (profiles/yuv_ingest.txt).

  python tools/yuv_ingest_probe.py [--frames 150] [--launches 20] [--steps 10] [--sam-chunk 30] [--no-host-path] [--out profiles/yuv_ingest.txt]

Kernel: lmx_k_yuv420_to_bgr on --frames frames of 1080 x 1920, NV12 pitched to 2048 bytes and I420 tight, HIP events around each of
--launches launches after 3 warm-up launches; bytes/s over the algorithmic 4.5 B/px (1.5 read, 3 written).  The yardstick is a torch
device-to-device copy_ of 2.25 n h w bytes — the same total traffic — timed the same way, the three alternating launch by launch.
Host path: NativeFused.step_yuv_host (rawvideo NV12, 1.5 B/px uploaded) against NativeFused.step_host (the BGR frames the kernel makes of
the same bytes, 3 B/px uploaded) with bench.py's models (YOLOv8-l, Hiera-B+, DINOv3 ViT-L/16, synthetic weights, f16 plans), alternating,
median of --steps steps after 2 warm-up steps each; the upload alone (pageable host memory, as the C call copies it) apart."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"))

H, W, PITCH = 1080, 1920, 2048


def bgr_to_nv12(frames):
    """u8 BGR [n,h,w,3] on the device -> rawvideo NV12 u8 [n, h * 3 / 2, w]: BT.601 studio swing in integers, chroma of the top-left
    pixel of each 2 x 2 block.  Torch arithmetic, set-up only: the probe needs decoder-shaped bytes of a real clip, not an inverse."""
    import torch

    f = frames.to(torch.int32)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16).clamp(0, 255)
    u = (((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128).clamp(0, 255)[:, 0::2, 0::2]
    v = (((112 * r - 94 * g - 18 * b + 128) >> 8) + 128).clamp(0, 255)[:, 0::2, 0::2]
    n, h, w = y.shape
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device=frames.device)
    out[:, :h] = y.to(torch.uint8)
    c = out[:, h:].view(n, h // 2, w // 2, 2)
    c[..., 0] = u.to(torch.uint8)
    c[..., 1] = v.to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sam-chunk", type=int, default=30)
    ap.add_argument("--no-host-path", action="store_true", help="the kernel table alone (a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_ingest.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from lmx import kernels as K
    from lmx import native, pipeline, synth

    dev = torch.device("cuda:0")
    n = args.frames
    px = n * H * W

    # ---- the clip as a decoder would leave it: tight NV12 in chunks of 10 frames (the int32 intermediates of the set-up are large)
    clip = synth.synth_clip(100, n)
    nv12 = torch.cat([bgr_to_nv12(torch.from_numpy(clip[i:i + 10]).to(dev)) for i in range(0, n, 10)])
    del clip
    luma = nv12[:, :H]
    # NV12 surfaces pitched to 2048, luma and chroma allocations apart
    sy = torch.zeros((n, H, PITCH), dtype=torch.uint8, device=dev)
    sc = torch.zeros((n, H // 2, PITCH), dtype=torch.uint8, device=dev)
    sy[:, :, :W] = luma
    sc[:, :, :W] = nv12[:, H:]
    # I420 tight planes
    iy = luma.contiguous()
    cc = nv12[:, H:].view(n, H // 2, W // 2, 2)
    iu, iv = cc[..., 0].contiguous(), cc[..., 1].contiguous()
    bgr = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    copy_src = torch.randint(0, 256, (px * 9 // 4,), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)

    legs = {
        "nv12 pitched 2048": lambda: K.yuv420_to_bgr(sy[:, :, :W], sc[:, :, :W], H, W, layout="nv12", matrix="bt709", out=bgr),
        "i420 tight": lambda: K.yuv420_to_bgr(iy, iu, H, W, layout="i420", matrix="bt709", v=iv, out=bgr),
        "torch copy_ of 2.25 B/px": lambda: copy_dst.copy_(copy_src),
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
    # the two layouts of the same clip give the same frames
    legs["nv12 pitched 2048"]()
    from_nv12 = bgr.clone()
    legs["i420 tight"]()
    torch.cuda.synchronize(dev)
    same_frames = bool(torch.equal(from_nv12, bgr))
    del from_nv12

    med = {k: statistics.median(v) for k, v in us.items()}
    base = med["torch copy_ of 2.25 B/px"]
    lines = [
        f"# tools/yuv_ingest_probe.py: {n} frames of {H} x {W}; {torch.cuda.get_device_name(dev)}",
        f"# 1. kernel: lmx_k_yuv420_to_bgr, HIP events around each launch, legs alternating, {args.launches} launches after 3 warm-up; "
        f"GB/s over the algorithmic 4.5 B/px = {4.5 * px / 1e6:.1f} MB (the copy moves the same bytes: 2.25 B/px read, 2.25 written)",
        f"{'leg':28s} {'median us':>10s} {'min':>9s} {'max':>9s} {'GB/s':>8s} {'x copy':>7s}",
    ]
    for name in legs:
        lines.append(f"{name:28s} {med[name]:10.1f} {min(us[name]):9.1f} {max(us[name]):9.1f} {4.5 * px / med[name] / 1e3:8.1f} {med[name] / base:7.2f}")
    lines.append(f"expectation to report against: within 1.5 x of the copy; NV12 {med['nv12 pitched 2048'] / base:.2f} x, I420 {med['i420 tight'] / base:.2f} x")
    lines.append(f"BGR frames from the NV12 surfaces and from the I420 planes of the same clip equal: {same_frames}")

    if not args.no_host_path:
        del sy, sc, iy, iu, iv, copy_src, copy_dst
        fx = pipeline.FusedExtractor(dev)
        n_pass = -(-n // args.sam_chunk)
        lanes = max(1, min(n_pass, fx.max_streams - 2))
        with tempfile.TemporaryDirectory() as tmp:
            paths = [os.path.join(tmp, f"{k}.lmx") for k in ("yolo", "sam", "dino")]
            native.write_yolo_image(fx.yolo, paths[0], ("f16",))
            native.write_sam_image(fx.sam, fx.decoder, paths[1], ("f16",))
            native.write_dino_image(fx.dino, paths[2])
            nf = native.NativeFused(*paths, n, args.sam_chunk, sam_lanes=lanes, max_streams=fx.max_streams, device=dev)
        del fx
        nf.prepare(H, W, "f16")
        yuv_host = nv12.cpu().numpy()
        bgr_host = K.yuv420_to_bgr(nv12[:, :H], nv12[:, H:], H, W, layout="nv12", matrix="bt601").cpu().numpy()
        del nv12, bgr
        steps = {"step_host (BGR, 3 B/px up)": lambda: nf.step_host(bgr_host, "f16", conf=0.5)[0],
                 "step_yuv_host (NV12, 1.5 B/px up)": lambda: nf.step_yuv_host(yuv_host, "f16", layout="nv12", matrix="bt601", conf=0.5)[0]}
        ms = {k: [] for k in steps}
        rec = {}
        for i in range(2 + args.steps):
            for name, fn in steps.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rec[name] = fn()  # synchronous: uploads, steps, downloads, synchronises
                if i >= 2:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        same_records = bool(np.array_equal(*rec.values()))
        # the upload alone: one copy from pageable host memory, as the C calls do it
        up = {}
        for name, host in (("BGR", bgr_host), ("NV12", yuv_host)):
            dst = torch.empty(host.shape, dtype=torch.uint8, device=dev)
            src = torch.from_numpy(host)
            t = []
            for i in range(2 + args.steps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                dst.copy_(src)
                torch.cuda.synchronize(dev)
                if i >= 2:
                    t.append((time.perf_counter() - t0) * 1e3)
            up[name] = (statistics.median(t), host.nbytes)
            del dst
        nf.close()
        lines.append(f"# 2. host path: bench.py's models (YOLOv8-l, Hiera-B+, DINOv3 ViT-L/16, f16 plans), sam_chunk {args.sam_chunk}, {lanes} lanes; host clock around "
                     f"the synchronous call, legs alternating, median of {args.steps} after 2 warm-up steps; reported, not gated")
        for name in steps:
            m = statistics.median(ms[name])
            lines.append(f"{name:36s} {m:8.2f} ms/step ({n / m * 1e3:7.1f} frames/s)  min {min(ms[name]):.2f} max {max(ms[name]):.2f}")
        for name, (m, nb) in up.items():
            lines.append(f"H2D copy alone, {name:4s} {nb / 1e6:8.1f} MB from pageable memory : {m:8.2f} ms ({nb / m / 1e6:6.1f} GB/s)")
        lines.append(f"records of the two legs equal byte for byte: {same_records}")

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
