"""Frames to an encoder, and the crop in between: the BGR -> YUV 4:2:0 kernel and the window form of the YUV 4:2:0 -> BGR kernel against
copies of the same traffic, and the unchanged whole-frame kernel beside them, one job, one MI355X (profiles/yuv_egress.txt).

  python tools/yuv_egress_probe.py [--frames 150] [--launches 20] [--parent-lib PATH] [--out profiles/yuv_egress.txt]

The recipe of tools/yuv_ingest_probe.py: --frames frames of 1080 x 1920, HIP events around each of --launches launches after 3 warm-up
launches, all legs alternating launch by launch in one process; bytes/s over the algorithmic 4.5 B/px of what a leg converts.  Beside
the legs the bar is set for — BGR frames to NV12 and to I420, the 720p window at an odd (x, y), the unchanged whole-frame kernel — two
more say what the odd window costs: the same window on the source's block grid, and BGR -> NV12 from a window of the BGR frames.  The
yardsticks are torch device-to-device copy_ calls of 2.25 B/px — the same total traffic — for the whole frame and for the window.
--parent-lib: a liblmx.so built from the parent commit; its lmx_k_yuv420_to_bgr then runs as one more alternating leg (a second
library in the same process: its own code object, the same HIP runtime), which is how the whole-frame kernel is shown not to have moved."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, PITCH = 1080, 1920, 2048
ROI = (321, 181, 1280, 720)  # x, y, w, h: a 720p window at an odd position
ROI_ALIGNED = (320, 180, 1280, 720)  # the same window one pixel up and left: on the source's block grid, output rows 16-byte aligned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_egress.txt"))
    args = ap.parse_args()

    import torch

    from lmx import _lib, synth
    from lmx import kernels as K
    from yuv_ingest_probe import bgr_to_nv12

    dev = torch.device("cuda:0")
    n = args.frames
    px, wpx = n * H * W, n * ROI[2] * ROI[3]

    host_clip = synth.synth_clip(100, n)
    clip = torch.cat([torch.from_numpy(host_clip[i:i + 10]).to(dev) for i in range(0, n, 10)])  # BGR u8 [n,H,W,3]
    del host_clip
    nv12 = torch.cat([bgr_to_nv12(clip[i:i + 10]) for i in range(0, n, 10)])
    sy = torch.zeros((n, H, PITCH), dtype=torch.uint8, device=dev)
    sc = torch.zeros((n, H // 2, PITCH), dtype=torch.uint8, device=dev)
    sy[:, :, :W] = nv12[:, :H]
    sc[:, :, :W] = nv12[:, H:]
    del nv12
    # outputs: NV12 surfaces pitched to 2048, I420 tight planes, BGR frames and windows
    oy = torch.empty((n, H, PITCH), dtype=torch.uint8, device=dev)
    oc = torch.empty((n, H // 2, PITCH), dtype=torch.uint8, device=dev)
    iy = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    iu, iv = (torch.empty((n, H // 2, W // 2), dtype=torch.uint8, device=dev) for _ in range(2))
    bgr = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    win = torch.empty((n, ROI[3], ROI[2], 3), dtype=torch.uint8, device=dev)
    wy = torch.empty((n, ROI[3], ROI[2]), dtype=torch.uint8, device=dev)
    wc = torch.empty((n, ROI[3] // 2, ROI[2]), dtype=torch.uint8, device=dev)
    copy_src = torch.randint(0, 256, (px * 9 // 4,), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    x0, y0 = ROI[0], ROI[1]
    crop = clip[:, y0:y0 + ROI[3], x0:x0 + ROI[2]]  # a window of the BGR frames where it lies: rows at odd byte addresses

    # the whole-frame kernel through a prepared descriptor, so that this tree's library and the parent's are called the same way
    f, _, _ = K.yuv_frames(sy[:, :, :W], sc[:, :, :W], H, W, "nv12", "bt709")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def whole_frame_leg(lib):
        def leg():
            assert lib.lmx_k_yuv420_to_bgr(C.byref(f), n, H, W, C.c_void_p(bgr.data_ptr()), stream) == 0
        return leg

    legs = {
        "bgr -> nv12 pitched 2048": (px, lambda: K.bgr_to_yuv420(clip, "nv12", "bt709", out=(oy[:, :, :W], oc[:, :, :W]))),
        "bgr -> i420 tight": (px, lambda: K.bgr_to_yuv420(clip, "i420", "bt709", out=(iy, iu, iv))),
        "nv12 -> bgr, 720p window at odd x, y": (wpx, lambda: K.yuv420_to_bgr_roi(sy[:, :, :W], sc[:, :, :W], H, W, ROI, "nv12", "bt709", out=win)),
        "nv12 -> bgr, 720p window at (320, 180)": (wpx, lambda: K.yuv420_to_bgr_roi(sy[:, :, :W], sc[:, :, :W], H, W, ROI_ALIGNED, "nv12", "bt709", out=win)),
        "bgr 720p window at x = 321 -> nv12": (wpx, lambda: K.bgr_to_yuv420(crop, "nv12", "bt709", out=(wy, wc))),
        "nv12 -> bgr, whole frame (unchanged)": (px, whole_frame_leg(_lib.load())),
        "torch copy_ of 2.25 B/px, frame": (px, lambda: copy_dst.copy_(copy_src)),
        "torch copy_ of 2.25 B/px, window": (wpx, lambda: copy_dst[: wpx * 9 // 4].copy_(copy_src[: wpx * 9 // 4])),
    }
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib), mode=os.RTLD_NOW | os.RTLD_LOCAL)
        parent.lmx_k_yuv420_to_bgr.restype, parent.lmx_k_yuv420_to_bgr.argtypes = _lib.SIGNATURES["lmx_k_yuv420_to_bgr"]
        legs["nv12 -> bgr, whole frame, parent's library"] = (px, whole_frame_leg(parent))

    us = {k: [] for k in legs}
    for i in range(3 + args.launches):
        for name, (_, fn) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            if i >= 3:
                us[name].append(a.elapsed_time(b) * 1e3)

    # what the legs wrote: the window of the whole-frame conversion, and NV12 and I420 of the same frames
    legs["nv12 -> bgr, whole frame (unchanged)"][1]()
    legs["nv12 -> bgr, 720p window at odd x, y"][1]()
    legs["bgr -> nv12 pitched 2048"][1]()
    legs["bgr -> i420 tight"][1]()
    legs["bgr 720p window at x = 321 -> nv12"][1]()
    torch.cuda.synchronize(dev)
    same_window = bool(torch.equal(win, bgr[:, y0:y0 + ROI[3], x0:x0 + ROI[2]]))
    cc = oc[:, :, :W].reshape(n, H // 2, W // 2, 2)
    same_planes = bool(torch.equal(oy[:, :, :W], iy) and torch.equal(cc[..., 0], iu) and torch.equal(cc[..., 1], iv))
    wy2, wc2 = K.bgr_to_yuv420(crop.contiguous(), "nv12", "bt709")
    same_crop = bool(torch.equal(wy, wy2) and torch.equal(wc, wc2))

    med = {k: statistics.median(v) for k, v in us.items()}
    base = {px: med["torch copy_ of 2.25 B/px, frame"], wpx: med["torch copy_ of 2.25 B/px, window"]}
    lines = [
        f"# tools/yuv_egress_probe.py: {n} frames of {H} x {W}, window {ROI[2]} x {ROI[3]} at ({ROI[0]}, {ROI[1]}); {torch.cuda.get_device_name(dev)}",
        f"# HIP events around each launch, legs alternating, {args.launches} launches after 3 warm-up; GB/s over the algorithmic 4.5 B/px = "
        f"{4.5 * px / 1e6:.1f} MB (frame) / {4.5 * wpx / 1e6:.1f} MB (window); x copy: against the copy_ of the same traffic",
        f"{'leg':44s} {'median us':>10s} {'min':>9s} {'max':>9s} {'GB/s':>8s} {'x copy':>7s}",
    ]
    for name, (p, _) in legs.items():
        lines.append(f"{name:44s} {med[name]:10.1f} {min(us[name]):9.1f} {max(us[name]):9.1f} {4.5 * p / med[name] / 1e3:8.1f} {med[name] / base[p]:7.2f}")
    lines.append("expectation to report against: within 1.5 x of the copy of the same traffic")
    if args.parent_lib:
        a, b = med["nv12 -> bgr, whole frame (unchanged)"], med["nv12 -> bgr, whole frame, parent's library"]
        lines.append(f"whole-frame kernel, this tree against the parent's library: {a:.1f} us against {b:.1f} us ({(a - b) / b * 100:+.2f} %)")
    lines.append(f"the window equals the same window of the whole-frame conversion: {same_window}")
    lines.append(f"NV12 and I420 planes of the same frames hold the same bytes: {same_planes}")
    lines.append(f"NV12 of the BGR window where it lies equals NV12 of its contiguous copy: {same_crop}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
