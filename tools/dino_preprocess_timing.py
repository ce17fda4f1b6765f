"""Times the two DINO preprocessing paths on the same 150 synthetic 1080p frames with HIP events:
  float : lmx_k_float_resize_patchify (DINOv3ViTImageProcessor: rescale -> float32 antialiased bilinear 224 x 224 -> normalize)
  pil   : lmx_k_pil_resize_h + _v + lmx_k_patchify_norm (dinov2-base: bicubic shortest-edge 256 on u8, crop 224)
Output allocation is inside the timed region of both (it is part of the call).  Prints the median and the minimum of REPS
timed calls after WARM untimed ones, and the achieved GB/s = frame bytes / time.
    python tools/dino_preprocess_timing.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd")]

from lmx import dino, synth, weights  # noqa: E402

N, WARM, REPS = 150, 5, 30


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)  # us
    return statistics.median(ts), min(ts)


def main():
    dev = torch.device("cuda:0")
    base = np.stack([synth.synth_frame(1, i) for i in range(6)], 0)
    frames = torch.from_numpy(base).to(dev).repeat(N // 6, 1, 1, 1).contiguous()
    assert tuple(frames.shape) == (N, 1080, 1920, 3)
    nbytes = frames.numel()
    cfg = dino.DinoConfig(hidden=256, layers=1, heads=4, mlp=1024)
    sd = weights.synth_state_dict(dino.param_spec(cfg), 1)
    import dataclasses

    pil = dino.DinoEmbedder(cfg, sd, dev)
    flt = dino.DinoEmbedder(dataclasses.replace(cfg, preproc=dino.DinoPreprocess(kind="float", filt="bilinear", shortest_edge=None,
                                                                                   size_hw=(224, 224), crop=None)), sd, dev)
    lines = [f"{N} frames 1080x1920x3 u8 = {nbytes / 1e6:.1f} MB in, {N * 196 * 768 * 2 / 1e6:.1f} MB f16 patch matrix out; "
             f"HIP events, {WARM} warm-up + {REPS} timed calls, {torch.cuda.get_device_name(0)}"]
    for name, m in (("float (lmx_k_float_resize_patchify)", flt), ("pil   (pil_resize_h + pil_resize_v + patchify_norm)", pil)):
        med, best = timed(lambda m=m: m.preprocess(frames))
        lines.append(f"{name:55s} median {med:8.1f} us  min {best:8.1f} us  {nbytes / med / 1e3:7.1f} GB/s of frame bytes (median)")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
