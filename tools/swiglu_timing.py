"""fc1 of a gated MLP, fused against unfused, timed with HIP events (profiles/r04_swiglu_fc1.txt).

  fused    one lmx_k_gemm launch with the LMX_ACT_SWIGLU epilogue: writes I f16 columns per row
  unfused  lmx_k_gemm (no activation) to a 2I-wide f16 buffer + lmx_k_swiglu: writes 2I, reads 2I, writes I

Default shape: DINOv3 ViT-H+/16 (K = 1280, N = 2I = 10240) at 8 and 256 frames of 201 tokens.  The two forms alternate inside
one process, `--reps` timed pairs after `--warmup` untimed ones; median and min / max per form.  TFLOP/s counts the GEMM's
2 M N K only, against the 2.5 PFLOP/s dense f16 peak.

  python tools/swiglu_timing.py [--K 1280 --N 10240 --M 1608 51456 --reps 30 --warmup 5 --out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd")]

from lmx import dino  # noqa: E402
from lmx import kernels as K  # noqa: E402

PEAK = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1280)
    ap.add_argument("--N", type=int, default=10240)
    ap.add_argument("--M", type=int, nargs="+", default=[8 * 201, 256 * 201])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Kd, N, I = a.K, a.N, a.N // 2
    r = np.random.default_rng(0)
    wg = (r.standard_normal((I, Kd)) * Kd ** -0.5).astype(np.float16)
    wu = (r.standard_normal((I, Kd)) * Kd ** -0.5).astype(np.float16)
    b = r.standard_normal(N).astype(np.float32)
    w_packed = torch.from_numpy(dino.pack_gated(wg, wu)).to(dev)
    b_packed = torch.from_numpy(dino.pack_gated(b[:I], b[I:])).to(dev)
    w_plain, b_plain = torch.from_numpy(np.concatenate([wg, wu], 0)).to(dev), torch.from_numpy(b).to(dev)
    lines = [f"fc1 of a gated MLP, K={Kd} N={N} (I={I}); {a.reps} alternating timed pairs after {a.warmup} warm-up pairs; HIP events; us",
             f"device: {torch.cuda.get_device_name(0)}",
             f"{'M':>7} {'form':<8} {'median':>9} {'min':>9} {'max':>9} {'TFLOP/s':>8} {'of peak':>8}"]
    for M in a.M:
        x = torch.from_numpy(r.standard_normal((M, Kd)).astype(np.float16)).to(dev)
        out_f = torch.empty((M, I), dtype=torch.float16, device=dev)
        out_u = torch.empty((M, I), dtype=torch.float16, device=dev)
        wide = torch.empty((M, N), dtype=torch.float16, device=dev)

        def fused():
            K.gemm(x, w_packed, bias=b_packed, act=K.ACT_SWIGLU, out=out_f)

        def unfused():
            K.gemm(x, w_plain, bias=b_plain, out=wide)
            K.swiglu(wide, out=out_u)

        t = {"fused": [], "unfused": []}
        for i in range(a.warmup + a.reps):
            for name, fn in (("fused", fused), ("unfused", unfused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    t[name].append(e0.elapsed_time(e1) * 1e3)
        # the unfused form rounds gate and up to f16 first: the two agree to that rounding, not bit for bit
        d = (out_f.float() - out_u.float()).abs()
        rel = float((d / (out_u.float().abs() + 1e-3)).max())
        for name in ("fused", "unfused"):
            med = statistics.median(t[name])
            tf = 2.0 * M * N * Kd / (med * 1e-6) / 1e12
            lines.append(f"{M:>7} {name:<8} {med:>9.1f} {min(t[name]):>9.1f} {max(t[name]):>9.1f} {tf:>8.1f} {100 * tf * 1e12 / PEAK:>7.1f}%")
        mf, mu = statistics.median(t["fused"]), statistics.median(t["unfused"])
        lines.append(f"{M:>7} fused / unfused = {mf / mu:.3f}   (max |fused - unfused| / (|unfused| + 1e-3) = {rel:.2e})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
