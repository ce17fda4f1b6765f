"""What tools/tcn_ab.py and tools/xfm_ab.py share: the import path, the arguments, HIP-event timing of sides that alternate inside each
round, the f32 MFMA bound and the table cells."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

F32_MFMA_FLOP_PER_CLK_PER_CU = 256  # 64 per SIMD (v_mfma_f32_16x16x4_f32: 2048 FLOP per 32 cycles), 4 SIMDs


def parse_args(name):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"{name}.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), f"{name} needs a GPU"
    return args


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def alternate(sides, rounds):
    """sides: (fn, iters) each.  Every side is warmed up, then the sides take turns inside each round; one list of ms per call per side."""
    for fn, _ in sides:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in sides]
    for _ in range(rounds):
        for times, (fn, iters) in zip(out, sides):
            times.append(timed(fn, iters))
    return out


def cell(v, width, digits):
    """median [min .. max]"""
    return f"{statistics.median(v):>{width}.{digits}f} [{min(v):.{digits}f} .. {max(v):.{digits}f}]"


def device(dev, rounds):
    """(CUs, MHz, the end of the table's first line)"""
    props = torch.cuda.get_device_properties(dev)
    cus, mhz = props.multi_processor_count, getattr(props, "clock_rate", 2400000) / 1e3
    return cus, mhz, f"{props.name}, {cus} CUs at up to {mhz:.0f} MHz; {rounds} alternating rounds, HIP events, median [min .. max]"


def bound(flop, cus, mhz):
    """(ms at the f32 MFMA rate, its derivation for the table)"""
    ms = flop / (cus * F32_MFMA_FLOP_PER_CLK_PER_CU * mhz * 1e6) * 1e3
    return ms, f"{flop / 1e9:.1f} GFLOP at {cus} CUs x {F32_MFMA_FLOP_PER_CLK_PER_CU} FLOP/clk x {mhz:.0f} MHz = {ms:.3f} ms"


def write(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
