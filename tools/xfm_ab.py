"""Timing of the gait transformer: lmx.xfm.XfmScorer (ONE launch for n clips x 10 MC-dropout samples with the confidence mask, and one
eval-mode launch for the saliency; csrc/xfm.hip) against the same network in float32 through PyTorch-ROCm on the same GPU, run the way
services/transformer-pipeline/app/main.py:196-237 and :426-441 run it: ten eager train-mode forwards one after the other, then the
eval-mode forward that reads the attention weights (clips batched for the n = 256 row).  That torch run is what the kernel's time is set
against.

HIP-event times; every shape is warmed up first; the two sides alternate inside each round and the table gives the median over the
rounds with the spread.  FLOPs are counted from the shapes (2 T K N per linear layer, 4 T T D for the scores and P.V of a layer).

    python tools/xfm_ab.py [--rounds 7] [--out profiles/xfm_ab.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import xfmref  # noqa: E402
from lmx import checkpoints, xfm  # noqa: E402

T, S = 125, 10
F32_MFMA_FLOP_PER_CLK_PER_CU = 256  # 64 per SIMD (v_mfma_f32_16x16x4_f32: 2048 FLOP per 32 cycles), 4 SIMDs


def flops_per_pass(cfg, steps):
    D = cfg.d_model
    layer = 2 * steps * D * 3 * D + 4 * steps * steps * D + 2 * steps * D * D + 4 * steps * D * cfg.ff
    return 2 * steps * cfg.input_dim * D + cfg.n_layers * layer + 2 * D * cfg.head + 2 * cfg.head


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xfm_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "xfm_ab needs a GPU"
    dev = torch.device("cuda:0")
    cfg = xfmref.SHIPPED
    _, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(cfg, 1), n_heads=cfg.n_heads, dropout=cfg.dropout)
    scorer = xfm.XfmScorer(cfg, w, device=dev)
    dev_w = {k: v.to(dev) for k, v in w.items()}

    def torch_score(x, mask):
        """predict_with_uncertainty (ten train-mode forwards, stack, mean, unbiased std), then the eval forward for the weights"""
        with torch.no_grad():
            preds = torch.stack([xfmref.forward(cfg, dev_w, x, mask, lambda v, site: F.dropout(v, cfg.dropout, True), torch.float32)[1]
                                 for _ in range(S)], 0)
            return preds.mean(0), preds.std(0), xfmref.forward(cfg, dev_w, x, None, None, torch.float32)[2]

    rows = {}
    for n, iters_lmx, iters_torch in ((1, 100, 5), (256, 20, 5)):
        g = torch.Generator().manual_seed(n)
        x = torch.randn((n, T, cfg.input_dim), generator=g).to(dev)
        mask = xfmref.make_masks(n, T, g).to(dev)
        mask8, seeds = mask.to(torch.uint8), list(range(1, n + 1))
        train_fn = lambda: scorer.score(x, mask8, seeds, S)  # noqa: E731
        lmx_fn = lambda: (scorer.score(x, mask8, seeds, S), scorer.saliency(x))  # noqa: E731
        torch_fn = lambda: torch_score(x, mask)  # noqa: E731
        for fn in (train_fn, lmx_fn, torch_fn):  # warm-up of every side at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a, b, c = [], [], []
        for _ in range(args.rounds):
            a.append(timed(lmx_fn, iters_lmx))
            b.append(timed(torch_fn, iters_torch))
            c.append(timed(train_fn, iters_lmx))
        rows[n] = (a, b, c)

    # the same grid of 2560 workgroups in eval mode: what the launch costs without the keep bits
    xe = torch.randn((256 * S, T, cfg.input_dim), generator=torch.Generator().manual_seed(3)).to(dev)
    eval_fn = lambda: scorer.score(xe, None, None, 0)  # noqa: E731
    for _ in range(3):
        eval_fn()
    torch.cuda.synchronize()
    ev = [timed(eval_fn, 20) for _ in range(args.rounds)]

    props = torch.cuda.get_device_properties(dev)
    cus, mhz = props.multi_processor_count, getattr(props, "clock_rate", 2400000) / 1e3
    fl = flops_per_pass(cfg, T)
    lines = [f"Gait transformer, shipped configuration (44 -> d_model 64, 4 heads, 4 layers, FF 256, head 32), clips of {T} steps, S = {S} samples, "
             f"masked; {props.name}, {cus} CUs at up to {mhz:.0f} MHz; {args.rounds} alternating rounds, HIP events, median [min .. max]",
             f"FLOPs per (clip, sample): {fl / 1e6:.2f} M",
             f"{'n':>4}  {'lmx S = 10 + eval launch, ms':>30}  {'torch eager 10 + 1 forwards, ms':>32}  {'ratio':>7}  {'lmx S = 10 launch alone, ms':>30}  "
             f"{'clips/s':>9}  {'TFLOP/s':>8}"]
    for n, (a, b, c) in rows.items():
        ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
        lines.append(f"{n:>4}  {ma:>12.4f} [{min(a):.4f} .. {max(a):.4f}]  {mb:>12.3f} [{min(b):.3f} .. {max(b):.3f}]  {mb / ma:>7.1f}  "
                     f"{mc:>12.4f} [{min(c):.4f} .. {max(c):.4f}]  {n / ma * 1e3:>9.0f}  {n * S * fl / mc / 1e9:>8.2f}")
    bound_ms = 256 * S * fl / (cus * F32_MFMA_FLOP_PER_CLK_PER_CU * mhz * 1e6) * 1e3
    lines.append(f"f32 MFMA bound for n = 256, S = 10: {256 * S * fl / 1e9:.1f} GFLOP at {cus} CUs x {F32_MFMA_FLOP_PER_CLK_PER_CU} FLOP/clk x {mhz:.0f} MHz "
                 f"= {bound_ms:.3f} ms; S = 10 launch / bound = {statistics.median(rows[256][2]) / bound_ms:.2f}")
    lines.append(f"eval mode, n = {256 * S} (the same {256 * S} workgroups, no keep bits, no mask): {statistics.median(ev):.4f} ms [{min(ev):.4f} .. {max(ev):.4f}]; "
                 f"/ bound = {statistics.median(ev) / bound_ms:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
