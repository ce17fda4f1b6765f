"""Timing of the TCN gait model: lmx.tcn.TcnScorer.score (ONE launch for n clips x 10 MC-dropout samples, csrc/tcn.hip) against the
same network in float32 through PyTorch-ROCm on the same GPU, run the way services/tcn-pipeline/app/main.py:169-195 runs it: ten eager
train-mode forwards, one after the other (clips batched for the n = 256 row).  That torch run is what the kernel's time is set against.

HIP-event times; every shape is warmed up first; the two sides alternate inside each round and the table gives the median over the
rounds with the spread.  FLOPs are counted from the shapes (2 T K N per convolution with K = taps x inputs, and the head).

    python tools/tcn_ab.py [--rounds 7] [--out profiles/tcn_ab.txt]"""
import statistics

import torch
import torch.nn.functional as F

import gait_ab as G

import tcnref  # noqa: E402
from lmx import checkpoints, tcn  # noqa: E402

T, S = 125, 10


def flops_per_pass(cfg, steps):
    total = 0
    for i, n in enumerate(cfg.channels):
        cin = cfg.block_inputs(i)
        total += 2 * steps * n * cfg.kernel_size * (cin + n) + (2 * steps * n * cin if cin != n else 0)
    return total + 2 * cfg.channels[-1] * cfg.head + 2 * cfg.head


def main():
    args = G.parse_args("tcn_ab")
    dev = torch.device("cuda:0")
    cfg = tcnref.SHIPPED
    _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 1), cfg.dropout)
    scorer = tcn.TcnScorer(cfg, folded, device=dev)
    dev_folded = {k: v.to(dev) for k, v in folded.items()}

    def torch_score(x):
        """predict_with_uncertainty: ten train-mode forwards, stack, mean, unbiased std"""
        with torch.no_grad():
            preds = torch.stack([tcnref.forward(cfg, dev_folded, x, lambda v, site: F.dropout(v, cfg.dropout, True), torch.float32)[1]
                                 for _ in range(S)], 0)
            return preds.mean(0), preds.std(0)

    rows = {}
    for n, iters_lmx, iters_torch in ((1, 200, 10), (256, 50, 10)):
        x = torch.randn((n, T, cfg.input_dim), generator=torch.Generator().manual_seed(n)).to(dev)
        seeds = list(range(1, n + 1))
        rows[n] = G.alternate([(lambda: scorer.score(x, seeds, S), iters_lmx), (lambda: torch_score(x), iters_torch)], args.rounds)

    # the same grid of 2560 workgroups in eval mode: what the launch costs without the keep bits
    xe = torch.randn((256 * S, T, cfg.input_dim), generator=torch.Generator().manual_seed(3)).to(dev)
    ev, = G.alternate([(lambda: scorer.score(xe, None, 0), 50)], args.rounds)

    cus, mhz, where = G.device(dev, args.rounds)
    fl = flops_per_pass(cfg, T)
    lines = [f"TCN gait model, shipped configuration (44 -> 4 x 64, k = 3, head 32), clips of {T} steps, S = {S} samples; {where}",
             f"FLOPs per (clip, sample): {fl / 1e6:.2f} M",
             f"{'n':>4}  {'lmx one launch, ms':>28}  {'torch eager 10 forwards, ms':>30}  {'ratio':>7}  {'lmx clips/s':>12}  {'lmx TFLOP/s':>11}"]
    for n, (a, b) in rows.items():
        ma, mb = statistics.median(a), statistics.median(b)
        lines.append(f"{n:>4}  {G.cell(a, 10, 4)}  {G.cell(b, 10, 3)}  {mb / ma:>7.1f}  {n / ma * 1e3:>12.0f}  {n * S * fl / ma / 1e9:>11.2f}")
    bound_ms, derivation = G.bound(256 * S * fl, cus, mhz)
    lines.append(f"f32 MFMA bound for n = 256: {derivation}; measured / bound = {statistics.median(rows[256][0]) / bound_ms:.2f}")
    lines.append(f"eval mode, n = {256 * S} (the same {256 * S} workgroups, no keep bits): {statistics.median(ev):.4f} ms [{min(ev):.4f} .. {max(ev):.4f}]; / bound = {statistics.median(ev) / bound_ms:.2f}")
    G.write(args.out, lines)


if __name__ == "__main__":
    main()
