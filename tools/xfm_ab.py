"""Timing of the gait transformer: lmx.xfm.XfmScorer (ONE launch for n clips x 10 MC-dropout samples with the confidence mask, and one
eval-mode launch for the saliency; csrc/xfm.hip) against the same network in float32 through PyTorch-ROCm on the same GPU, run the way
services/transformer-pipeline/app/main.py:196-237 and :426-441 run it: ten eager train-mode forwards one after the other, then the
eval-mode forward that reads the attention weights (clips batched for the n = 256 row).  That torch run is what the kernel's time is set
against.

HIP-event times; every shape is warmed up first; the two sides alternate inside each round and the table gives the median over the
rounds with the spread.  FLOPs are counted from the shapes (2 T K N per linear layer, 4 T T D for the scores and P.V of a layer).

    python tools/xfm_ab.py [--rounds 7] [--out profiles/xfm_ab.txt]"""
import statistics

import torch
import torch.nn.functional as F

import gait_ab as G

import xfmref  # noqa: E402
from lmx import checkpoints, xfm  # noqa: E402

T, S = 125, 10


def flops_per_pass(cfg, steps):
    D = cfg.d_model
    layer = 2 * steps * D * 3 * D + 4 * steps * steps * D + 2 * steps * D * D + 4 * steps * D * cfg.ff
    return 2 * steps * cfg.input_dim * D + cfg.n_layers * layer + 2 * D * cfg.head + 2 * cfg.head


def main():
    args = G.parse_args("xfm_ab")
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
        rows[n] = G.alternate([(lambda: (scorer.score(x, mask8, seeds, S), scorer.saliency(x)), iters_lmx), (lambda: torch_score(x, mask), iters_torch),
                               (lambda: scorer.score(x, mask8, seeds, S), iters_lmx)], args.rounds)

    # the same grid of 2560 workgroups in eval mode: what the launch costs without the keep bits
    xe = torch.randn((256 * S, T, cfg.input_dim), generator=torch.Generator().manual_seed(3)).to(dev)
    ev, = G.alternate([(lambda: scorer.score(xe, None, None, 0), 20)], args.rounds)

    cus, mhz, where = G.device(dev, args.rounds)
    fl = flops_per_pass(cfg, T)
    lines = [f"Gait transformer, shipped configuration (44 -> d_model 64, 4 heads, 4 layers, FF 256, head 32), clips of {T} steps, S = {S} samples, "
             f"masked; {where}",
             f"FLOPs per (clip, sample): {fl / 1e6:.2f} M",
             f"{'n':>4}  {'lmx S = 10 + eval launch, ms':>30}  {'torch eager 10 + 1 forwards, ms':>32}  {'ratio':>7}  {'lmx S = 10 launch alone, ms':>30}  "
             f"{'clips/s':>9}  {'TFLOP/s':>8}"]
    for n, (a, b, c) in rows.items():
        ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
        lines.append(f"{n:>4}  {G.cell(a, 12, 4)}  {G.cell(b, 12, 3)}  {mb / ma:>7.1f}  {G.cell(c, 12, 4)}  {n / ma * 1e3:>9.0f}  {n * S * fl / mc / 1e9:>8.2f}")
    bound_ms, derivation = G.bound(256 * S * fl, cus, mhz)
    lines.append(f"f32 MFMA bound for n = 256, S = 10: {derivation}; S = 10 launch / bound = {statistics.median(rows[256][2]) / bound_ms:.2f}")
    lines.append(f"eval mode, n = {256 * S} (the same {256 * S} workgroups, no keep bits, no mask): {statistics.median(ev):.4f} ms [{min(ev):.4f} .. {max(ev):.4f}]; / bound = {statistics.median(ev) / bound_ms:.2f}")
    G.write(args.out, lines)


if __name__ == "__main__":
    main()
