"""Timing of the graph transformer: lmx.gfm.GfmScorer (the bias kernel and ONE launch for n graphs x 10 MC-dropout samples, then the
same pair in eval mode for node scores and the attention column; csrc/gfm.hip) against the same network in float32 through PyTorch-ROCm
on the same GPU, run the way services/graph-transformer-pipeline runs it: ten eager train-mode forwards one after the other
(predict_with_uncertainty), then the eval-mode forward, graph after graph — tests/gfmref.py with F.dropout, which is the reference's
network minus its networkx shortest paths on the host (the restatement reads the prepared idx matrix, so the torch side is favoured).

HIP-event times; every shape is warmed up first; the two sides alternate inside each round and the table gives the median over the
rounds with the spread.  FLOPs are counted from the shapes (2 R K N per linear layer over R rows, 4 R R D for the scores and P.V).

    python tools/gfm_ab.py [--rounds 7] [--out profiles/gfm_ab.txt]"""
import statistics

import torch
import torch.nn.functional as F

import graph_ab as A
from gait_ab import cell, write

import gfmref  # noqa: E402
from lmx import checkpoints, gfm  # noqa: E402

S = A.S


def flops_per_pass(cfg, N):
    D = cfg.d_model

    def attention(R):
        return 2 * R * D * 3 * D + 4 * R * R * D + 2 * R * D * D

    layer = attention(N) + 4 * N * D * cfg.ff + attention(N + 1)
    tail = 2 * D * 2 * D * 2 + 2 * N * D * (D // 2) + 2 * 3 * D * D + 2 * D * (D // 2)
    return 2 * N * cfg.input_dim * D + 2 * N * D * D + cfg.n_layers * layer + tail


def main():
    def lmx_sides(scorer, graphs, seeds):
        train, ev = scorer.batch(graphs), scorer.batch(graphs, [0] * len(graphs))
        return (lambda: (scorer.forward(train, seeds, S), scorer.forward(ev, None, 0, node=True))), (lambda: scorer.forward(train, seeds, S))

    def eval_forward(cfg, w, gr, dev):
        ev = gfmref.forward(cfg, w, gr, None, torch.float32, 0, dev)
        return ev["node_pred"], ev["attn"]

    args, cfg, rows, _, (cus, mhz, where) = A.measure(
        "gfm_ab", gfm, gfm.GfmScorer, gfmref, checkpoints.gfm_from_state_dict,
        lambda cfg, w, gr, dev: gfmref.forward(cfg, w, gr, lambda v, site: F.dropout(v, cfg.dropout, True), torch.float32, 0, dev)["pred"],
        eval_forward, lmx_sides)
    lines = [f"Graph transformer, shipped configuration (50 -> d_model 128, 8 heads, 6 layers, FF 512), graphs with timestamps, k = 5, S = {S} "
             f"samples; {where}",
             f"{'N':>3} {'n':>4}  {'lmx S = 10 + eval launches, ms':>32}  {'torch eager 10 + 1 forwards per graph, ms':>42}  {'ratio':>7}  "
             f"{'lmx S = 10 launches alone, ms':>32}  {'graphs/s':>9}  {'TFLOP/s':>8}"]
    for (N, n), sides in rows.items():
        a, b, c = sides
        ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
        fl = flops_per_pass(cfg, N)
        lines.append(f"{N:>3} {n:>4}  {cell(a, 12, 4)}  {cell(b, 12, 3):>42}  {mb / ma:>7.1f}  {cell(c, 12, 4)}  {n / ma * 1e3:>9.0f}  "
                     f"{n * S * fl / mc / 1e9:>8.2f}")
    N = gfm.MAX_NODES
    lines += A.last_lines(rows, flops_per_pass(cfg, 8), flops_per_pass(cfg, N), N, cus, mhz, "launches")
    write(args.out, lines)


if __name__ == "__main__":
    main()
