"""Timing of GraphGPS: lmx.gnn.GnnScorer (ONE launch for n graphs x 10 MC-dropout samples, then one eval launch for the cow score, the
node scores and the attention weights; csrc/gnn.hip) against the same live network in float32 through PyTorch-ROCm on the same GPU, run
the way services/gnn-pipeline runs it: ten eager train-mode forwards one after the other (predict_with_uncertainty), then the eval-mode
forward, graph after graph — tests/gnnref.py with F.dropout.  The reference itself cannot run there; its eleven host-side
eigendecompositions and 16 dense matrix powers per forward, and its dead post-pool half, are NOT in this baseline (the restatement reads
the prepared encodings), so the torch side is favoured.

HIP-event times; every shape is warmed up first; the sides alternate inside each round and the table gives the median over the rounds
with the spread.  FLOPs are counted from the shapes (2 R K N per linear layer over R rows, 4 N N D for the scores and P.V).

    python tools/gnn_ab.py [--rounds 7] [--out profiles/gnn_ab.txt]"""
import statistics

import torch
import torch.nn.functional as F

import graph_ab as A
from gait_ab import cell, write

import gnnref  # noqa: E402
from lmx import checkpoints, gnn  # noqa: E402

S = A.S


def flops_per_pass(cfg, N, E):
    D, L = cfg.d_model, cfg.n_layers
    edge_enc = 2 * E * (D // 2) * D
    layer = 2 * N * D * 4 * D + 2 * E * D * D + 2 * N * D * 3 * D + 4 * N * N * D + 2 * N * D * D + 4 * N * D * cfg.ff
    update = 2 * E * 3 * D * D + 2 * E * D * D
    return 2 * N * cfg.input_dim * (D - 2 * cfg.pe_dim) + edge_enc + L * layer + (L - 1) * update + 2 * N * D * (D // 2)


def main():
    def lmx_sides(scorer, graphs, seeds):
        b = scorer.batch(graphs)
        return ((lambda: (scorer.forward(b, seeds, S), scorer.forward(b, None, 0))), (lambda: scorer.forward(b, seeds, S)),
                (lambda: scorer.forward(b, None, 0)))

    def eval_forward(cfg, w, gr, dev):
        ev = gnnref.forward(cfg, w, gr, None, torch.float32, False, dev)
        return ev["graph_pred"], ev["node_pred"], ev["attw"]

    args, cfg, rows, edges, (cus, mhz, where) = A.measure(
        "gnn_ab", gnn, gnn.GnnScorer, gnnref, checkpoints.gnn_from_state_dict,
        lambda cfg, w, gr, dev: gnnref.forward(cfg, w, gr, lambda v, site: F.dropout(v, cfg.dropout, True), torch.float32, True, dev)["node_pred"],
        eval_forward, lmx_sides)
    lines = [f"GraphGPS, shipped configuration (50 -> d_model 128, 8 heads, 2 live layers of num_layers 4, FF 512), graphs with timestamps, k = 5, "
             f"S = {S} samples; {where}",
             f"{'N':>3} {'E':>4} {'n':>4}  {'lmx S = 10 + eval launches, ms':>32}  {'torch eager 10 + 1 forwards per graph, ms':>42}  {'ratio':>7}  "
             f"{'lmx S = 10 launch alone, ms':>32}  {'lmx eval launch alone, ms':>32}  {'graphs/s':>9}  {'TFLOP/s':>8}"]
    for (N, n), sides in rows.items():
        a, b, c, d = sides
        ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
        fl = flops_per_pass(cfg, N, edges[N])
        lines.append(f"{N:>3} {edges[N]:>4} {n:>4}  {cell(a, 12, 4)}  {cell(b, 12, 3):>42}  {mb / ma:>7.1f}  {cell(c, 12, 4)}  {cell(d, 12, 4)}  "
                     f"{n / ma * 1e3:>9.0f}  {n * S * fl / mc / 1e9:>8.2f}")
    N = gnn.MAX_NODES
    lines += A.last_lines(rows, flops_per_pass(cfg, 8, edges[8]), flops_per_pass(cfg, N, edges[N]), N, cus, mhz, "launch")
    lines.append("Not in the torch baseline: the reference's eleven host-side eigendecompositions and matrix powers per video, and its dead post-pool layers.")
    write(args.out, lines)


if __name__ == "__main__":
    main()
