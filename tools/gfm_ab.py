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

import gait_ab as G

import gfmref  # noqa: E402
from lmx import checkpoints, gfm  # noqa: E402

S, BACKLOG = 10, 64


def flops_per_pass(cfg, N):
    D = cfg.d_model

    def attention(R):
        return 2 * R * D * 3 * D + 4 * R * R * D + 2 * R * D * D

    layer = attention(N) + 4 * N * D * cfg.ff + attention(N + 1)
    tail = 2 * D * 2 * D * 2 + 2 * N * D * (D // 2) + 2 * 3 * D * D + 2 * D * (D // 2)
    return 2 * N * cfg.input_dim * D + 2 * N * D * D + cfg.n_layers * layer + tail


def main():
    args = G.parse_args("gfm_ab")
    dev = torch.device("cuda:0")
    cfg = gfmref.SHIPPED
    _, w = checkpoints.gfm_from_state_dict(gfmref.state_dict(cfg, 1), num_heads=cfg.n_heads, dropout=cfg.dropout)
    scorer = gfm.GfmScorer(cfg, w, device=dev)
    dev_w = {k: v.to(dev) for k, v in w.items()}

    def torch_score(graphs):
        """per graph: predict_with_uncertainty (ten train-mode forwards, stack, mean, unbiased std), then the eval forward"""
        out = []
        with torch.no_grad():
            for gr in graphs:
                preds = torch.stack([gfmref.forward(cfg, dev_w, gr, lambda v, site: F.dropout(v, cfg.dropout, True), torch.float32, 0, dev)["pred"]
                                     for _ in range(S)], 0)
                ev = gfmref.forward(cfg, dev_w, gr, None, torch.float32, 0, dev)
                out.append((preds.mean(0), preds.std(0), ev["node_pred"], ev["attn"]))
        return out

    rows = {}
    for N in (8, gfm.MAX_NODES):
        for n, iters_lmx, iters_torch in ((1, 50, 2), (BACKLOG, 10, 1)):
            g = torch.Generator().manual_seed(100 * N + n)
            graphs = [gfmref.make_graphs(cfg, N, g)[1] for _ in range(n)]
            train, ev = scorer.batch(graphs), scorer.batch(graphs, [0] * n)
            seeds = list(range(1, n + 1))
            rows[(N, n)] = G.alternate([(lambda: (scorer.forward(train, seeds, S), scorer.forward(ev, None, 0, node=True)), iters_lmx),
                                        (lambda: torch_score(graphs), iters_torch), (lambda: scorer.forward(train, seeds, S), iters_lmx)], args.rounds)

    cus, mhz, where = G.device(dev, args.rounds)
    lines = [f"Graph transformer, shipped configuration (50 -> d_model 128, 8 heads, 6 layers, FF 512), graphs with timestamps, k = 5, S = {S} "
             f"samples; {where}",
             f"{'N':>3} {'n':>4}  {'lmx S = 10 + eval launches, ms':>32}  {'torch eager 10 + 1 forwards per graph, ms':>42}  {'ratio':>7}  "
             f"{'lmx S = 10 launches alone, ms':>32}  {'graphs/s':>9}  {'TFLOP/s':>8}"]
    for (N, n), sides in rows.items():
        a, b, c = sides
        ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
        fl = flops_per_pass(cfg, N)
        lines.append(f"{N:>3} {n:>4}  {G.cell(a, 12, 4)}  {G.cell(b, 12, 3):>42}  {mb / ma:>7.1f}  {G.cell(c, 12, 4)}  {n / ma * 1e3:>9.0f}  "
                     f"{n * S * fl / mc / 1e9:>8.2f}")
    N = gfm.MAX_NODES
    fl = flops_per_pass(cfg, N)
    lines.append(f"FLOPs per (graph, sample): {flops_per_pass(cfg, 8) / 1e6:.2f} M at N = 8, {fl / 1e6:.2f} M at N = {N}")
    bound_ms, derivation = G.bound(BACKLOG * S * fl, cus, mhz)
    lines.append(f"f32 MFMA bound for N = {N}, n = {BACKLOG}, S = {S}: {derivation}; S = 10 launches / bound = "
                 f"{statistics.median(rows[(N, BACKLOG)][-1]) / bound_ms:.2f}")
    G.write(args.out, lines)


if __name__ == "__main__":
    main()
