"""What tools/gfm_ab.py and tools/gnn_ab.py share on top of gait_ab: the shipped network on the GPU, the PyTorch-ROCm side run the way
the services run it (ten eager train-mode forwards one after the other, then the eval-mode forward, graph after graph), the shapes
(N = 8 and the largest graph, one graph and a backlog of 64), and the last lines of the table."""
import statistics

import torch

import gait_ab as G

S, BACKLOG = 10, 64


def measure(name, mod, scorer_cls, ref, from_state_dict, train_forward, eval_forward, lmx_sides):
    """train_forward(cfg, weights, graph, dev) -> one train-mode prediction, eval_forward(...) -> the tuple of eval outputs;
    lmx_sides(scorer, graphs, seeds) -> callables: S = 10 and eval together first, then the launches timed alone.  Returns (args, cfg,
    {(N, n): one list of ms per side, the torch side second}, {N: edges of a graph}, G.device's triple)."""
    args = G.parse_args(name)
    dev = torch.device("cuda:0")
    cfg = ref.SHIPPED
    _, w = from_state_dict(ref.state_dict(cfg, 1), num_heads=cfg.n_heads, dropout=cfg.dropout)
    scorer = scorer_cls(cfg, w, device=dev)
    dev_w = {k: v.to(dev) for k, v in w.items()}

    def torch_score(graphs):
        """per graph: predict_with_uncertainty (ten train-mode forwards, stack, mean, unbiased std), then the eval forward"""
        out = []
        with torch.no_grad():
            for gr in graphs:
                preds = torch.stack([train_forward(cfg, dev_w, gr, dev) for _ in range(S)], 0)
                out.append((preds.mean(0), preds.std(0)) + eval_forward(cfg, dev_w, gr, dev))
        return out

    rows, edges = {}, {}
    for N in (8, mod.MAX_NODES):
        for n, iters_lmx, iters_torch in ((1, 50, 2), (BACKLOG, 10, 1)):
            g = torch.Generator().manual_seed(100 * N + n)
            graphs = [ref.make_graphs(cfg, N, g)[1] for _ in range(n)]
            edges[N] = len(graphs[0]["edges"])
            both, *alone = lmx_sides(scorer, graphs, list(range(1, n + 1)))
            rows[(N, n)] = G.alternate([(both, iters_lmx), (lambda: torch_score(graphs), iters_torch)] + [(f, iters_lmx) for f in alone], args.rounds)
    return args, cfg, rows, edges, G.device(dev, args.rounds)


def last_lines(rows, flops_8, flops_max, N, cus, mhz, launches):
    """the FLOP counts and the f32 MFMA bound of the backlog at the largest N against the S = 10 side (the third); `launches`: the word"""
    bound_ms, derivation = G.bound(BACKLOG * S * flops_max, cus, mhz)
    return [f"FLOPs per (graph, sample): {flops_8 / 1e6:.2f} M at N = 8, {flops_max / 1e6:.2f} M at N = {N}",
            f"f32 MFMA bound for N = {N}, n = {BACKLOG}, S = {S}: {derivation}; S = 10 {launches} / bound = "
            f"{statistics.median(rows[(N, BACKLOG)][2]) / bound_ms:.2f}"]
