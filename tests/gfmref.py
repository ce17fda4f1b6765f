"""Yardstick of the graph transformer tests (a helper, not a test): the network of include/lmx.h "The graph transformer" restated
functionally in torch — matmuls, F.layer_norm, torch.softmax, dropout as explicit keep arrays — in float32 or float64; a seeded weight
generator that emits a state_dict under the reference's key names (every bias, spd_bias, the degree tables and the virtual nodes
nonzero); the graph builder's pinned rules restated in numpy; the cases; and the tolerance rule of tcnref.tolerances, extended to the
virtual node, the node scores and the attention column."""
import dataclasses
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import tcnref
from lmx import gfm

SHIPPED = gfm.GfmConfig()
# ragged input, FF % 64 != 0, and both clamps bite: k = 5 neighbours exceed max_degree 4, paths exceed max_spd 2
TINY = gfm.GfmConfig(input_dim=5, d_model=32, n_heads=2, n_layers=1, ff=48, max_degree=4, max_spd=2, dropout=0.3)
WIDE = gfm.GfmConfig(input_dim=50, d_model=64, n_heads=2, n_layers=2, ff=128, dropout=0.1)  # head_dim 32
CONFIGS = {"shipped": SHIPPED, "tiny": TINY, "wide": WIDE}
# N and N + 1 (the virtual node's row) on every side of the 16-row tile, up to the limit
N_BY_CONFIG = {"shipped": (1, 2, 14, 15, 16, 17, 31, 32, 33, 47, 48, 63, gfm.MAX_NODES), "tiny": (1, 6, 7, 33), "wide": (5, 48)}
S_VALUES = (0, 2, 10)
M64 = tcnref.M64
PRED_FLOOR = tcnref.PRED_FLOOR
K_NEIGHBOURS = 5
EMB_DIM = 12


def state_dict(cfg, seed):
    """A state_dict as `torch.save(model.state_dict())` of the reference's CowLamenessGraphormer writes it, with Xavier-sized matrices."""
    g = torch.Generator().manual_seed(seed)

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    sd = {}

    def linear(prefix, n, k):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = uniform((n, k), (6.0 / (n + k)) ** 0.5), uniform((n,), 0.2)

    def norm(prefix):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = 1.0 + uniform((cfg.d_model,), 0.3), uniform((cfg.d_model,), 0.2)

    D, H = cfg.d_model, cfg.n_heads
    linear("input_proj.0", D, cfg.input_dim)
    norm("input_proj.1")
    sd["encodings.centrality_enc.degree_encoder.weight"] = uniform((cfg.max_degree + 1, D), 0.3)
    sd["encodings.centrality_enc.out_degree_encoder.weight"] = uniform((cfg.max_degree + 1, D), 0.3)
    sd["encodings.spatial_enc.spd_bias.weight"] = uniform((cfg.max_spd + 2, H), 1.0)
    linear("encodings.edge_enc.edge_proj.0", 2 * H, cfg.edge_dim)
    linear("encodings.edge_enc.edge_proj.2", H, 2 * H)
    linear("encodings.temporal_enc.time_proj", D, D)
    sd["encodings.temporal_enc.div_term"] = torch.exp(torch.arange(0, D, 2).float() * (-math.log(10000.0) / D))
    for i in range(cfg.n_layers):
        p = f"encoder.layers.{i}"
        norm(f"{p}.norm1"), norm(f"{p}.norm2")
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            linear(f"{p}.self_attn.{name}", D, D)
        linear(f"{p}.ffn.0", cfg.ff, D), linear(f"{p}.ffn.3", D, cfg.ff)
        v = f"encoder.virtual_node_layers.{i}"
        sd[f"{v}.virtual_node"] = uniform((1, D), 0.5)
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            linear(f"{v}.vn_attention.{name}", D, D)
        linear(f"{v}.vn_update.0", 2 * D, D), linear(f"{v}.vn_update.2", D, 2 * D), norm(f"{v}.vn_update.3")
    norm("encoder.final_norm")
    linear("readout.attention_pool.0", D // 2, D), linear("readout.attention_pool.2", 1, D // 2)
    linear("readout.combine.0", D, 3 * D), norm("readout.combine.2")
    linear("pred_head.0", D // 2, D), linear("pred_head.3", D // 4, D // 2), linear("pred_head.6", 1, D // 4)
    linear("node_pred.0", D // 2, D), linear("node_pred.3", 1, D // 2)
    return sd


def build_graph(cfg, x, emb, ts=None, k=K_NEIGHBOURS):
    """The rules of include/lmx.h for lmx_h_gfm_graph restated in numpy, operation for operation (the sums in ascending channel order, so
    that the doubles are the library's): the dict of lmx.gfm.build_graph."""
    emb = np.asarray(emb, np.float32)
    N, E = emb.shape
    k = min(k, N - 1)
    edges, attr = [], []
    if k > 0:
        e64 = emb.astype(np.float64)
        ss = np.zeros((N,))
        for c in range(E):
            ss = ss + e64[:, c] * e64[:, c]
        unit = e64 / (np.sqrt(ss) + 1e-8)[:, None]
        sim = np.zeros((N, N))
        for c in range(E):
            sim = sim + unit[:, c, None] * unit[None, :, c]
        for i in range(N):
            order = sorted((j for j in range(N) if j != i), key=lambda j: (sim[i, j], j))  # ties: the lower index first
            for j in order[-k:]:
                edges.append((i, j)), attr.append((np.float32(max(0.0, sim[i, j])), 1.0, 0.0))
    if ts is not None and N > 1:
        ts = np.asarray(ts, np.float32)
        order = np.argsort(ts, kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            weight = np.float32(math.exp(-abs(float(ts[b]) - float(ts[a])) / 86400.0))
            edges += [(int(a), int(b)), (int(b), int(a))]
            attr += [(weight, 0.0, 1.0)] * 2
    return finish_graph(cfg, x, np.array(edges, np.int32).reshape(-1, 2), np.array(attr, np.float32).reshape(-1, 3), ts)


def finish_graph(cfg, x, edges, attr, ts=None):
    """degrees, the winning edge and the shortest-path index of an edge list"""
    N = len(x)
    din, dout = np.zeros((N,), np.int64), np.zeros((N,), np.int64)
    win, adj = np.full((N, N), -1, np.int32), np.zeros((N, N), bool)
    for e, (s, d) in enumerate(edges):
        dout[s] += 1
        din[d] += 1
        win[s, d] = e  # the later edge wins
        adj[s, d] = adj[d, s] = True
    idx = np.zeros((N, N), np.uint8)
    for i in range(N):
        dist = np.full((N,), -1)
        dist[i], front, d = 0, [i], 0
        while front:
            d += 1
            nxt = [v for v in np.flatnonzero(adj[front].any(0)) if dist[v] < 0]
            dist[nxt] = d
            front = nxt
        idx[i] = np.where((dist < 0) | (dist > cfg.max_spd), cfg.max_spd, dist) + 1
    return {"x": np.ascontiguousarray(x, np.float32), "timestamps": None if ts is None else np.asarray(ts, np.float32), "edges": edges,
            "edge_attr": attr, "deg_in": np.minimum(din, cfg.max_degree).astype(np.uint8), "deg_out": np.minimum(dout, cfg.max_degree).astype(np.uint8),
            "idx": idx, "win": win}


def site_shapes(cfg, N):
    """The activation each DRAWN dropout site multiplies, in torch's memory order (include/lmx.h has the table); site 6L + 3 is never drawn."""
    D, H = cfg.d_model, cfg.n_heads
    out = [(N, D)]
    for _ in range(cfg.n_layers):
        out += [(H, N, N), (N, D), (N, cfg.ff), (N, D), (H, N + 1, N + 1), (N + 1, D)]
    return out + [(D // 2,), (D // 4,)]


def keep_arrays(cfg, N, seed, sample):
    """Every drawn site's keep array of one (graph, sample), shaped as the activation it multiplies."""
    return [torch.from_numpy(tcnref.keep_bits(seed, sample, site, cfg.n_sites, int(np.prod(sh)), cfg.dropout).astype(np.float64)).reshape(sh)
            for site, sh in enumerate(site_shapes(cfg, N))]


def bernoulli_keeps(cfg, N, batch, generator):
    """keep arrays drawn by torch's own generator, as nn.Dropout draws them: Bernoulli(1 - p) per element"""
    return [torch.bernoulli(torch.full((batch,) + sh, 1.0 - cfg.dropout), generator=generator) for sh in site_shapes(cfg, N)]


def attention_bias(cfg, W, graph, dtype, device="cpu"):
    """[H, N, N]: spd[idx] + edge_mlp(edge_attr[win]) where there is an edge"""
    idx = torch.from_numpy(graph["idx"].astype(np.int64)).to(device)
    win = torch.from_numpy(graph["win"].astype(np.int64)).to(device)
    bias = W["spd"][idx]  # [N, N, H]
    if len(graph["edge_attr"]):
        attr = torch.from_numpy(graph["edge_attr"]).to(device=device, dtype=dtype)
        mlp = torch.relu(attr @ W["edge1.weight"].t() + W["edge1.bias"]) @ W["edge2.weight"].t() + W["edge2.bias"]
        bias = bias + torch.where((win >= 0)[..., None], mlp[win.clamp(min=0)], torch.zeros((), dtype=dtype, device=device))
    return bias.permute(2, 0, 1)


def forward(cfg, w, graph, keeps=None, dtype=torch.float64, target=None, device="cpu"):
    """One graph -> dict(trunk [N, D], vn [D], pred scalar, node_pred [N], attn [N] or None) in `dtype`.  keeps: None (eval mode), one
    0/1 array per drawn site (site_shapes; with a leading B every output gains a leading B), or a function (activation, site) ->
    activation that does the dropout itself (tools: F.dropout)."""
    W = {k: v.to(device=device, dtype=dtype) for k, v in w.items()}
    D, H, dh, L = cfg.d_model, cfg.n_heads, cfg.head_dim, cfg.n_layers
    batched = keeps is not None and not callable(keeps) and keeps[0].dim() == 3
    scale = torch.tensor(float(np.float32(1.0 / (1.0 - cfg.dropout))), dtype=dtype, device=device)
    cs = torch.tensor(float(np.float32(float(dh) ** -0.5)), dtype=dtype, device=device)

    def drop(v, site):
        if callable(keeps):
            return keeps(v, site)
        if keeps is None:
            return v
        k = keeps[site].to(device=device, dtype=dtype)
        return v * (k if batched else k[None]) * scale

    def norm(v, name):
        return F.layer_norm(v, (D,), W[name + ".weight"], W[name + ".bias"], 1e-5)

    def attend(a, bias, p, names, site):
        B, R = a.shape[:2]
        q, k, v = ((a @ W[p + n + ".weight"].t() + W[p + n + ".bias"]).reshape(B, R, H, dh).transpose(1, 2) for n in names[:3])
        P = drop(torch.softmax(q @ k.transpose(-1, -2) * cs + bias, -1), site)
        o = (P @ v).transpose(1, 2).reshape(B, R, D)
        return o @ W[p + names[3] + ".weight"].t() + W[p + names[3] + ".bias"], P

    x = torch.from_numpy(graph["x"]).to(device=device, dtype=dtype)[None]
    N = x.shape[1]
    enc = W["deg_in"][torch.from_numpy(graph["deg_in"].astype(np.int64)).to(device)] + W["deg_out"][torch.from_numpy(graph["deg_out"].astype(np.int64)).to(device)]
    if graph["timestamps"] is not None:
        ts = torch.from_numpy(graph["timestamps"]).to(device)  # float32 arithmetic up to the sinusoid's argument, as the header pins it
        days = torch.clamp((ts - ts.min()) / 86400.0, max=365.0)
        arg = (days[:, None] * w["div_term"].to(device=device, dtype=torch.float32)[None]).to(dtype)
        pe = torch.stack([torch.sin(arg), torch.cos(arg)], -1).reshape(N, D)
        enc = enc + (pe @ W["time.weight"].t() + W["time.bias"])
    bias = attention_bias(cfg, W, graph, dtype, device)
    ext = torch.zeros((H, N + 1, N + 1), dtype=dtype, device=device)
    ext[:, 1:, 1:] = bias
    h = drop(norm(x @ W["in.weight"].t() + W["in.bias"], "in_norm"), 0) + enc
    P = vn = None
    for l in range(L):
        p = f"layer.{l}."
        y, P = attend(norm(h, p + "ln1"), bias, p, ("q", "k", "v", "out"), 1 + 6 * l)
        h = h + drop(y, 2 + 6 * l)
        f = drop(F.gelu(norm(h, p + "ln2") @ W[p + "ff1.weight"].t() + W[p + "ff1.bias"]), 3 + 6 * l)
        h = h + drop(f @ W[p + "ff2.weight"].t() + W[p + "ff2.bias"], 4 + 6 * l)
        xv = torch.cat([W[p + "vn"].expand(h.shape[0], 1, D), h], 1)
        y = drop(attend(xv, ext, p, ("vq", "vk", "vv", "vout"), 5 + 6 * l)[0], 6 + 6 * l)
        h = y[:, 1:]
        if l == L - 1:
            u = F.gelu(y[:, 0] @ W[p + "vu1.weight"].t() + W[p + "vu1.bias"]) @ W[p + "vu2.weight"].t() + W[p + "vu2.bias"]
            vn = norm(u, p + "vu_norm")
    trunk = norm(h, "lnf")
    score = torch.tanh(trunk @ W["pool1.weight"].t() + W["pool1.bias"]) @ W["pool2.weight"].t() + W["pool2.bias"]  # [B, N, 1]
    pool = (torch.softmax(score, 1) * trunk).sum(1)
    r = norm(torch.relu(torch.cat([trunk.mean(1), vn, pool], -1) @ W["comb.weight"].t() + W["comb.bias"]), "comb_norm")
    h1 = drop(torch.relu(r @ W["ph1.weight"].t() + W["ph1.bias"]), 6 * L + 1)
    h2 = drop(torch.relu(h1 @ W["ph2.weight"].t() + W["ph2.bias"]), 6 * L + 2)
    pred = torch.sigmoid(h2 @ W["ph3.weight"].t() + W["ph3.bias"])[:, 0]
    node = torch.sigmoid(torch.relu(trunk @ W["nh1.weight"].t() + W["nh1.bias"]) @ W["nh2.weight"].t() + W["nh2.bias"])[..., 0]
    attn = None if target is None else P.mean(1)[:, :, target]
    out = {"trunk": trunk, "vn": vn, "pred": pred, "node_pred": node, "attn": attn, "last_attention": P}
    return out if batched else {k: (None if v is None else v[0]) for k, v in out.items()}


def make_graphs(cfg, N, g, path=False):
    """The graphs of one node count: kNN only; with timestamps (two equal ones and one span above 365 days; at N = 2 the temporal edge
    duplicates the kNN edge); for N >= 12 two well-separated clusters without timestamps, so that unreachable pairs exist; and, on
    request, a hand-made path graph of 14 nodes (shortest paths beyond max_spd)."""
    def feats(n):
        return torch.randn((n, cfg.input_dim), generator=g).numpy()

    emb = torch.randn((N, EMB_DIM), generator=g).numpy()
    ts = (1.7e9 + torch.rand((N,), generator=g) * 30 * 86400.0).numpy().astype(np.float32)
    if N >= 2:
        ts[N // 2] = ts[0]  # equal timestamps
    if N >= 3:
        ts[N - 1] = ts.min() + np.float32(400 * 86400.0)
    out = [build_graph(cfg, feats(N), emb), build_graph(cfg, feats(N), emb, ts)]
    if N >= 12:
        split = torch.randn((N, EMB_DIM), generator=g).numpy() * 0.05
        split[:N // 2, 0] += 10.0
        split[N // 2:, 1] += 10.0
        out.append(build_graph(cfg, feats(N), split))
    if path:
        edges = np.array([(i, i + 1) for i in range(13)] + [(i + 1, i) for i in range(13)], np.int32)
        attr = np.stack([torch.rand((26,), generator=g).numpy(), np.ones((26,), np.float32), np.zeros((26,), np.float32)], 1).astype(np.float32)
        out.append(finish_graph(cfg, feats(14), edges, attr))
    return out


@dataclasses.dataclass
class Case:
    """One (configuration, N, S) of a test module with its graphs and its float64 references, computed once."""
    name: str
    cfg: object
    weights: dict
    graphs: list
    targets: list
    seeds: list
    S: int
    ref: list = None     # per graph: dict of float64 tensors, trunk [max(S, 1), N, D], vn [max(S, 1), D], pred [max(S, 1)], node_pred, attn
    err: dict = None     # per output: max |float32 - float64| (trunk, vn, attn: relative to max |float64| of the case)
    scale: dict = None   # per output: max |float64| of the case


OUTPUTS = ("trunk", "vn", "pred", "node_pred", "attn")
RELATIVE = ("trunk", "vn", "attn")


def make_case(name, cfg, weights, N, S, seed=0, path=False):
    g = torch.Generator().manual_seed(1000 * N + 10 * S + seed)
    graphs = make_graphs(cfg, N, g, path)
    n = len(graphs)
    seeds = [int(v) & M64 for v in torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g).tolist()]
    seeds[0] |= 1 << 63  # the top bit too
    targets = [int(torch.randint(0, len(gr["x"]), (1,), generator=g)) for gr in graphs]
    case = Case(name, cfg, weights, graphs, targets, seeds, S, [], {})
    smax, keys = max(S, 1), OUTPUTS if S == 0 else OUTPUTS[:3]
    diff, scale = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    for i, gr in enumerate(graphs):
        r64, r32 = {k: [] for k in keys}, {k: [] for k in keys}
        for s in range(smax):
            keeps = keep_arrays(cfg, len(gr["x"]), seeds[i], s) if S else None
            a = forward(cfg, weights, gr, keeps, torch.float64, targets[i])
            b = forward(cfg, weights, gr, keeps, torch.float32, targets[i])
            for k in keys:
                r64[k].append(a[k]), r32[k].append(b[k].double())
        ref = {k: torch.stack(v) for k, v in r64.items()}
        if S == 0:
            ref["node_pred"], ref["attn"] = ref["node_pred"][0], ref["attn"][0]
        for k in keys:
            d32 = torch.stack(r32[k]).reshape(ref[k].shape)
            diff[k] = max(diff[k], float((d32 - ref[k]).abs().max()))
            scale[k] = max(scale[k], float(ref[k].abs().max()))
        case.ref.append(ref)
    case.scale = scale
    case.err = {k: diff[k] / scale[k] if k in RELATIVE else diff[k] for k in keys}
    return case


def tolerances(cases):
    """The rule of tcnref.tolerances, unchanged: e_ref is the largest float32-vs-float64 difference of gfmref itself over ALL cases of
    the module (trunk, vn and the attention column: relative to max |float64| of their case); the code under test may be off from
    float64 by 4 e_ref — the same f32 operations in another order — and a prediction (graph or node) by 4 f32 spacings at 1.0 more.
    Returns {output: (tolerance, e_ref)}."""
    out = {}
    for k in OUTPUTS:
        e = max((c.err[k] for c in cases if k in c.err), default=0.0)
        out[k] = (4 * e + (0.0 if k in RELATIVE else PRED_FLOOR), e)
    return out


def check_case(case, got, tols, what):
    """got: per graph a dict of the outputs of the code under test, shaped as case.ref; returns {output: error / allowed}."""
    ratios = {}
    for k in (OUTPUTS if case.S == 0 else OUTPUTS[:3]):
        d = max(float((got[i][k].double().cpu().reshape(case.ref[i][k].shape) - case.ref[i][k]).abs().max()) for i in range(len(case.graphs)))
        bound = tols[k][0] * (case.scale[k] if k in RELATIVE else 1.0)
        ratios[k] = d / bound
    print(f"{what} {case.name}: " + ", ".join(f"{k} |d| / bound {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, case.name, k, v)
    return ratios


def run_case(scorer, case):
    """The code under test on a case: per graph a dict shaped as case.ref (one call for all graphs and samples, one more in eval mode
    only when S == 0 for the node scores and the attention column)."""
    b = scorer.batch(case.graphs, case.targets if case.S == 0 else None)
    pred, stats, node, attn, trunk, vn = scorer.forward(b, case.seeds, case.S, node=case.S == 0, trunk=True, vn=True)
    cut = [int(v) for v in b.node_off]
    got = []
    for i in range(b.n):
        o = {"trunk": trunk[i], "vn": vn[i], "pred": pred[i]}
        if case.S == 0:
            o["node_pred"], o["attn"] = node[cut[i]:cut[i + 1]], attn[cut[i]:cut[i + 1]]
        got.append(o)
    return got, pred, stats


# ---- the reference's own model, where a checkout of it is at hand ----------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphormer_small_w5.npz")
GOLDEN_CFG = gfm.GfmConfig(input_dim=50, d_model=32, n_heads=2, n_layers=2, ff=64)  # what the golden file was recorded with
GOLDEN_SIZES = ((7, False), (17, True), (33, True))  # (nodes, with timestamps)


def reference_app():
    """services/graph-transformer-pipeline/app of a checkout of the reference, or None: the directory LMX_REFERENCE names, else a checkout
    called `reference` beside this repository."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tree in (os.environ.get("LMX_REFERENCE"), os.path.join(os.path.dirname(root), "reference")):
        app = os.path.join(tree, "services", "graph-transformer-pipeline", "app") if tree else None
        if app and os.path.isfile(os.path.join(app, "model", "graphormer.py")):
            return app
    return None


def reference_modules():
    """The reference's `model.graphormer`, imported under a name of its own (no top-level `model` enters sys.modules) with a stand-in for
    torch_geometric.data.Data, which is all the model uses of that package; None where the checkout or networkx is missing."""
    import importlib.util
    import os
    import sys
    import types

    app = reference_app()
    if app is None or importlib.util.find_spec("networkx") is None:
        return None
    name = "lmx_reference_graphormer_model"
    if name + ".graphormer" in sys.modules:
        return sys.modules[name + ".graphormer"]

    class Data:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    tg, tgd = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.data")
    tgd.Data, tg.data = Data, tgd
    saved = {k: sys.modules.get(k) for k in ("torch_geometric", "torch_geometric.data")}
    sys.modules.update({"torch_geometric": tg, "torch_geometric.data": tgd})
    try:
        pkg = os.path.join(app, "model")
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return sys.modules[name + ".graphormer"]


def load_golden():
    """(cfg, weights, [case]) of the golden file: each case a dict with the graph as gfmref.build_graph makes it from the recorded inputs
    (its edge attributes replaced by the recorded ones, so that only the network is compared), the reference builder's edge_index and
    edge_attr, the target, and the reference's eval-mode outputs graph_pred, node_pred [N] and attn [N] (head average of the last layer's
    attention, the target's column)."""
    from lmx import checkpoints

    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    cfg, w = checkpoints.gfm_from_state_dict(sd, num_heads=GOLDEN_CFG.n_heads, dropout=GOLDEN_CFG.dropout)
    assert cfg == GOLDEN_CFG
    cases = []
    for i, (N, timed) in enumerate(GOLDEN_SIZES):
        p = f"g{i}/"
        graph = build_graph(cfg, z[p + "x"], z[p + "emb"], z[p + "ts"] if timed else None)
        cases.append({"graph": graph, "built_attr": graph["edge_attr"], "edge_index": z[p + "edge_index"], "edge_attr": z[p + "edge_attr"],
                      "emb": z[p + "emb"], "target": int(z[p + "target"]), "graph_pred": float(z[p + "graph_pred"]),
                      "node_pred": torch.from_numpy(z[p + "node_pred"]).double(), "attn": torch.from_numpy(z[p + "attn"]).double()})
        graph["edge_attr"] = z[p + "edge_attr"]
    return cfg, w, cases


def check_golden(cases, got, w, cfg, what):
    """got: per case (pred, node_pred [N], attn [N]) of the code under test against the REFERENCE's recorded float32 outputs.  The rule of
    tolerances(): the recorded outputs and the code under test may each be off from float64 by 4 e_ref — the restatement's own float32
    error over the golden's cases — so they may differ by 8 e_ref, plus 4 float32 spacings on a prediction; the attention column relative
    to its case's maximum."""
    e = {"pred": 0.0, "node_pred": 0.0, "attn": 0.0}
    for c in cases:
        r64 = forward(cfg, w, c["graph"], None, torch.float64, c["target"])
        r32 = forward(cfg, w, c["graph"], None, torch.float32, c["target"])
        c["scale"] = float(r64["attn"].abs().max())
        for k in e:
            e[k] = max(e[k], float((r32[k].double() - r64[k]).abs().max()) / (c["scale"] if k == "attn" else 1.0))
    worst = dict.fromkeys(e, 0.0)
    for c, (pred, node, attn) in zip(cases, got):
        diffs = {"pred": abs(float(pred) - c["graph_pred"]), "node_pred": float((node.double().cpu() - c["node_pred"]).abs().max()),
                 "attn": float((attn.double().cpu() - c["attn"]).abs().max()) / c["scale"]}
        for k, d in diffs.items():
            bound = 8 * e[k] + (0.0 if k == "attn" else PRED_FLOOR)
            worst[k] = max(worst[k], d / bound)
            assert d <= bound, (what, k, d, bound)
    print(f"{what} against the reference's recorded outputs, worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
    return worst
