"""What the GraphGPS tests share (no test in here): the LIVE network of services/gnn-pipeline's EnhancedGraphGPS restated functionally
in torch, in float32 or float64, with dropout as explicit keep arrays and BatchNorm in both modes; a seeded state_dict under the
reference's key names, dead keys included; the graph builder's and both encodings' pinned rules (include/lmx.h "GraphGPS") restated in
numpy; and the tolerance rule of tcnref.tolerances."""
import dataclasses
import math

import numpy as np
import torch
import torch.nn.functional as F

import tcnref
from lmx import gnn

SHIPPED = gnn.GnnConfig()  # 50 -> 128, 8 heads, num_layers 4 (two live layers), pe 16
# one live layer (no edge update at all), ragged input, 6 edges at N = 3
TINY = gnn.GnnConfig(input_dim=5, d_model=32, n_heads=2, n_layers=1, pe_dim=8, ff=128, dropout=0.3)
WIDE = gnn.GnnConfig(input_dim=50, d_model=64, n_heads=2, n_layers=2, pe_dim=16, ff=256, dropout=0.1)  # head_dim 32
CONFIGS = {"shipped": SHIPPED, "tiny": TINY, "wide": WIDE}
# N on both sides of the 16-row tile and of the dense-eigh boundary (9 | 10), and MAX_NODES once
N_BY_CONFIG = {"shipped": (2, 3, 8, 9, 10, 15, 16, 17, 33, gnn.MAX_NODES), "tiny": (2, 3, 17), "wide": (9, 33)}
S_VALUES = (0, 2, 10)
M64 = tcnref.M64
PRED_FLOOR = tcnref.PRED_FLOOR
K_NEIGHBOURS = 5
EMB_DIM = 12


def state_dict(cfg, seed, dead=True):
    """A state_dict as `torch.save(model.state_dict())` of the reference's EnhancedGraphGPS writes it (num_layers = 2 x cfg.n_layers):
    every bias nonzero, running statistics nonzero with variances in 0.5 .. 2, and (dead) the keys that reach no output."""
    g = torch.Generator().manual_seed(seed)
    D, P = cfg.d_model, cfg.pe_dim

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    sd = {}

    def linear(prefix, n, k):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = uniform((n, k), (6.0 / (n + k)) ** 0.5), uniform((n,), 0.2)

    def norm(prefix, d=D):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"] = 1.0 + uniform((d,), 0.3), uniform((d,), 0.2)

    def bnorm(prefix):
        norm(prefix)
        sd[f"{prefix}.running_mean"], sd[f"{prefix}.running_var"] = uniform((D,), 0.5), 0.5 + 1.5 * torch.rand((D,), generator=g)
        sd[f"{prefix}.num_batches_tracked"] = torch.tensor(7)

    def gps_layer(p):
        norm(f"{p}.norm1"), norm(f"{p}.norm2"), norm(f"{p}.norm3")
        for name in "ABDEC":
            linear(f"{p}.local_conv.{name}", D, D)
        linear(f"{p}.local_conv.edge_update.0", D, 3 * D), linear(f"{p}.local_conv.edge_update.2", D, D)
        bnorm(f"{p}.local_conv.bn_node"), bnorm(f"{p}.local_conv.bn_edge")
        sd[f"{p}.global_attn.attention.in_proj_weight"] = uniform((3 * D, D), (6.0 / (4 * D)) ** 0.5)
        sd[f"{p}.global_attn.attention.in_proj_bias"] = uniform((3 * D,), 0.2)
        linear(f"{p}.global_attn.attention.out_proj", D, D)
        norm(f"{p}.global_attn.norm")
        linear(f"{p}.global_attn.pe_bias", cfg.n_heads, D)
        linear(f"{p}.ffn.0", cfg.ff, D), linear(f"{p}.ffn.3", D, cfg.ff)

    linear("input_proj", D - 2 * P, cfg.input_dim)
    linear("edge_encoder.encoder.0", D // 2, cfg.edge_dim), linear("edge_encoder.encoder.2", D, D // 2), norm("edge_encoder.encoder.3")
    for enc, k in (("lap_pe", gnn.LAP_K), ("rw_pe", gnn.RW_K)):
        linear(f"{enc}.transform.0", 2 * P, k), linear(f"{enc}.transform.2", P, 2 * P), norm(f"{enc}.transform.3", P)
    for i in range(cfg.n_layers):
        gps_layer(f"pre_pool_layers.{i}")
    norm("final_norm")
    linear("pred_head.node_attention.0", D // 2, D), linear("pred_head.node_attention.2", 1, D // 2)
    linear("pred_head.classifier.0", D, 2 * D), linear("pred_head.classifier.3", D // 2, D), linear("pred_head.classifier.6", 1, D // 2)
    linear("pred_head.node_classifier.0", D // 2, D), linear("pred_head.node_classifier.3", 1, D // 2)
    if dead:
        for i in range(cfg.n_layers):
            gps_layer(f"post_pool_layers.{i}")
        linear("pool_layer.pool.gnn.lin_rel", 1, D)
        sd["pool_layer.pool.gnn.lin_root.weight"] = uniform((1, D), 0.1)
        linear("pool_layer.project.0", D, D), norm("pool_layer.project.2")
        linear("multi_scale_readout.scale_attention.0", D, 2 * D), linear("multi_scale_readout.scale_attention.2", 2, D)
        linear("multi_scale_readout.output_proj.0", D, D), norm("multi_scale_readout.output_proj.2")
    else:
        last = f"pre_pool_layers.{cfg.n_layers - 1}.local_conv."
        sd = {k: v for k, v in sd.items() if not k.startswith((last + "edge_update.", last + "bn_edge.")) and ".pe_bias." not in k}
    return sd


def laplacian(N, edges):
    """(A with multiplicities and self-loops, its row sums, L = I - D^-1/2 A D^-1/2 symmetrised from its lower triangle), float64"""
    A = np.zeros((N, N))
    for s, d in edges:
        A[s, d] += 1.0
    A += np.eye(N)
    deg = np.zeros((N,))
    for j in range(N):
        deg = deg + A[:, j]
    dis = 1.0 / np.sqrt(deg)
    L = np.eye(N) - (dis[:, None] * A) * dis[None, :]
    L = np.tril(L) + np.tril(L, -1).T
    return A, deg, L


def lap_pe(N, edges):
    """The rule of include/lmx.h through numpy's eigh on the lower triangle: |columns 1 .. 8| in ascending eigenvalue, zero columns where
    N <= 8.  Equal to the library's Jacobi wherever the spectrum is simple (the tests say when); returns (pe f32, eigenvalues, L)."""
    _, _, L = laplacian(N, edges)
    lam, V = np.linalg.eigh(L, UPLO="L")
    order = np.argsort(lam, kind="stable")
    lam, V = lam[order], V[:, order]
    pe = np.zeros((N, gnn.LAP_K))
    k = min(gnn.LAP_K, N - 1)
    pe[:, :k] = np.abs(V[:, 1:1 + k])
    return pe.astype(np.float32), lam, L


def rw_pe(N, edges):
    """diag(P^k), k = 1 .. 16, P = D^-1 A in float64 with every inner product in ascending index order, then float32"""
    A, deg, _ = laplacian(N, edges)
    P = (1.0 / deg)[:, None] * A
    Pk, out = P.copy(), np.zeros((N, gnn.RW_K), np.float32)
    for step in range(gnn.RW_K):
        out[:, step] = np.diag(Pk).astype(np.float32)
        nxt = np.zeros((N, N))
        for m in range(N):
            nxt = nxt + Pk[:, m, None] * P[None, m, :]
        Pk = nxt
    return out


def build_graph(cfg, x, emb, ts=None, k=K_NEIGHBOURS):
    """The rules of include/lmx.h for lmx_h_gnn_graph restated in numpy, operation for operation (the sums in ascending channel order,
    so that the doubles are the library's): the dict of lmx.gnn.build_graph.  ts: the timestamps of a known cow, or None."""
    emb = np.asarray(emb, np.float32)
    N, E = emb.shape
    if N <= k:
        k = max(1, N - 1)
    edges, attr = [], []
    if N > 1:
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
                edges.append((i, j)), attr.append((np.float32(sim[i, j]), 1.0, 0.0))  # the raw cosine
    if ts is not None and N > 1:
        ts = np.asarray(ts, np.float64)  # the reference keeps its timestamps as Python floats
        order = np.argsort(ts, kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            weight = np.float32(math.tanh(abs(float(ts[b]) - float(ts[a])) / 86400.0))
            edges += [(int(a), int(b)), (int(b), int(a))]
            attr += [(weight, 0.0, 1.0)] * 2
    return finish_graph(x, np.array(edges, np.int32).reshape(-1, 2), np.array(attr, np.float32).reshape(-1, 3))


def finish_graph(x, edges, attr):
    """the CSR by destination (edges of one destination in edge order), the clamped in-degree and both encodings of an edge list"""
    N = len(x)
    order = np.argsort(edges[:, 1], kind="stable").astype(np.int32) if len(edges) else np.zeros((0,), np.int32)
    din = np.bincount(edges[:, 1], minlength=N) if len(edges) else np.zeros((N,), np.int64)
    ptr = np.zeros((N + 1,), np.int32)
    ptr[1:] = np.cumsum(din)
    return {"x": np.ascontiguousarray(x, np.float32), "edges": edges, "edge_attr": attr, "csr_ptr": ptr, "csr_edge": order,
            "deg": np.maximum(din, 1).astype(np.int32), "lap": lap_pe(N, edges)[0], "rw": rw_pe(N, edges)}


def site_shapes(cfg, N):
    """The activation each dropout site multiplies, in torch's memory order (include/lmx.h has the table)."""
    D, H = cfg.d_model, cfg.n_heads
    out = []
    for _ in range(cfg.n_layers):
        out += [(N, D), (H, N, N), (N, D), (N, cfg.ff), (N, D)]
    return out + [(N, D // 2)]


def keep_arrays(cfg, N, seed, sample):
    """Every site's keep array of one (graph, sample), shaped as the activation it multiplies."""
    return [torch.from_numpy(tcnref.keep_bits(seed, sample, site, cfg.n_sites, int(np.prod(sh)), cfg.dropout).astype(np.float64)).reshape(sh)
            for site, sh in enumerate(site_shapes(cfg, N))]


def bernoulli_keeps(cfg, N, batch, generator):
    """keep arrays drawn by torch's own generator, as nn.Dropout draws them: Bernoulli(1 - p) per element"""
    return [torch.bernoulli(torch.full((batch,) + sh, 1.0 - cfg.dropout), generator=generator) for sh in site_shapes(cfg, N)]


def forward(cfg, w, graph, keeps=None, dtype=torch.float64, train=None, device="cpu"):
    """One graph -> dict(trunk [N, D], node_pred [N], graph_pred scalar, attw [N]) in `dtype`.  keeps: None (no dropout) or one 0/1 array
    per site (site_shapes; with a leading B every output gains a leading B), or a function (activation, site) -> activation that does the
    dropout itself (tools/gnn_ab.py: F.dropout).  train (default: keeps is not None): BatchNorm with the
    batch statistics of the graph (mean and biased variance over the nodes, respectively the edges) instead of the running ones."""
    train = keeps is not None if train is None else train
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

    def lin(v, name):
        return v @ W[name + ".weight"].t() + W[name + ".bias"]

    def norm(v, name):
        return F.layer_norm(v, (v.shape[-1],), W[name + ".weight"], W[name + ".bias"], 1e-5)

    def bn(v, name):  # [B, rows, D]
        if train:
            mean, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
        else:
            mean, var = W[name + ".running_mean"], W[name + ".running_var"]
        return (v - mean) / torch.sqrt(var + 1e-5) * W[name + ".weight"] + W[name + ".bias"]

    def tens(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)[None]

    x = tens(graph["x"])
    N, E = x.shape[1], len(graph["edges"])
    src = torch.from_numpy(graph["edges"][:, 0].astype(np.int64)).to(device)
    dst = torch.from_numpy(graph["edges"][:, 1].astype(np.int64)).to(device)
    deg = tens(graph["deg"])[..., None]
    enc = [norm(lin(torch.relu(lin(tens(graph[k]), k + "1")), k + "2"), k + "_norm") for k in ("lap", "rw")]
    h = torch.cat([lin(x, "in")] + enc, -1)
    ea = norm(lin(torch.relu(lin(tens(graph["edge_attr"]), "ee1")), "ee2"), "ee_norm") if E else None
    for l in range(L):
        p = f"layer.{l}."
        a = norm(h, p + "ln1")
        Ax, Bx, Dx, Ex = (lin(a, p + n) for n in "ABDE")
        agg = torch.zeros_like(Ax)
        if E:
            Ce = lin(ea, p + "C")
            Ce = Ce.expand(Ax.shape[0], -1, -1)
            sigma = torch.sigmoid(Ce + Dx[:, dst] + Ex[:, src])
            agg = agg.index_add(1, dst, sigma * Bx[:, src])
            if l < L - 1:
                ea = bn(lin(torch.relu(lin(torch.cat([Dx[:, dst], Ex[:, src], Ce], -1), p + "eu1")), p + "eu2"), p + "bne")
        h = h + drop(torch.relu(bn(Ax + agg / deg, p + "bnn")), 5 * l)
        a = norm(h, p + "ln2")
        B = a.shape[0]
        q, k, v = (t.reshape(B, N, H, dh).transpose(1, 2) for t in lin(a, p + "in_proj").split(D, -1))
        P = drop(torch.softmax(q @ k.transpose(-1, -2) * cs, -1), 5 * l + 1)
        y = lin((P @ v).transpose(1, 2).reshape(B, N, D), p + "out")
        h = h + (norm(a + drop(y, 5 * l + 2), p + "lna") - a)
        f = drop(F.gelu(lin(norm(h, p + "ln3"), p + "ff1")), 5 * l + 3)
        h = h + drop(lin(f, p + "ff2"), 5 * l + 4)
    trunk = norm(h, "lnf")
    node = torch.sigmoid(lin(drop(torch.relu(lin(trunk, "nh1")), 5 * L), "nh2"))[..., 0]
    attw = torch.softmax(lin(torch.tanh(lin(trunk, "na1")), "na2"), 1)  # [B, N, 1]
    rep = torch.cat([trunk.mean(1), (attw * trunk).sum(1)], -1)
    gp = torch.sigmoid(lin(torch.relu(lin(torch.relu(lin(rep, "cl1")), "cl2")), "cl3"))[:, 0]
    out = {"trunk": trunk, "node_pred": node, "graph_pred": gp, "attw": attw[..., 0]}
    return out if batched else {k: v[0] for k, v in out.items()}


def feats(cfg, n, g):
    return torch.randn((n, cfg.input_dim), generator=g).numpy()


def make_graphs(cfg, N, g):
    """The graphs of one node count: kNN only, and with timestamps (two equal ones; at N = 2 each temporal edge doubles a kNN edge: a
    multi-edge, multiplicity 2 in A)."""
    emb = torch.randn((N, EMB_DIM), generator=g).numpy()
    ts = 1.7e9 + (torch.rand((N,), generator=g).double() * 3 * 86400.0).numpy()
    ts[N // 2] = ts[0]  # equal timestamps
    out = [build_graph(cfg, feats(cfg, N, g), emb), build_graph(cfg, feats(cfg, N, g), emb, ts)]
    if N == 2:  # the kNN edge and the temporal edge that share (src, dst): a multi-edge, multiplicity 2 in A
        pairs = [tuple(e) for e in out[1]["edges"]]
        assert len(pairs) == 4 and sorted(pairs) == [(0, 1), (0, 1), (1, 0), (1, 0)], pairs
        assert out[1]["edge_attr"][:, 1].tolist() == [1.0, 1.0, 0.0, 0.0] and laplacian(2, out[1]["edges"])[0][0, 1] == 2.0
    return out


def edge_tile_graphs(cfg, g):
    """E on both sides of a 16-edge tile: (N, k, timestamps) -> E = 15, 16, 16, 31, 32, 33"""
    out = []
    for N, k, timed in ((5, 3, False), (8, 2, False), (6, 1, True), (11, 1, True), (8, 4, False), (7, 3, True)):
        emb = torch.randn((N, EMB_DIM), generator=g).numpy()
        ts = 1.7e9 + (torch.rand((N,), generator=g).double() * 3 * 86400.0).numpy()
        out.append(build_graph(cfg, feats(cfg, N, g), emb, ts if timed else None, k))
    assert [len(gr["edges"]) for gr in out] == [15, 16, 16, 31, 32, 33]
    return out


def lonely_graph(cfg, g):
    """Eight nodes without timestamps, k = 2: seven close to one direction and one opposite them, which is nobody's neighbour: in-degree 0,
    the clamp to 1 and an empty CSR row."""
    emb = np.zeros((8, EMB_DIM), np.float32)
    emb[:, 0] = 1.0
    emb[:, 1] = np.linspace(-0.3, 0.3, 8)
    emb[3] = -emb[3] - np.float32(0.05)
    gr = build_graph(cfg, feats(cfg, 8, g), emb, None, 2)
    assert gr["csr_ptr"][4] == gr["csr_ptr"][3] and gr["deg"][3] == 1 and not (gr["edges"][:, 1] == 3).any()
    return gr


@dataclasses.dataclass
class Case:
    """One (configuration, graphs, S) of a test module with its float64 references, computed once."""
    name: str
    cfg: object
    weights: dict
    graphs: list
    seeds: list
    S: int
    ref: list = None     # per graph: dict of float64 tensors: trunk [max(S, 1), N, D] and node_mc [S, N], or node_pred, graph_pred, attw
    err: dict = None     # per output: max |float32 - float64| (trunk, attw: relative to max |float64| of the case)
    scale: dict = None   # per output: max |float64| of the case


OUTPUTS = ("trunk", "node_mc", "node_pred", "graph_pred", "attw")
RELATIVE = ("trunk", "attw")


def outputs_of(S):
    return OUTPUTS[:2] if S else ("trunk",) + OUTPUTS[2:]


def make_case(name, cfg, weights, graphs, S, seed=0):
    g = torch.Generator().manual_seed(7919 * len(graphs[0]["x"]) + 10 * S + seed)
    n = len(graphs)
    seeds = [int(v) & M64 for v in torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g).tolist()]
    seeds[0] |= 1 << 63  # the top bit too
    case = Case(name, cfg, weights, graphs, seeds, S, [], {})
    keys = outputs_of(S)
    diff, scale = {k: 0.0 for k in keys}, {k: 0.0 for k in keys}
    for i, gr in enumerate(graphs):
        r64, r32 = {k: [] for k in keys}, {k: [] for k in keys}
        for s in range(max(S, 1)):
            keeps = keep_arrays(cfg, len(gr["x"]), seeds[i], s) if S else None
            a = forward(cfg, weights, gr, keeps, torch.float64)
            b = forward(cfg, weights, gr, keeps, torch.float32)
            a["node_mc"], b["node_mc"] = a["node_pred"], b["node_pred"]
            for k in keys:
                r64[k].append(a[k]), r32[k].append(b[k].double())
        ref = {k: torch.stack(v) for k, v in r64.items()}
        d32 = {k: torch.stack(v) for k, v in r32.items()}
        if S == 0:
            for k in keys[1:]:
                ref[k], d32[k] = ref[k][0], d32[k][0]
        for k in keys:
            diff[k] = max(diff[k], float((d32[k] - ref[k]).abs().max()))
            scale[k] = max(scale[k], float(ref[k].abs().max()))
        case.ref.append(ref)
    case.scale = scale
    case.err = {k: diff[k] / scale[k] if k in RELATIVE else diff[k] for k in keys}
    return case


def make_cases(models):
    """Every case of the forward tests: models {name: (cfg, weights, ...)}.  Per configuration and S: the graphs of every N, and for the
    shipped and the tiny configuration the edge-tile graphs and the graph with a node nobody points at."""
    cases = []
    for name, Ns in N_BY_CONFIG.items():
        cfg, w = models[name][:2]
        for S in S_VALUES:
            for N in Ns:
                if N == gnn.MAX_NODES and S == 2:
                    continue  # MAX_NODES once per mode
                g = torch.Generator().manual_seed(1000 * N + S)
                cases.append(make_case(f"{name}-N{N}-S{S}", cfg, w, make_graphs(cfg, N, g), S))
            if name != "wide":
                g = torch.Generator().manual_seed(77 + S)
                cases.append(make_case(f"{name}-edges-S{S}", cfg, w, edge_tile_graphs(cfg, g) + [lonely_graph(cfg, g)], S))
    return cases


def tolerances(cases):
    """The rule of tcnref.tolerances, unchanged: e_ref is the largest float32-vs-float64 difference of gnnref itself over ALL cases of the
    module (trunk and the attention weights: relative to max |float64| of their case); the code under test may be off from float64 by
    4 e_ref — the same f32 operations in another order — and a sigmoid output by 4 f32 spacings at 1.0 more.
    Returns {output: (tolerance, e_ref)}."""
    out = {}
    for k in OUTPUTS:
        e = max((c.err[k] for c in cases if k in c.err), default=0.0)
        out[k] = (4 * e + (0.0 if k in RELATIVE else PRED_FLOOR), e)
    return out


def check_case(case, got, tols, what, failed=None):
    """got: per graph a dict of the outputs of the code under test, shaped as case.ref; returns {output: error / allowed}.  failed: a
    list that collects (what, case, output, ratio) of every miss instead of the assertion here, for a caller that asserts it is empty
    after every case has printed its figures."""
    ratios = {}
    for k in outputs_of(case.S):
        d = max(float((got[i][k].double().cpu().reshape(case.ref[i][k].shape) - case.ref[i][k]).abs().max()) for i in range(len(case.graphs)))
        bound = tols[k][0] * (case.scale[k] if k in RELATIVE else 1.0)
        ratios[k] = d / bound
    print(f"{what} {case.name}: " + ", ".join(f"{k} |d| / bound {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        if failed is not None and not v <= 1.0:
            failed.append((what, case.name, k, round(v, 3)))
        else:
            assert v <= 1.0, (what, case.name, k, v)
    return ratios


def run_case(scorer, case):
    """The code under test on a case, one call for all graphs and samples: per graph a dict shaped as case.ref, and (node_mc, stats)."""
    b = scorer.batch(case.graphs)
    mc, stats, gp, node, attw, trunk = scorer.forward(b, case.seeds, case.S, trunk=True)
    cut = [int(v) for v in b.node_off]
    got = []
    for i in range(b.n):
        o = {"trunk": trunk[i]}
        if case.S:
            o["node_mc"] = mc[cut[i]:cut[i + 1]].t()
        else:
            o["node_pred"], o["graph_pred"], o["attw"] = node[cut[i]:cut[i + 1]], gp[i], attw[cut[i]:cut[i + 1]]
        got.append(o)
    return got, mc, stats


_SHARED = {}


def shared():
    """({name: (cfg, weights)}, cases): computed once per process, shared by every test module, never changed"""
    if not _SHARED:
        from lmx import checkpoints
        models = {}
        for i, (name, cfg) in enumerate(CONFIGS.items()):
            got, w = checkpoints.gnn_from_state_dict(state_dict(cfg, 71 + i), num_heads=cfg.n_heads, dropout=cfg.dropout)
            assert got == cfg, (got, cfg)
            models[name] = (cfg, w)
        _SHARED["models"], _SHARED["cases"] = models, make_cases(models)
    return _SHARED["models"], _SHARED["cases"]


# ---- the reference's own model, where a checkout of it is at hand ----------------------------------------------------------------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphgps_small_w7.npz")
GOLDEN_CFG = gnn.GnnConfig(input_dim=50, d_model=32, n_heads=2, n_layers=2, pe_dim=8, ff=128)  # what the golden file was recorded with
GOLDEN_SIZES = ((7, False), (17, True), (33, True))  # (nodes, a known cow with timestamps); 7 <= 9: the reference's dense eigh


def reference_main():
    """services/gnn-pipeline/app/main.py of a checkout of the reference, or None: the directory LMX_REFERENCE names, else a checkout
    called `reference` beside this repository."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tree in (os.environ.get("LMX_REFERENCE"), os.path.join(os.path.dirname(root), "reference")):
        path = os.path.join(tree, "services", "gnn-pipeline", "app", "main.py") if tree else None
        if path and os.path.isfile(path):
            return path
    return None


def reference_module():
    """The reference's gnn-pipeline main.py imported under a name of its own, with stand-ins for what it imports from torch_geometric
    (Data; degree, global_mean_pool and global_add_pool written in torch; a SAGPooling whose forward raises, so that the reference's own
    `except` skips the dead branch) and for its NATS client; None where the checkout, scipy or yaml is missing."""
    import importlib.util
    import sys
    import types

    path = reference_main()
    if path is None or importlib.util.find_spec("scipy") is None or importlib.util.find_spec("yaml") is None:
        return None
    name = "lmx_reference_gnn_pipeline_main"
    if name in sys.modules:
        return sys.modules[name]

    class Data:
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def to(self, device):
            return self

    class SAGPooling(torch.nn.Module):
        def __init__(self, *a, **kw):
            super().__init__()

        def forward(self, *a, **kw):
            raise RuntimeError("stand-in: the pooled branch reaches no output")

    def degree(index, num_nodes, dtype=torch.float32):
        return torch.zeros((num_nodes,), dtype=dtype).index_add_(0, index, torch.ones((index.numel(),), dtype=dtype))

    def global_add_pool(x, batch):
        return torch.zeros((int(batch.max()) + 1, x.shape[1]), dtype=x.dtype).index_add_(0, batch, x)

    def global_mean_pool(x, batch):
        return global_add_pool(x, batch) / degree(batch, int(batch.max()) + 1, x.dtype)[:, None]

    mods = {k: types.ModuleType(k) for k in ("torch_geometric", "torch_geometric.data", "torch_geometric.nn", "torch_geometric.utils", "shared",
                                             "shared.utils", "shared.utils.nats_client")}
    mods["torch_geometric.data"].Data = mods["torch_geometric.data"].Batch = Data
    tgn, tgu = mods["torch_geometric.nn"], mods["torch_geometric.utils"]
    tgn.GATConv = tgn.GCNConv = None
    tgn.global_mean_pool, tgn.global_add_pool, tgn.SAGPooling = global_mean_pool, global_add_pool, SAGPooling
    tgu.add_self_loops, tgu.degree = None, degree
    mods["shared.utils.nats_client"].NATSClient = object
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return module


def reference_net(ref, cfg, dropout=None):
    return ref.EnhancedGraphGPS(input_dim=cfg.input_dim, hidden_dim=cfg.d_model, edge_input_dim=3, num_layers=2 * cfg.n_layers, num_heads=cfg.n_heads,
                                dropout=cfg.dropout if dropout is None else dropout, pe_dim=cfg.pe_dim)


def reference_graph(ref, x, emb, ts):
    """the reference's GraphBuilder on one cow's videos (ts: a known cow with timestamps, or None)"""
    N = len(x)
    cows, stamps = (["cow"] * N, [float(t) for t in ts]) if ts is not None else (None, None)
    return ref.GraphBuilder(k_neighbors=K_NEIGHBOURS).build_graph(np.asarray(x), np.asarray(emb), [str(i) for i in range(N)], cows, stamps)


def reference_forward(net, data):
    """net(data) with the raw encodings the reference computed on the way: (result, lap [N, 8] before the abs, rw [N, 16])"""
    seen = {}
    lap_fn, rw_fn = net.lap_pe.compute_laplacian_eigenvectors, net.rw_pe.compute_rwpe

    def lap(edge_index, num_nodes):
        seen["lap"] = lap_fn(edge_index, num_nodes)
        return seen["lap"]

    def rw(edge_index, num_nodes):
        seen["rw"] = rw_fn(edge_index, num_nodes)
        return seen["rw"]

    net.lap_pe.compute_laplacian_eigenvectors, net.rw_pe.compute_rwpe = lap, rw
    try:
        with torch.no_grad():
            res = net(data)
    finally:
        del net.lap_pe.compute_laplacian_eigenvectors, net.rw_pe.compute_rwpe
    return res, seen["lap"].numpy(), seen["rw"].numpy()


def load_golden():
    """(cfg, weights, [case]) of the golden file: each case a dict with the graph as gnnref.build_graph makes it from the recorded inputs,
    `fed`: the same graph with the RECORDED edge attributes and encodings (so that only the network is compared), the reference
    builder's edge_index / edge_attr, its raw lap / rw, and its eval-mode outputs graph_pred, node_pred [N], attw [N]."""
    from lmx import checkpoints

    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    cfg, w = checkpoints.gnn_from_state_dict(sd, num_heads=GOLDEN_CFG.n_heads, dropout=GOLDEN_CFG.dropout)
    assert cfg == GOLDEN_CFG
    cases = []
    for i, (N, timed) in enumerate(GOLDEN_SIZES):
        p = f"g{i}/"
        graph = build_graph(cfg, z[p + "x"], z[p + "emb"], z[p + "ts"] if timed else None)
        fed = dict(graph, edge_attr=z[p + "edge_attr"], lap=np.abs(z[p + "lap"]).astype(np.float32), rw=z[p + "rw"])
        cases.append({"graph": graph, "fed": fed, "edge_index": z[p + "edge_index"], "edge_attr": z[p + "edge_attr"], "lap": z[p + "lap"],
                      "rw": z[p + "rw"], "graph_pred": float(z[p + "graph_pred"]), "node_pred": torch.from_numpy(z[p + "node_pred"]).double(),
                      "attw": torch.from_numpy(z[p + "attw"]).double()})
    return cfg, w, cases


def check_golden(cases, got, w, cfg, what):
    """got: per case (graph_pred, node_pred [N], attw [N]) of the code under test, fed the recorded encodings, against the REFERENCE's
    recorded float32 outputs.  The rule of tolerances(): the recorded outputs and the code under test may each be off from float64 by
    4 e_ref — the restatement's own float32 error over the golden's cases — so they may differ by 8 e_ref, plus 4 float32 spacings on a
    sigmoid output; the attention weights relative to their case's maximum."""
    e = {"graph_pred": 0.0, "node_pred": 0.0, "attw": 0.0}
    for c in cases:
        r64, r32 = forward(cfg, w, c["fed"], None, torch.float64), forward(cfg, w, c["fed"], None, torch.float32)
        c["scale"] = float(r64["attw"].abs().max())
        for k in e:
            e[k] = max(e[k], float((r32[k].double() - r64[k]).abs().max()) / (c["scale"] if k == "attw" else 1.0))
    worst = dict.fromkeys(e, 0.0)
    for c, (gp, node, attw) in zip(cases, got):
        diffs = {"graph_pred": abs(float(gp) - c["graph_pred"]), "node_pred": float((node.double().cpu() - c["node_pred"]).abs().max()),
                 "attw": float((attw.double().cpu() - c["attw"]).abs().max()) / c["scale"]}
        for k, d in diffs.items():
            bound = 8 * e[k] + (0.0 if k == "attw" else PRED_FLOOR)
            worst[k] = max(worst[k], d / bound)
            assert d <= bound, (what, k, d, bound)
    print(f"{what} against the reference's recorded outputs, worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
    return worst


# ---- the weight image (csrc/gnn_image.h) and the service mirror's results tree ----------------------------------------------------------
def bad_images(raw):
    """{name: bytes} of truncated and corrupted copies of a kind-7 image, each refused by lmx_gnn_image_check_host"""
    import struct

    from lmx import native

    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    word = lambda i, v: raw[:48 + 4 * i] + struct.pack("<i", v) + raw[48 + 4 * i + 4:]  # noqa: E731
    return {"cut_header": raw[:40], "cut_config": raw[:70], "cut_directory": raw[:dir_off + 3 * native.ENTRY_BYTES + 17],
            "cut_data": raw[:data_off + (len(raw) - data_off) // 2], "cut_last_byte": raw[:-1],
            "kind": raw[:12] + struct.pack("<I", native.KIND_GFM) + raw[16:], "d_model_40": word(1, 40), "n_heads_0": word(2, 0),
            "n_layers_5": word(3, 5), "n_layers_negative": word(3, -3), "pe_dim_12": word(4, 12), "ff_520": word(5, 520), "edge_dim_4": word(6, 4),
            "reserved_1": word(7, 1), "n_tensors_huge": raw[:20] + struct.pack("<I", 2 ** 20) + raw[24:],
            "offset_wraps": raw[:dir_off + 72] + struct.pack("<Q", 2 ** 64 - 64) + raw[dir_off + 80:],
            "p_nan": raw[:48 + 32] + struct.pack("<d", float("nan")) + raw[48 + 40:]}


BAD_IMAGE_TEXTS = {"kind": "kind 6 is not GNN", "d_model_40": "d_model 40", "n_heads_0": "n_heads 0", "n_layers_5": "n_layers 5",
                   "n_layers_negative": "n_layers -3", "pe_dim_12": "pe_dim 12", "ff_520": "ff 520", "edge_dim_4": "edge_dim 4",
                   "reserved_1": "reserved word", "p_nan": "p nan"}


def results_tree(root, videos, rng):
    """videos: (video_id, cow_id or None, timestamp or None); every video gets the four result files, some with fields missing"""
    import json

    for kind in ("tracking", "tleap", "sam3", "yolo", "dinov3"):
        (root / kind).mkdir(parents=True, exist_ok=True)
    for i, (vid, cow, ts) in enumerate(videos):
        track = {"video_id": vid, "reid_results": [{"cow_id": None}, {"cow_id": cow}] if cow else []}
        if ts is not None:
            track["timestamp"] = ts
        (root / "tracking" / f"{vid}_tracking.json").write_text(json.dumps(track))
        loco = {"back_arch_mean": float(rng.random()), "head_bob_magnitude": float(rng.random()), "stride_fl_mean": float(rng.random())}
        if i % 2:
            loco["lameness_score"] = float(rng.random())
        (root / "tleap" / f"{vid}_tleap.json").write_text(json.dumps({"locomotion_features": loco}))
        (root / "sam3" / f"{vid}_sam3.json").write_text(json.dumps({"features": {"avg_area_ratio": float(rng.random()), "avg_circularity": 0.4}}))
        if i % 3:
            (root / "yolo" / f"{vid}_yolo.json").write_text(json.dumps({"features": {"avg_confidence": float(rng.random())}}))
        (root / "dinov3" / f"{vid}_dinov3.json").write_text(json.dumps({"embedding": [float(v) for v in rng.standard_normal(40 if i % 2 else 20)]}))
