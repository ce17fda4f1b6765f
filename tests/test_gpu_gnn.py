"""GraphGPS on the device (csrc/gnn.hip; include/lmx.h "GraphGPS"): the device and the host forward against gnnref in float64 under the
rule of gnnref.tolerances over every case, and the properties that need no reference — attention-pool weights that sum to 1,
independence of the batch position, of the neighbours' sizes and of S, two runs that give the same bytes, guard words around every
output, every input and the workspace, n = 0, the refusals, and the spread against torch's own generator."""
import ctypes as C

import numpy as np
import pytest
import torch

import gnnref
from lmx import _lib, gnn
from lmx import kernels as K
from tcnref import check_stats

pytestmark = pytest.mark.gpu
FILL = 0x7FC0DEAD  # a quiet NaN with a payload


@pytest.fixture(scope="module")
def models(cuda):
    return {name: (cfg, w, gnn.GnnScorer(cfg, w, device=cuda), gnn.GnnScorer(cfg, w, backend="host")) for name, (cfg, w) in gnnref.shared()[0].items()}


def test_device_and_host_forward_against_float64(cuda, models):
    """Every case under the rule of gnnref.tolerances.  The hardest is shipped-N2-S10: a graph of two nodes in train mode normalises every
    channel of bn_node and bn_edge over TWO rows, y = +-(d / 2) / sqrt(d^2 / 4 + 1e-5) with d the difference of the rows, a slope of
    1 / (2 sqrt(1e-5)) = 158 at small d, and bn_edge feeds bn_node.  With MFMAs chained through their accumulator operand the device
    missed that case (1.15 x the bound); with every MFMA of a product with weights started from zero and joined by TwoSum (csrc/gnn.hip) it holds it at 0.15."""
    cases = gnnref.shared()[1]
    tols = gnnref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases:", {k: f"{v[1]:.3g}" for k, v in tols.items()})
    worst, failed = {"device": {}, "host": {}}, []
    for case in cases:
        _, _, dev, host = models[case.name.split("-")[0]]
        for who, scorer in (("device", dev), ("host", host)):
            got, mc, stats = gnnref.run_case(scorer, case)
            for k, v in gnnref.check_case(case, got, tols, who, failed).items():
                worst[who][k] = max(worst[who].get(k, 0.0), v)
            if case.S:
                check_stats(mc, stats, case.S)
    print("worst error / bound:", worst)
    assert not failed, failed


def _graphs(cfg, N, seed):
    return gnnref.make_graphs(cfg, N, torch.Generator().manual_seed(seed))


def test_attention_pool_weights_sum_to_one(cuda, models):
    """w_i = e_i / sum: the f32 sum of N terms is off by at most N roundings, which all quotients share, and each quotient adds one"""
    for name, N in (("shipped", 17), ("shipped", gnn.MAX_NODES), ("tiny", 3), ("wide", 33)):
        cfg, _, dev, _ = models[name]
        _, _, attw = dev.evaluate(_graphs(cfg, N, 5))
        for a in attw:
            assert abs(float(a.double().sum()) - 1.0) <= (N + 2) * 2.0 ** -24, (name, N, float(a.double().sum()))


def test_a_graph_does_not_depend_on_its_batch_its_neighbours_or_S(cuda, models):
    for name, N, sizes in (("shipped", 17, (2, gnn.MAX_NODES)), ("tiny", 33, (2, 7)), ("wide", 48, (5, 17))):
        cfg, _, dev, _ = models[name]
        mine = _graphs(cfg, N, 7)[1]
        others = [_graphs(cfg, sizes[0], 8)[0], _graphs(cfg, sizes[1], 9)[1]]
        alone = dev.forward([mine], [99], 10, trunk=True)
        alone0 = dev.forward([mine], None, 0, trunk=True)
        again = dev.forward([mine], [99], 10, trunk=True)
        assert torch.equal(again[0], alone[0]) and torch.equal(again[5][0], alone[5][0])  # the aggregation has one order
        for pos in range(3):
            graphs, seeds = list(others), [1, 2]
            graphs.insert(pos, mine), seeds.insert(pos, 99)
            b = dev.batch(graphs)
            cut = slice(int(b.node_off[pos]), int(b.node_off[pos + 1]))
            mc, stats, _, _, _, trunk = dev.forward(b, seeds, 10, trunk=True)
            assert torch.equal(mc[cut], alone[0]) and torch.equal(stats[cut], alone[1]) and torch.equal(trunk[pos], alone[5][0]), (name, pos)
            _, _, gp, node, attw, trunk = dev.forward(b, None, 0, trunk=True)
            assert torch.equal(gp[pos], alone0[2][0]) and torch.equal(node[cut], alone0[3]) and torch.equal(attw[cut], alone0[4]), (name, pos)
            assert torch.equal(trunk[pos], alone0[5][0]), (name, pos)
        m4, _, _, _, _, t4 = dev.forward([mine], [99], 4, trunk=True)
        assert torch.equal(m4, alone[0][:, :4]) and torch.equal(t4[0], alone[5][0][:4])  # sample s of S = 4 is sample s of S = 10
        assert not torch.equal(dev.forward([mine], [98], 10)[0], alone[0])  # another seed is another draw


def _raw_forward(scorer, batch, seeds, S, mc, stats, gp, node, attw, trunk, ws):
    """lmx_k_gnn_forward into the caller's own buffers"""
    lib = _lib.load()
    sd = np.array(seeds, np.uint64)
    g = batch.struct()
    K.check(lib.lmx_k_gnn_forward(C.byref(scorer.weights), C.byref(g), C.c_void_p(sd.ctypes.data), S, scorer.cfg.dropout, K._ptr(mc), K._ptr(stats),
                                  K._ptr(gp), K._ptr(node), K._ptr(attw), K._ptr(trunk), K._ptr(ws), K._stream(batch.x.device)), "lmx_k_gnn_forward")


def test_padding_does_not_leak_and_guard_words_hold(cuda, models):
    """N = 17 with a neighbour of N = 2 in the same launch: 17 and 2 rows are no multiple of the 16-row tile, 108 and 4 edges none of
    the 16-edge tile.  Nothing outside the outputs and the workspace is written, whatever they held before, every word of an output is,
    and the bytes around the inputs reach no result."""
    cfg, _, dev, _ = models["shipped"]
    graphs, seeds, G = [_graphs(cfg, 17, 3)[1], _graphs(cfg, 2, 4)[1]], [11, 12], 512
    n, nodes, D = 2, 19, cfg.d_model
    lib = _lib.load()
    for S in (3, 0):
        results = []
        for fill_byte in (0x00, 0xFF):
            b = dev.batch(graphs)
            for name in ("x", "lap", "rw", "edge_src", "edge_dst", "edge_attr", "csr_ptr", "csr_edge", "deg"):
                t = getattr(b, name)
                flat = t.reshape(-1)
                pad = max(G // t.element_size(), 16)
                big = torch.empty((pad + flat.numel() + pad,), dtype=t.dtype, device=cuda)
                big.view(torch.uint8).fill_(fill_byte)
                big[pad:pad + flat.numel()].copy_(flat)
                setattr(b, name, big[pad:pad + flat.numel()].view(t.shape))
                setattr(b, "_keep_" + name, big)
            bufs = {}
            counts = (("mc", nodes * S), ("stats", nodes * 2)) if S else (("gp", n), ("node", nodes), ("attw", nodes))
            for name, count in counts + (("trunk", nodes * max(S, 1) * D),):
                buf = torch.full((G + count + G,), FILL, dtype=torch.int32, device=cuda)
                bufs[name] = (buf, buf[G:G + count].view(torch.float32))
            words = int(lib.lmx_gnn_workspace_bytes(n, S, b.max_n, b.max_e, D, cfg.n_layers)) // 4
            wsbuf = torch.full((G + words + G,), FILL, dtype=torch.int32, device=cuda)
            get = lambda k: bufs[k][1] if k in bufs else None  # noqa: E731
            _raw_forward(dev, b, seeds, S, get("mc"), get("stats"), get("gp"), get("node"), get("attw"), get("trunk"), wsbuf[G:G + words])
            assert bool((wsbuf[:G] == FILL).all()) and bool((wsbuf[G + words:] == FILL).all()), "workspace"
            for name, (buf, inner) in bufs.items():
                assert bool((buf[:G] == FILL).all()) and bool((buf[G + inner.numel():] == FILL).all()), name
                assert bool(torch.isfinite(inner).all()), name  # every word inside is written
            results.append({k: v[1].clone() for k, v in bufs.items()})
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), k
        mc, stats, gp, node, attw, trunk = dev.forward(graphs, seeds, S, trunk=True)
        assert torch.equal(torch.cat([t.flatten() for t in trunk]), results[0]["trunk"])
        if S:
            assert torch.equal(mc.flatten(), results[0]["mc"]) and torch.equal(stats.flatten(), results[0]["stats"])
        else:
            assert torch.equal(gp, results[0]["gp"]) and torch.equal(node, results[0]["node"]) and torch.equal(attw, results[0]["attw"])


def test_zero_graphs_and_refusals(cuda, models):
    cfg, _, dev, host = models["shipped"]
    graphs = _graphs(cfg, 7, 2)
    mc, stats = dev.forward([], [], 10)[:2]
    assert tuple(mc.shape) == (0, 10) and tuple(stats.shape) == (0, 2)
    assert tuple(dev.forward([], None, 0)[2].shape) == (0,)
    with pytest.raises(K.LmxError, match="CPU tensor"):
        K.gnn_forward(dev.weights, host.batch(graphs), [1, 2], 10, cfg.dropout)
    with pytest.raises(K.LmxError, match="S 1 "):
        dev.forward(graphs, [1, 2], 1)
    with pytest.raises(K.LmxError, match="seeds"):
        dev.forward(graphs, [1], 10)
    one = gnnref.build_graph(cfg, np.zeros((1, cfg.input_dim), np.float32), np.ones((1, 4), np.float32))
    with pytest.raises(K.LmxError, match="N = 1 node: BatchNorm has no batch statistics"):
        dev.forward([one], [1], 10)
    assert tuple(dev.forward([one], None, 0)[3].shape) == (1,)  # the eval launch takes it
    # the library itself refuses what the Python checks refuse: bad offsets, a bad N, one node with S > 0, a bad S, a bad field, outputs of
    # the other mode
    lib = _lib.load()
    mc, stats = torch.empty((14, 10), device=cuda), torch.empty((14, 2), device=cuda)
    gp, node, attw = torch.empty((2,), device=cuda), torch.empty((14,), device=cuda), torch.empty((14,), device=cuda)
    ws = torch.empty((1 << 20,), dtype=torch.int64, device=cuda)
    sd = np.array([1, 2], np.uint64)

    def refused(w, b, S, text, outs=None):
        g = b.struct()
        o = outs or ((mc, stats, None, None, None) if S else (None, None, gp, node, attw))
        rc = lib.lmx_k_gnn_forward(C.byref(w), C.byref(g), C.c_void_p(sd.ctypes.data), S, 0.1, *[K._ptr(t) for t in o], None, K._ptr(ws), K._stream(cuda))
        assert rc != 0 and text in lib.lmx_last_error().decode(), lib.lmx_last_error()

    N = gnn.MAX_NODES + 1
    for node_off, text in (([1, 8, 15], "not at 0"), ([0, 7, 7], "graph 1 has N = 0 nodes"), ([0, 7, 7 + N], f"N = {N} nodes")):
        b = dev.batch(graphs)
        b.node_off = np.array(node_off, np.int32)
        refused(dev.weights, b, 10, text)
    b = dev.batch(graphs)
    b.node_off = np.array([0, 7, 8], np.int32)
    refused(dev.weights, b, 10, "graph 1 has N = 1 node")
    b = dev.batch(graphs)
    b.edge_off = np.array([0, 5, 3], np.int32)
    refused(dev.weights, b, 10, "edge_off descends at graph 1")
    b.edge_off = np.array([0, 5, 5 + gnn.MAX_EDGES + 1], np.int32)
    refused(dev.weights, b, 10, f"E = {gnn.MAX_EDGES + 1} edges")
    refused(dev.weights, dev.batch(graphs), 1, "S 1 ")
    refused(dev.weights, dev.batch(graphs), 10, "eval mode only, S = 10", (mc, stats, gp, None, None))
    refused(dev.weights, dev.batch(graphs), 0, "S > 0 only", (mc, None, gp, node, attw))
    w = type(dev.weights).from_buffer_copy(bytes(dev.weights))
    w.pe_dim = 12
    refused(w, dev.batch(graphs), 10, "pe_dim 12")
    torch.cuda.synchronize(cuda)


def test_spread_agrees_with_torchs_generator(cuda, models):
    """Parity with torch's generator is statistical: gnnref in float32 under 2000 draws of torch.bernoulli masks (what nn.Dropout draws in
    train mode), batch statistics in BatchNorm, against the device's mean over S = 200 of the library's own bits, for the node whose
    score spreads most.  5 standard errors of a mean of 200, from the torch run's own standard deviation."""
    cfg, w, dev, _ = models["shipped"]
    graph = _graphs(cfg, 17, 4)[1]
    g = torch.Generator().manual_seed(0)
    preds = torch.cat([gnnref.forward(cfg, w, graph, gnnref.bernoulli_keeps(cfg, 17, 250, g), torch.float32)["node_pred"] for _ in range(8)]).double()
    node = int(preds.std(0).argmax())
    mean, std = float(preds[:, node].mean()), float(preds[:, node].std())
    got_mean, got_std = dev.score([graph], [gnn.graph_seed("video")], 200)[0]
    se = std / 200 ** 0.5
    print(f"torch: mean {mean:.5f} std {std:.5f} over 2000; device: mean {float(got_mean[node]):.5f} std {float(got_std[node]):.5f} over 200; se {se:.5f}")
    assert std > 0 and abs(float(got_mean[node]) - mean) <= 5 * se


def test_golden_outputs_of_the_reference_are_reproduced(cuda):
    """The GPU machine has no checkout of the reference: tests/golden/graphgps_small_w7.npz holds what the reference's own
    EnhancedGraphGPS gave for three graphs, and the device, fed the recorded encodings, reproduces it within the rule
    (gnnref.check_golden), all three in one launch."""
    cfg, w, cases = gnnref.load_golden()
    gp, node, attw = gnn.GnnScorer(cfg, w, device=cuda).evaluate([c["fed"] for c in cases])
    gnnref.check_golden(cases, list(zip(gp, node, attw)), w, cfg, "device")


def test_native_handle_gives_the_scorers_bits(cuda, models, tmp_path):
    from lmx import native

    cfg, w, dev, _ = models["shipped"]
    path = tmp_path / "gnn.lmx"
    native.write_gnn_image(cfg, w, path)
    graphs = [_graphs(cfg, 17, 3)[1], _graphs(cfg, 2, 4)[0], _graphs(cfg, gnn.MAX_NODES, 5)[1]]
    seeds = [gnn.graph_seed(v) for v in ("a", "b", "c")]
    edges = sum(len(g["edges"]) for g in graphs)
    with native.NativeGnn(path, max_graphs=4, max_nodes_total=120, max_edges_total=edges, max_samples=10, device=cuda) as h:
        i = h.info
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.pe_dim, i.ff, i.edge_dim) == cfg.shape()
        assert (i.max_nodes, i.max_edges, i.max_graphs, i.max_nodes_total, i.max_edges_total, i.max_samples, i.p) == (
            gnn.MAX_NODES, gnn.MAX_EDGES, 4, 120, edges, 10, cfg.dropout)
        mc, stats = dev.forward(graphs, seeds, 10)[:2]
        for m, s, _, _, _ in (h.score(graphs, seeds, 10), h.score_host(graphs, seeds, 10)):
            assert torch.equal(m.cpu(), mc.cpu()) and torch.equal(s.cpu(), stats.cpu())
        _, _, gp, node, attw, _ = dev.forward(graphs, None, 0)
        for _, _, g0, n0, a0 in (h.score(graphs, None, 0), h.score_host(graphs, None, 0)):
            assert torch.equal(g0.cpu(), gp.cpu()) and torch.equal(n0.cpu(), node.cpu()) and torch.equal(a0.cpu(), attw.cpu())
        with pytest.raises(K.LmxError, match="n = 5 graphs"):
            h.score(graphs[1:2] * 5, [1] * 5)
        with pytest.raises(K.LmxError, match="192 nodes in all"):
            h.score([graphs[2], graphs[2], graphs[1]], [1, 2, 3])
        with pytest.raises(K.LmxError, match="edges in all"):
            h.score([graphs[2], graphs[0], graphs[1], graphs[1]], [1, 2, 3, 4])  # 116 nodes, two edges too many
        with pytest.raises(K.LmxError, match="S = 11"):
            h.score(graphs, seeds, 11)
        with pytest.raises(K.LmxError, match="S 1 "):
            h.score(graphs, seeds, 1)
    torch.cuda.synchronize(cuda)
