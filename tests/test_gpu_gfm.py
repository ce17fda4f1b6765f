"""The graph transformer on the device (csrc/gfm.hip; include/lmx.h "The graph transformer"): the device and the host forward against
gfmref in float64 under the rule of gfmref.tolerances over every case, and the properties that need no reference — attention rows that
sum to 1, independence of the batch position, of the neighbours' sizes and of S, guard words around every output and input, n = 0,
the refusals, and the spread against torch's own generator."""
import ctypes as C

import numpy as np
import pytest
import torch

import gfmref
from lmx import _lib, checkpoints, gfm, native
from lmx import kernels as K
from tcnref import check_stats

pytestmark = pytest.mark.gpu
FILL = 0x7FC0DEAD  # a quiet NaN with a payload


@pytest.fixture(scope="module")
def models(cuda):
    out = {}
    for i, (name, cfg) in enumerate(gfmref.CONFIGS.items()):
        got, w = checkpoints.gfm_from_state_dict(gfmref.state_dict(cfg, 51 + i), num_heads=cfg.n_heads, dropout=cfg.dropout)
        assert got == cfg
        out[name] = (cfg, w, gfm.GfmScorer(cfg, w, device=cuda), gfm.GfmScorer(cfg, w, backend="host"))
    return out


@pytest.fixture(scope="module")
def cases(models):
    """(configuration, N, S) with the graphs of gfmref.make_graphs each, the path graph of 14 nodes with N = 14 and N = 6; the float64
    and float32 references are computed once and never changed"""
    return [gfmref.make_case(f"{name}-N{N}-S{S}", models[name][0], models[name][1], N, S, path=N in (14, 6))
            for name, Ns in gfmref.N_BY_CONFIG.items() for N in Ns for S in gfmref.S_VALUES]


def test_device_and_host_forward_against_float64(cuda, models, cases):
    tols = gfmref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases:", {k: f"{v[1]:.3g}" for k, v in tols.items()})
    worst = {"device": {}, "host": {}}
    for case in cases:
        _, _, dev, host = models[case.name.split("-")[0]]
        for who, scorer in (("device", dev), ("host", host)):
            got, pred, stats = gfmref.run_case(scorer, case)
            for k, v in gfmref.check_case(case, got, tols, who).items():
                worst[who][k] = max(worst[who].get(k, 0.0), v)
            check_stats(pred, stats, case.S)
    print("worst error / bound:", worst)


def _graphs(cfg, N, seed):
    return gfmref.make_graphs(cfg, N, torch.Generator().manual_seed(seed))


def test_attention_rows_sum_to_one(cuda, models):
    """Every row of the last layer's P sums to 1 in every head, so node i's entries of the attention columns of ALL targets add up to 1
    and the whole matrix to N.  One launch: the graph N times, once per target."""
    for name, N in (("shipped", 17), ("tiny", 33), ("wide", 5)):
        cfg, _, dev, _ = models[name]
        for graph in _graphs(cfg, N, 5)[:2]:
            attn = dev.forward([graph] * N, None, 0, targets=list(range(N)))[3].double().cpu().reshape(N, N)  # [target, node]
            # a row's f32 sum is off by at most N roundings, which all its quotients share; the quotients, the H additions of the heads
            # and the division by H add one rounding each to values that sum to 1
            assert (attn.sum(0) - 1).abs().max() <= (N + cfg.n_heads + 2) * 2.0 ** -24, (name, N, attn.sum(0))
            assert abs(float(attn.sum()) - N) <= N * 2.0 ** -21


def test_a_graph_does_not_depend_on_its_batch_its_neighbours_or_S(cuda, models):
    for name, N, sizes in (("shipped", 17, (2, gfm.MAX_NODES)), ("tiny", 33, (1, 7)), ("wide", 48, (5, 17))):
        cfg, _, dev, _ = models[name]
        mine = _graphs(cfg, N, 7)[1]
        others = [_graphs(cfg, sizes[0], 8)[0], _graphs(cfg, sizes[1], 9)[1]]
        alone = dev.forward([mine], [99], 10, trunk=True, vn=True)
        alone0 = dev.forward([mine], None, 0, targets=[N // 2], node=True)
        for pos in range(3):
            graphs, seeds, targets = list(others), [1, 2], [0, 0]
            graphs.insert(pos, mine), seeds.insert(pos, 99), targets.insert(pos, N // 2)
            pred, stats, _, _, trunk, vn = dev.forward(graphs, seeds, 10, trunk=True, vn=True)
            assert torch.equal(pred[pos], alone[0][0]) and torch.equal(stats[pos], alone[1][0]), (name, pos)
            assert torch.equal(trunk[pos], alone[4][0]) and torch.equal(vn[pos], alone[5][0]), (name, pos)
            b = dev.batch(graphs, targets)
            pred0, _, node0, attn0, _, _ = dev.forward(b, None, 0, node=True)
            cut = slice(int(b.node_off[pos]), int(b.node_off[pos + 1]))
            assert torch.equal(pred0[pos], alone0[0][0]) and torch.equal(node0[cut], alone0[2]) and torch.equal(attn0[cut], alone0[3]), (name, pos)
        p4, _, _, _, t4, _ = dev.forward([mine], [99], 4, trunk=True)
        assert torch.equal(p4[0], alone[0][0, :4]) and torch.equal(t4[0], alone[4][0][:4])
        assert not torch.equal(dev.forward([mine], [98], 10)[0], alone[0])  # another seed is another draw


def _raw_forward(scorer, batch, seeds, S, pred, stats, node, attn, trunk, vn):
    """lmx_k_gfm_forward into the caller's own buffers"""
    lib = _lib.load()
    sd = np.array(seeds, np.uint64)
    dev = batch.x.device
    ws = torch.empty((int(lib.lmx_gfm_workspace_bytes(batch.n, batch.cells, scorer.cfg.n_heads)) // 8 + 2,), dtype=torch.int64, device=dev)
    g = batch.struct()
    K.check(lib.lmx_k_gfm_forward(C.byref(scorer.weights), C.byref(g), C.c_void_p(sd.ctypes.data), S, scorer.cfg.dropout, K._ptr(pred), K._ptr(stats),
                                  K._ptr(node), K._ptr(attn), K._ptr(trunk), K._ptr(vn), K._ptr(ws), K._stream(dev)), "lmx_k_gfm_forward")


def test_padding_does_not_leak_and_guard_words_hold(cuda, models):
    """N = 17 with a neighbour of N = 2 in the same launch: 18 and 3 rows are no multiple of the 16-row tile, the rest of the tiles
    exists in LDS only.  Nothing outside the outputs is written, whatever they held before, every word inside is, and the bytes around
    the inputs reach no result."""
    cfg, _, dev, _ = models["shipped"]
    graphs, seeds, G = [_graphs(cfg, 17, 3)[1], _graphs(cfg, 2, 4)[1]], [11, 12], 512
    n, nodes, D = 2, 19, cfg.d_model
    for S in (3, 0):
        results = []
        for fill_byte in (0x00, 0xFF):
            b = dev.batch(graphs, [5, 1])
            for name in ("x", "timestamps", "has_time", "deg_in", "deg_out", "idx", "win", "edge_attr", "target"):
                t = getattr(b, name)
                flat = t.reshape(-1)
                pad = max(G // t.element_size(), 16)
                big = torch.empty((pad + flat.numel() + pad,), dtype=t.dtype, device=cuda)
                big.view(torch.uint8).fill_(fill_byte)
                big[pad:pad + flat.numel()].copy_(flat)
                setattr(b, name, big[pad:pad + flat.numel()].view(t.shape))
                setattr(b, "_keep_" + name, big)
            bufs = {}
            counts = (("pred", n * max(S, 1)), ("stats", n * 2), ("trunk", nodes * max(S, 1) * D), ("vn", n * max(S, 1) * D))
            for name, count in counts + ((("node", nodes), ("attn", nodes)) if S == 0 else ()):
                buf = torch.full((G + count + G,), FILL, dtype=torch.int32, device=cuda)
                bufs[name] = (buf, buf[G:G + count].view(torch.float32))
            _raw_forward(dev, b, seeds, S, bufs["pred"][1], bufs["stats"][1], bufs["node"][1] if S == 0 else None,
                         bufs["attn"][1] if S == 0 else None, bufs["trunk"][1], bufs["vn"][1])
            for name, (buf, inner) in bufs.items():
                assert bool((buf[:G] == FILL).all()) and bool((buf[G + inner.numel():] == FILL).all()), name
                assert bool(torch.isfinite(inner).all()), name  # every word inside is written
            results.append({k: v[1].clone() for k, v in bufs.items()})
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), k
        pred, stats, node, attn, trunk, vn = dev.forward(dev.batch(graphs, [5, 1] if S == 0 else None), seeds, S, node=S == 0, trunk=True, vn=True)
        assert torch.equal(pred.flatten(), results[0]["pred"]) and torch.equal(stats.flatten(), results[0]["stats"])
        assert torch.equal(torch.cat([t.flatten() for t in trunk]), results[0]["trunk"]) and torch.equal(vn.flatten(), results[0]["vn"])
        assert S or (torch.equal(node, results[0]["node"]) and torch.equal(attn, results[0]["attn"]))


def test_zero_graphs_and_refusals(cuda, models):
    cfg, _, dev, host = models["shipped"]
    graphs = _graphs(cfg, 7, 2)[:2]
    pred, stats = dev.forward([], [], 10)[:2]
    assert tuple(pred.shape) == (0, 10) and tuple(stats.shape) == (0, 2)
    with pytest.raises(K.LmxError, match="CPU tensor"):
        K.gfm_forward(dev.weights, host.batch(graphs), [1, 2], 10, cfg.dropout)
    with pytest.raises(K.LmxError, match="S 1 "):
        dev.forward(graphs, [1, 2], 1)
    with pytest.raises(K.LmxError, match="eval mode only, S = 10"):
        dev.forward(graphs, [1, 2], 10, node=True)
    with pytest.raises(K.LmxError, match="eval mode only, S = 10"):
        K.gfm_forward(dev.weights, dev.batch(graphs, [0, 0]), [1, 2], 10, cfg.dropout, attn=True)
    with pytest.raises(K.LmxError, match="seeds"):
        dev.forward(graphs, [1], 10)
    big = dict(graphs[0])
    N = gfm.MAX_NODES + 1
    big.update(x=np.zeros((N, cfg.input_dim), np.float32), timestamps=None, deg_in=np.zeros((N,), np.uint8), deg_out=np.zeros((N,), np.uint8),
               idx=np.ones((N, N), np.uint8), win=np.full((N, N), -1, np.int32), edges=np.zeros((0, 2), np.int32), edge_attr=np.zeros((0, 3), np.float32))
    with pytest.raises(K.LmxError, match=f"N = {N} nodes"):
        dev.forward([big], [1], 10)
    # the library itself refuses what the Python checks refuse: bad offsets, a bad N, a bad S and a bad field straight to the entry point
    lib = _lib.load()
    pred, stats = torch.empty((2, 10), device=cuda), torch.empty((2, 2), device=cuda)
    ws = torch.empty((4096,), dtype=torch.int64, device=cuda)
    sd = np.array([1, 2], np.uint64)

    def refused(w, b, S, text):
        g = b.struct()
        rc = lib.lmx_k_gfm_forward(C.byref(w), C.byref(g), C.c_void_p(sd.ctypes.data), S, 0.1, K._ptr(pred), K._ptr(stats), None, None, None, None,
                                   K._ptr(ws), K._stream(cuda))
        assert rc != 0 and text in lib.lmx_last_error().decode(), lib.lmx_last_error()

    for node_off, text in (([1, 8, 15], "not at 0"), ([0, 7, 7], "graph 1 has N = 0 nodes"), ([0, 7, 7 + N], f"N = {N} nodes")):
        b = dev.batch(graphs)
        b.node_off = np.array(node_off, np.int32)
        refused(dev.weights, b, 10, text)
    b = dev.batch(graphs)
    b.edge_off = np.array([0, 5, 3], np.int32)
    refused(dev.weights, b, 10, "edge_off descends at graph 1")
    refused(dev.weights, dev.batch(graphs), 1, "S 1 ")
    w = type(dev.weights).from_buffer_copy(bytes(dev.weights))
    w.ff = 520
    refused(w, dev.batch(graphs), 10, "ff 520")
    torch.cuda.synchronize(cuda)


def test_spread_agrees_with_torchs_generator(cuda, models):
    """Parity with torch's generator is statistical: gfmref in float32 under 2000 draws of torch.bernoulli masks (what nn.Dropout draws
    in train mode) against the device's mean over S = 200 of the library's own bits.  5 standard errors of a mean of 200, from the torch
    run's own standard deviation."""
    cfg, w, dev, _ = models["shipped"]
    graph = _graphs(cfg, 17, 4)[1]
    g = torch.Generator().manual_seed(0)
    preds = torch.cat([gfmref.forward(cfg, w, graph, gfmref.bernoulli_keeps(cfg, 17, 250, g), torch.float32)["pred"] for _ in range(8)]).double()
    mean, std = float(preds.mean()), float(preds.std())
    got_mean, got_std, _ = dev.score([graph], [gfm.graph_seed("video")], 200)
    se = std / 200 ** 0.5
    print(f"torch: mean {mean:.5f} std {std:.5f} over 2000; device: mean {float(got_mean[0]):.5f} std {float(got_std[0]):.5f} over 200; se {se:.5f}")
    assert std > 0 and abs(float(got_mean[0]) - mean) <= 5 * se


def test_golden_outputs_of_the_reference_are_reproduced(cuda):
    """The GPU machine has no checkout of the reference: tests/golden/graphormer_small_w5.npz holds what the reference's own
    CowLamenessGraphormer gave for three graphs, and the device reproduces it within the rule (gfmref.check_golden), all three in one launch."""
    cfg, w, cases = gfmref.load_golden()
    dev = gfm.GfmScorer(cfg, w, device=cuda)
    pred, nodes, attn = dev.node_scores([c["graph"] for c in cases], [c["target"] for c in cases])
    gfmref.check_golden(cases, list(zip(pred, nodes, attn)), w, cfg, "device")


def test_native_handle_gives_the_scorers_bits(cuda, models, tmp_path):
    cfg, w, dev, _ = models["shipped"]
    path = tmp_path / "gfm.lmx"
    native.write_gfm_image(cfg, w, path)
    graphs = [_graphs(cfg, 17, 3)[1], _graphs(cfg, 2, 4)[0], _graphs(cfg, gfm.MAX_NODES, 5)[1]]
    seeds, targets = [gfm.graph_seed(v) for v in ("a", "b", "c")], [5, 1, 90]
    with native.NativeGfm(path, max_graphs=4, max_nodes_total=120, max_samples=10, device=cuda) as h:
        i = h.info
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.ff, i.edge_dim, i.max_degree, i.max_spd) == cfg.shape()
        assert (i.max_nodes, i.max_graphs, i.max_nodes_total, i.max_samples, i.p) == (gfm.MAX_NODES, 4, 120, 10, cfg.dropout)
        pred, stats = dev.forward(graphs, seeds, 10)[:2]
        for m, s, p, _, _ in (h.score(graphs, seeds, 10), h.score_host(graphs, seeds, 10)):
            assert torch.equal(p.cpu(), pred.cpu()) and torch.equal(m.cpu(), stats[:, 0].cpu()) and torch.equal(s.cpu(), stats[:, 1].cpu())
        pred0, _, node0, attn0, _, _ = dev.forward(dev.batch(graphs, targets), None, 0, node=True)
        for m, s, p, nd, at in (h.score(graphs, None, 0, targets, node=True), h.score_host(graphs, None, 0, targets, node=True)):
            assert torch.equal(p.cpu(), pred0.cpu()) and torch.equal(nd.cpu(), node0.cpu()) and torch.equal(at.cpu(), attn0.cpu())
        with pytest.raises(K.LmxError, match="n = 5 graphs"):
            h.score(graphs[1:2] * 5, [1] * 5)
        with pytest.raises(K.LmxError, match="192 nodes in all"):
            h.score([graphs[2], graphs[2], graphs[1]], [1, 2, 3])
        with pytest.raises(K.LmxError, match="S = 11"):
            h.score(graphs, seeds, 11)
        with pytest.raises(K.LmxError, match="S 1 "):
            h.score(graphs, seeds, 1)
        with pytest.raises(K.LmxError, match="eval mode only"):
            h.score(graphs, seeds, 10, node=True)
    torch.cuda.synchronize(cuda)
