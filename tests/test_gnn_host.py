"""GraphGPS without a GPU (include/lmx.h "GraphGPS"): the plain C++ forward lmx_h_gnn_forward against gnnref in float64 under the rule of
gnnref.tolerances, lmx_h_gnn_graph against the numpy restatement of its pinned rules (the Laplacian encoding by residual, eigenvalues
and |eigenvectors| against numpy's eigh), the key map of an EnhancedGraphGPS state_dict with its dead keys, independence of the batch
position, the refusals, and the Python limits against the header's."""
import os
import re

import numpy as np
import pytest
import torch

import gnnref
from lmx import checkpoints, gnn
from lmx import kernels as K
from tcnref import check_stats

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lmx.h")


@pytest.fixture(scope="module")
def models():
    return {name: (cfg, w, gnn.GnnScorer(cfg, w, backend="host")) for name, (cfg, w) in gnnref.shared()[0].items()}


def test_host_forward_against_float64(models):
    cases = gnnref.shared()[1]
    tols = gnnref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases:", {k: f"{v[1]:.3g}" for k, v in tols.items()})
    worst, failed = {}, []
    for case in cases:
        got, mc, stats = gnnref.run_case(models[case.name.split("-")[0]][2], case)
        for k, v in gnnref.check_case(case, got, tols, "host", failed).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if case.S:
            check_stats(mc, stats, case.S)
    print("worst error / bound:", worst)
    assert not failed, failed


def _graph_inputs():
    """(N, k, embeddings, timestamps or None): every N of the forward tests with and without timestamps, ties in similarity and in time,
    the edge-tile graphs' (N, k), the lonely node, N = 1"""
    g = torch.Generator().manual_seed(11)
    out = []
    for N in (1, 2, 3, 8, 9, 10, 15, 16, 17, 33, gnn.MAX_NODES):
        emb = torch.randn((N, gnnref.EMB_DIM), generator=g).numpy()
        ts = 1.7e9 + (torch.rand((N,), generator=g).double() * 3 * 86400.0).numpy()
        ts[N // 2] = ts[0]
        out += [(N, 5, emb, None), (N, 5, emb, ts)]
    for N, k in ((5, 3), (8, 2), (6, 1), (11, 1), (8, 4), (7, 3)):
        out.append((N, k, torch.randn((N, gnnref.EMB_DIM), generator=g).numpy(), None))
    tie = torch.randn((6, gnnref.EMB_DIM), generator=g).numpy()
    tie[4] = tie[1]  # two nodes every other node sees at exactly the same similarity
    out.append((6, 2, tie, np.zeros((6,), np.float64)))  # and every timestamp equal
    return out


def test_graph_builder_equals_the_numpy_restatement():
    cfg = gnnref.SHIPPED
    simple = total = 0
    for N, k, emb, ts in _graph_inputs():
        x = np.zeros((N, cfg.input_dim), np.float32)
        got, want = gnn.build_graph(cfg, x, emb, ts, k), gnnref.build_graph(cfg, x, emb, ts, k)
        for key in ("edges", "csr_ptr", "csr_edge", "deg"):
            assert np.array_equal(got[key], want[key]), (N, k, key)
        E = len(want["edges"])
        assert E <= 5 * N + 2 * (N - 1) and E <= gnn.MAX_EDGES
        spacing = lambda a: np.spacing(np.abs(a).astype(np.float32))  # noqa: E731
        assert (np.abs(got["edge_attr"] - want["edge_attr"]) <= spacing(want["edge_attr"])).all(), (N, k)
        assert (np.abs(got["rw"] - want["rw"]) <= spacing(want["rw"])).all(), (N, k)
        # the Laplacian encoding: the library's Jacobi eigenpairs by residual, by eigenvalues against numpy's eigh on the lower triangle,
        # and by |v| against eigh's where the neighbouring eigenvalues are apart; lap is their columns 1 .. 8, rounded
        _, _, L = gnnref.lap_pe(N, want["edges"])
        lam, V = K.gnn_laplacian(want["edges"], N)
        lam_np, V_np = np.linalg.eigh(L, UPLO="L")
        norm = np.linalg.norm(L, 2)
        assert (np.diff(lam) >= 0).all() and np.abs(lam - lam_np).max() <= 1e-12, (N, k)
        assert np.linalg.norm(L @ V - V * lam[None, :], axis=0).max() <= 1e-12 * norm, (N, k)
        kk = min(gnn.LAP_K, N - 1)
        assert not got["lap"][:, kk:].any()
        assert np.array_equal(got["lap"][:, :kk], np.abs(V[:, 1:1 + kk]).astype(np.float32)), (N, k)
        if N > 1:
            total += 1
            if np.diff(lam_np).min() > 1e-6:
                simple += 1
                assert np.abs(np.abs(V) - np.abs(V_np)).max() <= 1e-9, (N, k)
    print(f"{simple} of {total} graphs have a simple spectrum")
    assert 2 * simple >= total, (simple, total)


def test_key_map_reads_the_state_dict_and_drops_the_dead_keys_by_prefix():
    cfg = gnnref.WIDE
    sd = gnnref.state_dict(cfg, 5)
    got, w = checkpoints.gnn_from_state_dict(sd, num_heads=cfg.n_heads, dropout=cfg.dropout)
    assert got == cfg
    live = gnnref.state_dict(cfg, 5, dead=False)
    assert len(live) < len(sd)
    got2, w2 = checkpoints.gnn_from_state_dict(live, num_heads=cfg.n_heads, dropout=cfg.dropout)
    assert got2 == cfg and w.keys() == w2.keys() and all(torch.equal(w[k], w2[k]) for k in w)
    # whatever lies under a dead prefix is dropped, whatever its spelling
    sd["pool_layer.pool.some.other.spelling"] = torch.zeros(3)
    sd["post_pool_layers.1.anything"] = torch.zeros(3)
    sd[f"pre_pool_layers.{cfg.n_layers - 1}.local_conv.edge_update.9.weight"] = torch.zeros(3)
    assert checkpoints.gnn_from_state_dict(sd, num_heads=cfg.n_heads, dropout=cfg.dropout)[0] == cfg
    # the first live layer's edge update is NOT dead
    with pytest.raises(K.LmxError, match="pre_pool_layers.0.local_conv.edge_update.0.weight is missing"):
        checkpoints.gnn_from_state_dict({k: v for k, v in live.items() if k != "pre_pool_layers.0.local_conv.edge_update.0.weight"}, cfg.n_heads)
    with pytest.raises(K.LmxError, match="pre_pool_layers.1.local_conv.bn_node.running_var is missing"):
        checkpoints.gnn_from_state_dict({k: v for k, v in live.items() if k != "pre_pool_layers.1.local_conv.bn_node.running_var"}, cfg.n_heads)
    with pytest.raises(K.LmxError, match="stray.weight is neither read"):
        checkpoints.gnn_from_state_dict(dict(live, **{"stray.weight": torch.zeros(1)}), cfg.n_heads)
    legacy = {"input_proj.weight": torch.zeros(32, 64), "layers.0.norm1.weight": torch.zeros(64), "pred_head.0.weight": torch.zeros(32, 64)}
    with pytest.raises(K.LmxError, match="GraphGPS state_dict .*legacy class is not served"):
        checkpoints.gnn_from_state_dict(legacy)
    with pytest.raises(K.LmxError, match="n_heads 3 gives d_model 64"):
        checkpoints.gnn_from_state_dict(live, num_heads=3)
    odd = dict(live)
    odd["pre_pool_layers.0.ffn.0.weight"], odd["pre_pool_layers.0.ffn.0.bias"] = torch.zeros(250, 64), torch.zeros(250)
    with pytest.raises(K.LmxError, match="ff 250"):
        checkpoints.gnn_from_state_dict(odd, cfg.n_heads)
    odd = dict(live)
    odd["pre_pool_layers.1.local_conv.C.weight"] = torch.zeros(64, 3)  # the legacy class's 3-wide C
    with pytest.raises(K.LmxError, match=r"layer.1.C.weight has shape \(64, 3\)"):
        checkpoints.gnn_from_state_dict(odd, cfg.n_heads)
    with pytest.raises(K.LmxError, match="not an EnhancedGraphGPS"):
        checkpoints.gnn_from_state_dict({"a": torch.zeros(1)})


def test_a_graph_does_not_depend_on_its_batch_position_on_the_host(models):
    cfg, _, host = models["wide"]
    g = lambda N, s: gnnref.make_graphs(cfg, N, torch.Generator().manual_seed(s))  # noqa: E731
    mine, others = g(17, 1)[1], [g(2, 2)[0], g(33, 3)[1]]
    alone, alone0 = host.forward([mine], [99], 4, trunk=True), host.forward([mine], None, 0, trunk=True)
    for pos in range(3):
        graphs, seeds = list(others), [1, 2]
        graphs.insert(pos, mine), seeds.insert(pos, 99)
        b = host.batch(graphs)
        cut = slice(int(b.node_off[pos]), int(b.node_off[pos + 1]))
        mc, stats, _, _, _, trunk = host.forward(b, seeds, 4, trunk=True)
        assert torch.equal(mc[cut], alone[0]) and torch.equal(stats[cut], alone[1]) and torch.equal(trunk[pos], alone[5][0])
        _, _, gp, node, attw, _ = host.forward(b, None, 0)
        assert torch.equal(gp[pos], alone0[2][0]) and torch.equal(node[cut], alone0[3]) and torch.equal(attw[cut], alone0[4])
    assert abs(float(alone0[4].double().sum()) - 1.0) <= (17 + 2) * 2.0 ** -24


def test_refusals_on_the_host(models):
    import ctypes as C

    from lmx import _lib

    cfg, _, host = models["shipped"]
    graphs = gnnref.make_graphs(cfg, 7, torch.Generator().manual_seed(2))
    one = gnnref.build_graph(cfg, np.zeros((1, cfg.input_dim), np.float32), np.ones((1, 4), np.float32))
    assert len(one["edges"]) == 0 and not one["lap"].any() and (one["rw"] == 1).all()
    with pytest.raises(K.LmxError, match="N = 1 node: BatchNorm has no batch statistics"):
        host.forward([one], [1], 10)
    gp, node, attw = host.evaluate([one])
    assert float(attw[0][0]) == 1.0 and 0.0 < float(gp[0]) < 1.0
    with pytest.raises(K.LmxError, match="S 1 "):
        host.forward(graphs, [1, 2], 1)
    with pytest.raises(K.LmxError, match=f"a graph of {gnn.MAX_NODES + 1} nodes"):
        gnn.build_graph(cfg, np.zeros((gnn.MAX_NODES + 1, cfg.input_dim), np.float32), np.ones((gnn.MAX_NODES + 1, 4), np.float32))
    with pytest.raises(K.LmxError, match="k = 6 neighbours"):
        gnn.build_graph(cfg, graphs[0]["x"], np.ones((7, 4), np.float32), None, 6)
    lib = _lib.load()
    mc, stats = torch.empty((14, 10)), torch.empty((14, 2))
    sd = np.array([1, 2], np.uint64)

    def refused(b, S, text):
        g = b.struct()
        rc = lib.lmx_h_gnn_forward(C.byref(host.weights), C.byref(g), C.c_void_p(sd.ctypes.data), S, 0.1, K._ptr(mc), K._ptr(stats), None, None, None, None)
        assert rc != 0 and text in lib.lmx_last_error().decode(), lib.lmx_last_error()

    b = host.batch(graphs)
    b.node_off = np.array([0, 7, 8], np.int32)
    refused(b, 10, "graph 1 has N = 1 node")
    b = host.batch(graphs)
    b.edge_dst = b.edge_dst.clone()
    b.edge_dst[3] = 9
    refused(b, 10, "is no edge into node")
    b = host.batch(graphs)
    b.csr_ptr = b.csr_ptr.clone()
    b.csr_ptr[7] -= 1
    refused(b, 10, "csr_ptr runs")


def test_python_limits_equal_the_headers():
    txt = open(HDR).read()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", txt).group(1))  # noqa: E731
    assert (gnn.MAX_NODES, gnn.MAX_EDGES, gnn.MAX_LAYERS, gnn.LAP_K, gnn.RW_K) == tuple(
        value("LMX_GNN_" + n) for n in ("MAX_NODES", "MAX_EDGES", "MAX_LAYERS", "LAP_K", "RW_K"))
    assert gnn.MAX_EDGES == 5 * gnn.MAX_NODES + 2 * (gnn.MAX_NODES - 1)
    from lmx import gfm
    assert gnn.MAX_NODES == gfm.MAX_NODES  # the two graph services accept the same cows
    assert gnnref.SHIPPED.n_sites == 11


def test_weight_image_round_trip_and_refusals(models, tmp_path):
    import struct

    from lmx import native

    for name, (cfg, w, _) in models.items():
        path = tmp_path / f"{name}.lmx"
        size = native.write_gnn_image(cfg, w, path)
        assert size == path.stat().st_size
        i = native.check_gnn_image(path)
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.pe_dim, i.ff, i.edge_dim) == cfg.shape()
        assert (i.max_nodes, i.max_edges, i.p) == (gnn.MAX_NODES, gnn.MAX_EDGES, cfg.dropout)
    raw = (tmp_path / "shipped.lmx").read_bytes()
    assert struct.unpack_from("<I", raw, 12)[0] == native.KIND_GNN == 7
    # every tensor of the packed network is in the file, bit for bit, where its directory entry says; the last layer's edge update is not
    dir_off, _ = struct.unpack_from("<QQ", raw, 24)
    packed = gnn.pack_tensors(*models["shipped"][:2])
    n_tensors = struct.unpack_from("<I", raw, 20)[0]
    assert n_tensors == len(packed) == 20 + 32 + 24 + 16 and "layer.1.eu1_w" not in packed
    seen = set()
    for k in range(n_tensors):
        entry = raw[dir_off + k * native.ENTRY_BYTES:dir_off + (k + 1) * native.ENTRY_BYTES]
        tname = entry[:native.NAME_BYTES].rstrip(b"\0").decode()
        offset, nbytes = struct.unpack_from("<QQ", entry, 72)
        assert raw[offset:offset + nbytes] == packed[tname].tobytes(), tname
        seen.add(tname)
    assert seen == set(packed)
    bad = gnnref.bad_images(raw)
    assert set(gnnref.BAD_IMAGE_TEXTS) <= set(bad)
    for name, data in bad.items():
        path = tmp_path / f"bad_{name}.lmx"
        path.write_bytes(data)
        with pytest.raises(K.LmxError, match=gnnref.BAD_IMAGE_TEXTS.get(name, "gnn image")):
            native.check_gnn_image(path)
    with pytest.raises(K.LmxError):
        native.check_gnn_image(tmp_path / "absent.lmx")
