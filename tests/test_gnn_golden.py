"""GraphGPS against the REFERENCE's own EnhancedGraphGPS and GraphBuilder: tests/golden/graphgps_small_w7.npz (454,980 bytes, recorded by
tests/golden/make_golden_graphgps.py) on every machine, and the reference itself where a checkout of it is at hand."""
import numpy as np
import pytest
import torch

import gnnref
from lmx import checkpoints, gnn


@pytest.fixture(scope="module")
def golden():
    return gnnref.load_golden()


def test_golden_state_dict_maps_with_its_dead_keys(golden):
    cfg, w, _ = golden
    z = np.load(gnnref.GOLDEN)
    keys = [k[3:] for k in z.files if k.startswith("sd/")]
    dead = [k for k in keys if k.startswith(checkpoints.GNN_DEAD_PREFIXES) or ".pe_bias." in k or
            k.startswith(("pre_pool_layers.1.local_conv.edge_update.", "pre_pool_layers.1.local_conv.bn_edge."))]
    assert cfg == gnnref.GOLDEN_CFG and len(dead) > 40 and any(k.startswith("post_pool_layers.1.") for k in dead)
    assert "layer.0.eu1.weight" in w and "layer.1.eu1.weight" not in w


def test_builder_and_encodings_equal_the_references(golden):
    cfg, _, cases = golden
    z = np.load(gnnref.GOLDEN)
    for i, (c, (N, timed)) in enumerate(zip(cases, gnnref.GOLDEN_SIZES)):
        ts = z[f"g{i}/ts"] if timed else None
        for graph in (c["graph"], gnn.build_graph(cfg, c["graph"]["x"], z[f"g{i}/emb"], ts)):  # the restatement's and the library's
            assert np.array_equal(graph["edges"].T, c["edge_index"]), N
            # the reference's similarity is a float32 BLAS product of 16 terms of magnitude <= 1 each (unpinned): 16 + 2 roundings of 2^-24
            assert np.abs(graph["edge_attr"] - c["edge_attr"]).max() <= 18 * 2.0 ** -24, N
            assert (np.abs(graph["rw"] - c["rw"]) <= np.spacing(c["rw"])).all(), N
            if N <= 9:  # the reference's dense eigh; above it eigsh from a random start vector: unpinned
                # wherever the spectrum is simple: the columns whose eigenvalue is 1e-6 away from both neighbours (a graph of 7 nodes
                # with 5 neighbours each is nearly complete and has a repeated eigenvalue, whose eigenvectors are any basis of its plane)
                lam = gnnref.lap_pe(N, graph["edges"])[1]
                apart = [j - 1 for j in range(1, N) if lam[j] - lam[j - 1] > 1e-6 and (j == N - 1 or lam[j + 1] - lam[j] > 1e-6)]
                assert len(apart) >= 3, (N, lam)
                assert np.abs(graph["lap"][:, apart] - np.abs(c["lap"][:, apart])).max() <= 1e-6, N


def test_restatement_and_host_forward_reproduce_the_recorded_outputs(golden):
    cfg, w, cases = golden
    for dtype in (torch.float64, torch.float32):
        out = [gnnref.forward(cfg, w, c["fed"], None, dtype) for c in cases]
        gnnref.check_golden(cases, [(o["graph_pred"], o["node_pred"], o["attw"]) for o in out], w, cfg, f"gnnref {dtype}")
    host = gnn.GnnScorer(cfg, w, backend="host")
    gp, node, attw = host.evaluate([c["fed"] for c in cases])
    gnnref.check_golden(cases, list(zip(gp, node, attw)), w, cfg, "host")


# ---- the reference's own model, where it is at hand ------------------------------------------------------------------------------------
def _reference():
    ref = gnnref.reference_module()
    if ref is None:
        pytest.skip("no checkout of the reference beside the repository (or under LMX_REFERENCE), or no scipy / yaml")
    return ref


def test_golden_file_is_what_the_reference_gives():
    ref = _reference()
    z = np.load(gnnref.GOLDEN)
    cfg = gnnref.GOLDEN_CFG
    net = gnnref.reference_net(ref, cfg).eval()
    net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
    for i, (N, timed) in enumerate(gnnref.GOLDEN_SIZES):
        p = f"g{i}/"
        data = gnnref.reference_graph(ref, z[p + "x"], z[p + "emb"], z[p + "ts"] if timed else None)
        assert np.array_equal(data.edge_index.numpy(), z[p + "edge_index"]) and np.array_equal(data.edge_attr.numpy(), z[p + "edge_attr"])
        res, lap, rw = gnnref.reference_forward(net, data)
        assert np.array_equal(rw, z[p + "rw"])
        if N <= 9:  # above it every forward of the reference draws another eigsh start vector
            assert np.array_equal(lap, z[p + "lap"])
            assert np.array_equal(res["node_pred"][:, 0].numpy(), z[p + "node_pred"]) and float(res["graph_pred"]) == float(z[p + "graph_pred"])


def test_the_references_train_mode_forward_agrees_with_the_batch_statistics_path():
    """dropout p = 0 leaves train mode's BatchNorm as the only difference from eval mode: the reference's train-mode node scores against
    the restatement with train=True, fed the encodings the reference computed in that forward"""
    ref = _reference()
    cfg = gnnref.GOLDEN_CFG
    z = np.load(gnnref.GOLDEN)
    net = gnnref.reference_net(ref, cfg, dropout=0.0)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    net.load_state_dict(sd, strict=True)
    _, w = checkpoints.gnn_from_state_dict(sd, num_heads=cfg.n_heads, dropout=cfg.dropout)
    for i, (N, timed) in enumerate(gnnref.GOLDEN_SIZES):
        p = f"g{i}/"
        data = gnnref.reference_graph(ref, z[p + "x"], z[p + "emb"], z[p + "ts"] if timed else None)
        net.train()
        res, lap, rw = gnnref.reference_forward(net, data)
        graph = gnnref.build_graph(cfg, z[p + "x"], z[p + "emb"], z[p + "ts"] if timed else None)
        fed = dict(graph, edge_attr=data.edge_attr.numpy(), lap=np.abs(lap).astype(np.float32), rw=rw)
        r64, r32 = (gnnref.forward(cfg, w, fed, None, t, train=True)["node_pred"] for t in (torch.float64, torch.float32))
        e = float((r32.double() - r64).abs().max())
        d = float((res["node_pred"][:, 0].double() - r64).abs().max())
        d_eval = float((res["node_pred"][:, 0].double() - gnnref.forward(cfg, w, fed, None, torch.float64, train=False)["node_pred"]).abs().max())
        print(f"N = {N}: reference train mode against the batch-statistics path {d:.3g} (restatement's own float32 error {e:.3g}); against the eval path {d_eval:.3g}")
        assert d <= 4 * e + gnnref.PRED_FLOOR and d_eval > 100 * d
