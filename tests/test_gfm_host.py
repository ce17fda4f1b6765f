"""The graph transformer without a GPU (include/lmx.h "The graph transformer"; csrc/host_gfm.cpp, lmx/gfm.py):
  * lmx_h_gfm_forward against gfmref in float64 under the tolerance rule of gfmref.tolerances, over every case;
  * lmx_h_gfm_graph equal to the numpy restatement of the pinned rules: edges, attributes, degrees, idx, the winner matrix, with
    all-zero embeddings (every similarity ties) and all-equal timestamps among the inputs;
  * gfm_from_state_dict: the reference's 220 keys, the configuration from the shapes, the refusals;
  * the configuration and call refusals with the field named, in Python and handed straight to the entry point;
  * the golden file recorded from the reference's own CowLamenessGraphormer and GraphormerGraphBuilder (tests/golden/
    make_golden_graphormer.py): the restatement, the host forward and the graph builder against the reference's recorded outputs;
  * where a checkout of the reference (beside the repository, or where LMX_REFERENCE names it) and networkx are present: the reference's
    own model and builder run live in eval mode against the float64 restatement, and the golden file is what they give today."""
import asyncio
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import gfmref
import struct

from lmx import _lib, checkpoints, gfm, native
from lmx import kernels as K


@pytest.fixture(scope="module")
def models():
    out = {}
    for i, (name, cfg) in enumerate(gfmref.CONFIGS.items()):
        sd = gfmref.state_dict(cfg, 41 + i)
        got, w = checkpoints.gfm_from_state_dict(sd, num_heads=cfg.n_heads, dropout=cfg.dropout)
        assert got == cfg
        out[name] = (cfg, w, gfm.GfmScorer(cfg, w, backend="host"), sd)
    return out


# ---- the host forward ----------------------------------------------------------------------------------------------------------------
def test_host_forward_against_float64(models):
    cases = [gfmref.make_case(f"{name}-N{N}-S{S}", models[name][0], models[name][1], N, S, path=N in (14, 6))
             for name, Ns in gfmref.N_BY_CONFIG.items() for N in Ns for S in gfmref.S_VALUES]
    tols = gfmref.tolerances(cases)
    print(f"e_ref over {len(cases)} cases:", {k: f"{v[1]:.3g}" for k, v in tols.items()})
    worst = {}
    for case in cases:
        host = models[case.name.split("-")[0]][2]
        got, pred, stats = gfmref.run_case(host, case)
        for k, v in gfmref.check_case(case, got, tols, "host").items():
            worst[k] = max(worst.get(k, 0.0), v)
        p = pred.double()
        if case.S:
            assert (stats[:, 0].double() - p.mean(1)).abs().max() <= 4 * 2.0 ** -24 and (stats[:, 1].double() - p.std(1)).abs().max() <= 8 * 2.0 ** -24
        else:
            assert torch.equal(stats[:, 0], pred[:, 0]) and not stats[:, 1].any()
    print("worst error / bound:", worst)


def test_cases_hold_what_they_are_for(models):
    """the clamps bite in `tiny`, unreachable pairs exist in the cluster graphs, a duplicate edge exists at N = 2, the path graph goes
    beyond max_spd, equal timestamps and a span above 365 days are there"""
    cfg = models["tiny"][0]
    g = torch.Generator().manual_seed(3)
    plain, timed, split, path = gfmref.make_graphs(cfg, 33, g, path=True)
    assert timed["deg_out"].max() == cfg.max_degree and (np.bincount(timed["edges"][:, 0]) > cfg.max_degree).any()
    assert (plain["idx"] == cfg.max_spd + 1).any() and (plain["idx"] == 2).any() and (np.diag(plain["idx"]) == 1).all()
    full = gfmref.make_graphs(models["shipped"][0], 33, g, path=True)
    assert (full[2]["idx"][:16, 16:] == 11).all() and full[2]["idx"][:16, :16].max() < 11  # two components
    assert full[3]["idx"][0, 13] == 11 and full[3]["idx"][0, 9] == 10 and full[3]["idx"][0, 10] == 11
    ts = timed["timestamps"]
    assert ts[33 // 2] == ts[0] and ts.max() - ts.min() > 365 * 86400
    two = gfmref.make_graphs(cfg, 2, g)[1]
    assert len(two["edges"]) == 4 and (two["win"] == np.array([[-1, 2], [3, -1]])).all()  # the temporal edges win


# ---- the graph builder -----------------------------------------------------------------------------------------------------------------
def _same_graph(a, b):
    for key in ("edges", "edge_attr", "deg_in", "deg_out", "idx", "win"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("name", ["shipped", "tiny"])
def test_graph_builder_equals_the_numpy_restatement(models, name):
    cfg = models[name][0]
    g = torch.Generator().manual_seed(11)
    for N in (1, 2, 3, 7, 16, 33, gfm.MAX_NODES):
        x = np.zeros((N, cfg.input_dim), np.float32)
        emb = torch.randn((N, gfmref.EMB_DIM), generator=g).numpy()
        ts = (1.7e9 + torch.rand((N,), generator=g) * 40 * 86400.0).numpy().astype(np.float32)
        ts[N // 2] = ts[0]
        dup = emb.copy()
        dup[N // 3] = dup[0]  # two nodes with the same embedding: exact ties in every row
        for e, t, k in ((emb, None, 5), (emb, ts, 5), (emb, ts, 0), (emb, ts, 200), (dup, ts, 3), (np.zeros_like(emb), np.zeros_like(ts), 5),
                        (np.zeros_like(emb), None, 5), (emb, np.full_like(ts, 7.0), 2)):
            _same_graph(gfm.build_graph(cfg, x, e, t, k), gfmref.build_graph(cfg, x, e, t, k))
    zero = gfm.build_graph(cfg, np.zeros((6, cfg.input_dim), np.float32), np.zeros((6, 4), np.float32), np.zeros((6,), np.float32), 2)
    # every similarity ties: the two HIGHEST other indices, in ascending order; equal timestamps: the index order
    assert zero["edges"][:4].tolist() == [[0, 4], [0, 5], [1, 4], [1, 5]] and zero["edges"][12:16].tolist() == [[0, 1], [1, 0], [1, 2], [2, 1]]
    assert (zero["edge_attr"][:12] == np.array([0, 1, 0], np.float32)).all() and (zero["edge_attr"][12:] == np.array([1, 0, 1], np.float32)).all()


def test_graph_builder_refusals(models):
    cfg = models["shipped"][0]
    big = np.zeros((gfm.MAX_NODES + 1, 4), np.float32)
    with pytest.raises(K.LmxError, match=f"{gfm.MAX_NODES + 1} nodes.*{gfm.MAX_NODES}"):
        gfm.build_graph(cfg, np.zeros((gfm.MAX_NODES + 1, cfg.input_dim), np.float32), big)
    with pytest.raises(K.LmxError, match="N 96 outside 1 .. 95"):
        K.gfm_graph(big, None, 5, 50, 10)
    lib, one = _lib.load(), np.zeros((4, 4), np.float32)
    rc = lib.lmx_h_gfm_graph(one.ctypes.data, None, 4, 4, 5, 300, 10, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                             one.ctypes.data, one.ctypes.data, one.ctypes.data)
    assert rc != 0 and b"max_degree 300" in lib.lmx_last_error()


# ---- the key map -------------------------------------------------------------------------------------------------------------------------
def test_key_map_reads_the_references_220_keys(models):
    cfg, w, _, sd = models["shipped"]
    assert len(sd) == 220 and "encodings.temporal_enc.div_term" in sd and "input_proj.0.weight" in sd and "node_pred.3.bias" in sd
    assert sum(v.numel() for k, v in sd.items() if k != "encodings.temporal_enc.div_term") == 2097195  # the reference's parameter count
    assert cfg == gfm.GfmConfig()
    used = {theirs for theirs, _ in checkpoints.GFM_KEYS} | {("encoder." + t).format(i=i) for t, _ in checkpoints.GFM_LAYER_KEYS
                                                              for i in range(cfg.n_layers)}
    read = {k.rsplit(".", 1)[0] for k in sd if k.endswith((".weight", ".bias")) and "encoder.weight" not in k and "spd_bias" not in k}
    assert read == used
    assert torch.equal(w["layer.5.vq.weight"], sd["encoder.virtual_node_layers.5.vn_attention.q_proj.weight"])
    assert torch.equal(w["layer.2.vn"], sd["encoder.virtual_node_layers.2.virtual_node"][0])
    for key in ("encodings.temporal_enc.div_term", "encoder.layers.3.ffn.3.bias", "encoder.virtual_node_layers.0.virtual_node"):
        with pytest.raises(K.LmxError, match=key.replace(".", r"\.")):
            checkpoints.gfm_from_state_dict({k: v for k, v in sd.items() if k != key})
    with pytest.raises(K.LmxError, match="n_heads 5"):
        checkpoints.gfm_from_state_dict(sd, num_heads=5)
    with pytest.raises(K.LmxError, match="not a CowLamenessGraphormer"):
        checkpoints.gfm_from_state_dict({"x": torch.zeros(1)})
    # the packed tensors: a padded layer's extra outputs are zeros, q | k | v of a head are one layer
    t = models["wide"][2].tensors
    assert t["pool1_b"].shape == (32,) and t["layer.0.qkv_b"].shape == (2, 96)
    small = gfm.pack_tensors(models["tiny"][0], models["tiny"][1])
    assert small["pool1_b"].shape == (16,) and not small["pool2_w"].reshape(-1)[16:].any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,text", [("input_dim", 65, "input_dim 65"), ("d_model", 144, "d_model 144"), ("d_model", 40, "d_model 40"),
                                               ("n_heads", 2, "n_heads 2"), ("n_layers", 9, "n_layers 9"), ("ff", 520, "ff 520"), ("ff", 24, "ff 24"),
                                               ("edge_dim", 4, "edge_dim 4"), ("max_degree", 256, "max_degree 256"), ("max_spd", 31, "max_spd 31")])
def test_configurations_outside_the_list_are_refused_by_field_name(models, field, value, text):
    import dataclasses

    with pytest.raises(K.LmxError, match=text):
        dataclasses.replace(gfm.GfmConfig(), **{field: value}).validate()
    # ... and by the library itself, handed a struct with that field
    host = models["shipped"][2]
    w = _lib.GfmWeights.from_buffer_copy(bytes(host.weights))
    setattr(w, field, value)
    b = host.batch(gfmref.make_graphs(host.cfg, 3, torch.Generator().manual_seed(1))[:1])
    g, out = b.struct(), torch.zeros((8,))
    lib = _lib.load()
    rc = lib.lmx_h_gfm_forward(C.byref(w), C.byref(g), None, 0, 0.1, out.data_ptr(), out.data_ptr(), None, None, None, None)
    assert rc != 0 and text.encode() in lib.lmx_last_error(), lib.lmx_last_error()


def test_calls_outside_the_list_are_refused(models):
    cfg, _, host, _ = models["tiny"]
    g = torch.Generator().manual_seed(2)
    graphs = gfmref.make_graphs(cfg, 7, g)
    with pytest.raises(K.LmxError, match="S 1 "):
        host.forward(graphs, [1, 2], 1)
    with pytest.raises(K.LmxError, match="eval mode only, S = 2"):
        host.forward(graphs, [1, 2], 2, node=True)
    with pytest.raises(K.LmxError, match="eval mode only, S = 2"):
        K.gfm_forward_host(host.weights, host.batch(graphs, [0, 0]), [1, 2], 2, cfg.dropout, attn=True)
    with pytest.raises(K.LmxError, match="one seed per graph"):
        host.forward(graphs, None, 2)
    # the library's own checks of the offsets and of N, behind Python's
    lib, out = _lib.load(), torch.zeros((64,))
    for node_off, text in (([1, 8], b"not at 0"), ([0, 0], b"N = 0 nodes"), ([0, gfm.MAX_NODES + 1], b"N = 96 nodes")):
        b = host.batch(graphs[:1])
        b.node_off = np.array(node_off, np.int32)
        st = b.struct()
        rc = lib.lmx_h_gfm_forward(C.byref(host.weights), C.byref(st), None, 0, 0.1, out.data_ptr(), out.data_ptr(), None, None, None, None)
        assert rc != 0 and text in lib.lmx_last_error(), lib.lmx_last_error()
    b = host.batch(graphs[:1])
    st = b.struct()
    rc = lib.lmx_h_gfm_forward(C.byref(host.weights), C.byref(st), None, 0, 0.1, out.data_ptr(), out.data_ptr(), None, out.data_ptr(), None, None)
    assert rc != 0 and b"attn_to_target without target" in lib.lmx_last_error()
    assert lib.lmx_gfm_workspace_bytes(0, 0, 8) == 0 and lib.lmx_gfm_workspace_bytes(3, 100, 8) == 64 + 3200
    # n = 0 graphs is no error and touches nothing
    empty = host.batch([])
    pred, stats = host.forward(empty, [], 2)[:2]
    assert pred.shape == (0, 2) and stats.shape == (0, 2)


def test_a_graph_does_not_depend_on_its_batch_position_on_the_host(models):
    cfg, _, host, _ = models["tiny"]
    g = torch.Generator().manual_seed(9)
    mine, other = gfmref.make_graphs(cfg, 17, g)[1], gfmref.make_graphs(cfg, 2, g)
    alone = host.forward([mine], [77], 4, trunk=True)
    among = host.forward([other[0], mine, other[1]], [5, 77, 6], 4, trunk=True)
    assert torch.equal(alone[0][0], among[0][1]) and torch.equal(alone[1][0], among[1][1]) and torch.equal(alone[4][0], among[4][1])
    again = host.forward([mine], [78], 4)
    assert not torch.equal(alone[0], again[0])  # another seed is another draw


# ---- the reference's own model, where it is at hand ------------------------------------------------------------------------------------
def _reference_modules():
    ref = gfmref.reference_modules()
    if ref is None:
        pytest.skip("no checkout of the reference beside the repository (or under LMX_REFERENCE), or no networkx")
    return ref


def test_the_references_own_model_agrees_with_the_restatement():
    ref = _reference_modules()
    torch.manual_seed(5)
    cfg = gfm.GfmConfig(input_dim=50, d_model=32, n_heads=2, n_layers=2, ff=64)
    net = ref.CowLamenessGraphormer(input_dim=50, hidden_dim=32, num_layers=2, num_heads=2, ffn_dim=64).eval()
    with torch.no_grad():  # the reference initialises biases, spd_bias and the virtual nodes to (nearly) nothing
        for name, p in net.named_parameters():
            if name.endswith("bias") or "spd_bias" in name or "virtual_node" in name:
                p.copy_(torch.rand_like(p) - 0.5)
    got, w = checkpoints.gfm_from_state_dict(net.state_dict(), num_heads=2)
    assert got == cfg
    g = torch.Generator().manual_seed(6)
    seen = {"pred": [], "node_pred": [], "attn": []}  # per output: (case, error against float64, the restatement's own float32 error)
    for N in (1, 2, 7, 17, gfm.MAX_NODES):
        for timed in (False, True):
            x, emb = torch.randn((N, 50), generator=g), torch.randn((N, 16), generator=g)
            ts = (1.7e9 + torch.randperm(N, generator=g).float() * 86400.0 * 0.7) if timed else None  # distinct: argsort has no ties
            data = ref.GraphormerGraphBuilder(5).build_graph(x, emb, ts)
            mine = gfmref.build_graph(cfg, x.numpy(), emb.numpy(), None if ts is None else ts.numpy())
            assert np.array_equal(mine["edges"].T, data.edge_index.numpy())
            assert np.abs(mine["edge_attr"] - data.edge_attr.numpy()).max(initial=0.0) <= 4e-7  # numpy's float32 similarity against our double one
            mine["edge_attr"] = data.edge_attr.numpy()
            with torch.no_grad():
                out = net(data, return_attention=True)
            target = N // 2
            r64 = gfmref.forward(cfg, w, mine, None, torch.float64, target)
            r32 = gfmref.forward(cfg, w, mine, None, torch.float32, target)
            for key, theirs in (("pred", out["graph_pred"].reshape(())), ("node_pred", out["node_pred"][:, 0]),
                                ("attn", out["attention_weights"][-1].mean(0)[:, target])):
                scale = float(r64[key].abs().max()) if key == "attn" else 1.0  # the attention column relative to its case's maximum
                seen[key].append(((N, timed), float((theirs.double() - r64[key]).abs().max()) / scale,
                                  float((r32[key].double() - r64[key]).abs().max()) / scale))
    # the rule of gfmref.tolerances: 4 x the restatement's own float32 error over ALL cases, and 4 f32 spacings more on a prediction
    for key, rows in seen.items():
        bound = 4 * max(e for _, _, e in rows) + (0.0 if key == "attn" else gfmref.PRED_FLOOR)
        print(f"the reference's {key} against float64: worst error / bound {max(d for _, d, _ in rows) / bound:.3f}")
        for case, d, _ in rows:
            assert d <= bound, (key, case, d, bound)


# ---- the golden file: the reference's recorded outputs, on every machine ---------------------------------------------------------------
def test_golden_outputs_of_the_reference_are_reproduced_on_the_host():
    cfg, w, cases = gfmref.load_golden()
    for c in cases:  # the builder: the reference's edges in its order; its float32 similarity against our double one
        mine = gfm.build_graph(cfg, c["graph"]["x"], c["emb"], c["graph"]["timestamps"], gfmref.K_NEIGHBOURS)
        assert np.array_equal(mine["edges"].T, c["edge_index"]) and np.array_equal(mine["edge_attr"], c["built_attr"])
        assert np.abs(mine["edge_attr"] - c["edge_attr"]).max() <= 4e-7
    ref32 = []
    for c in cases:
        r = gfmref.forward(cfg, w, c["graph"], None, torch.float32, c["target"])
        ref32.append((r["pred"], r["node_pred"], r["attn"]))
    gfmref.check_golden(cases, ref32, w, cfg, "gfmref in float32")
    host = gfm.GfmScorer(cfg, w, backend="host")
    pred, nodes, attn = host.node_scores([c["graph"] for c in cases], [c["target"] for c in cases])
    gfmref.check_golden(cases, list(zip(pred, nodes, attn)), w, cfg, "host")


def test_golden_file_is_what_the_reference_gives():
    ref = _reference_modules()
    z = np.load(gfmref.GOLDEN)
    cfg = gfmref.GOLDEN_CFG
    net = ref.CowLamenessGraphormer(input_dim=cfg.input_dim, hidden_dim=cfg.d_model, num_layers=cfg.n_layers, num_heads=cfg.n_heads, ffn_dim=cfg.ff).eval()
    net.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
    for i, (N, timed) in enumerate(gfmref.GOLDEN_SIZES):
        p = f"g{i}/"
        data = ref.GraphormerGraphBuilder(gfmref.K_NEIGHBOURS).build_graph(torch.from_numpy(z[p + "x"]), torch.from_numpy(z[p + "emb"]),
                                                                          torch.from_numpy(z[p + "ts"]) if timed else None)
        assert np.array_equal(data.edge_index.numpy(), z[p + "edge_index"]) and np.abs(data.edge_attr.numpy() - z[p + "edge_attr"]).max() <= 2e-7
        with torch.no_grad():
            out = net(data, return_attention=True)
        assert abs(float(out["graph_pred"]) - float(z[p + "graph_pred"])) <= 1e-6
        assert np.abs(out["node_pred"][:, 0].numpy() - z[p + "node_pred"]).max() <= 1e-6
        assert np.abs(out["attention_weights"][-1].mean(0)[:, int(z[p + "target"])].numpy() - z[p + "attn"]).max() <= 1e-6


def test_python_limits_are_the_headers():
    """The node limit and the accepted configurations are stated once more in lmx/kernels.py: held to include/lmx.h and csrc/gfm.h, and
    at every edge of the list Python and the library give the same answer."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lmx.h")).read()
    assert int(re.search(r"#define LMX_GFM_MAX_NODES (\d+)", hdr).group(1)) == K.GFM_MAX_NODES == gfm.MAX_NODES
    assert int(re.search(r"#define LMX_GFM_MAX_LAYERS (\d+)", hdr).group(1)) == _lib.GfmWeights.MAX_LAYERS == 8
    enum = dict(re.findall(r"(LMX_GFM_MAX_\w+) = (\d+)", open(os.path.join(root, "vision-sam3-yolo-lameless_amd", "csrc", "gfm.h")).read()))
    limits = {"input_dim": int(enum["LMX_GFM_MAX_IN"]), "d_model": int(enum["LMX_GFM_MAX_D"]), "ff": int(enum["LMX_GFM_MAX_FF"]),
              "max_degree": int(enum["LMX_GFM_MAX_DEGREE"]), "max_spd": int(enum["LMX_GFM_MAX_IDX"]) - 2, "n_layers": 8}
    lib, out = _lib.load(), torch.zeros((8,))
    host = gfm.GfmScorer(gfmref.TINY, checkpoints.gfm_from_state_dict(gfmref.state_dict(gfmref.TINY, 1), num_heads=2, dropout=0.3)[1], backend="host")
    b = host.batch(gfmref.make_graphs(host.cfg, 3, torch.Generator().manual_seed(1))[:1])
    for field, top in limits.items():
        step = 16 if field in ("d_model", "ff") else 1
        for value, ok in ((top, True), (top + step, False)):
            shape = dict(zip(("input_dim", "d_model", "n_heads", "n_layers", "ff", "edge_dim", "max_degree", "max_spd"), host.cfg.shape()))
            shape[field] = value
            if field == "d_model":
                shape["n_heads"] = value // 16
            try:
                K.gfm_check_config("t", *shape.values())
                python_ok = True
            except K.LmxError:
                python_ok = False
            w = _lib.GfmWeights.from_buffer_copy(bytes(host.weights))
            for k, v in shape.items():
                setattr(w, k, v)
            g = b.struct()
            # the library checks the configuration first and names the field; with the field inside the list it goes on to later checks,
            # which refuse S = 1 at the latest
            rc = lib.lmx_h_gfm_forward(C.byref(w), C.byref(g), None, 1, 0.1, out.data_ptr(), out.data_ptr(), None, None, None, None)
            library_ok = rc != 0 and f"{field} {value}".encode() not in lib.lmx_last_error()
            assert python_ok == library_ok == ok, (field, value, python_ok, library_ok, lib.lmx_last_error())


# ---- the weight image ------------------------------------------------------------------------------------------------------------------
def bad_images(raw):
    """{name: bytes} of truncated and corrupted copies of a kind-6 image, each refused by lmx_gfm_image_check_host"""
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    word = lambda i, v: raw[:48 + 4 * i] + struct.pack("<i", v) + raw[48 + 4 * i + 4:]  # noqa: E731
    return {"cut_header": raw[:40], "cut_config": raw[:70], "cut_directory": raw[:dir_off + 3 * native.ENTRY_BYTES + 17],
            "cut_data": raw[:data_off + (len(raw) - data_off) // 2], "cut_last_byte": raw[:-1],
            "kind": raw[:12] + struct.pack("<I", native.KIND_XFM) + raw[16:], "d_model_40": word(1, 40), "n_heads_0": word(2, 0),
            "n_layers_9": word(3, 9), "n_layers_negative": word(3, -3), "ff_520": word(4, 520), "edge_dim_4": word(5, 4),
            "max_degree_49": word(6, 49), "max_spd_31": word(7, 31), "n_tensors_huge": raw[:20] + struct.pack("<I", 2 ** 20) + raw[24:],
            "offset_wraps": raw[:dir_off + 72] + struct.pack("<Q", 2 ** 64 - 64) + raw[dir_off + 80:],
            "p_nan": raw[:48 + 32] + struct.pack("<d", float("nan")) + raw[48 + 40:]}


def test_weight_image_round_trip_and_refusals(models, tmp_path):
    for name, (cfg, w, host, _) in models.items():
        path = tmp_path / f"{name}.lmx"
        size = native.write_gfm_image(cfg, w, path)
        assert size == path.stat().st_size
        i = native.check_gfm_image(path)
        assert (i.input_dim, i.d_model, i.n_heads, i.n_layers, i.ff, i.edge_dim, i.max_degree, i.max_spd) == cfg.shape()
        assert i.max_nodes == gfm.MAX_NODES and i.p == cfg.dropout
    raw = (tmp_path / "shipped.lmx").read_bytes()
    assert struct.unpack_from("<I", raw, 12)[0] == native.KIND_GFM == 6
    # every tensor of the packed network is in the file, bit for bit, where its directory entry says
    dir_off, _ = struct.unpack_from("<QQ", raw, 24)
    packed = gfm.pack_tensors(*models["shipped"][:2])
    n_tensors = struct.unpack_from("<I", raw, 20)[0]
    assert n_tensors == len(packed) == 14 + 17 * 6 + 26
    for k in range(n_tensors):
        entry = raw[dir_off + k * native.ENTRY_BYTES:dir_off + (k + 1) * native.ENTRY_BYTES]
        tname = entry[:native.NAME_BYTES].rstrip(b"\0").decode()
        offset, nbytes = struct.unpack_from("<QQ", entry, 72)
        assert raw[offset:offset + nbytes] == packed[tname].tobytes(), tname
    texts = {"kind": "kind 5 is not GFM", "d_model_40": "d_model 40", "n_heads_0": "n_heads 0", "n_layers_9": "n_layers 9",
             "n_layers_negative": "n_layers -3", "ff_520": "ff 520", "edge_dim_4": "edge_dim 4", "max_degree_49": "deg_in", "max_spd_31": "max_spd 31",
             "p_nan": "p nan"}
    for name, data in bad_images(raw).items():
        bad = tmp_path / f"bad_{name}.lmx"
        bad.write_bytes(data)
        with pytest.raises(K.LmxError, match=texts.get(name, "gfm image")):
            native.check_gfm_image(bad)
    with pytest.raises(K.LmxError):
        native.check_gfm_image(tmp_path / "absent.lmx")


# ---- the service mirror ----------------------------------------------------------------------------------------------------------------
def _results_tree(root, videos, rng):
    """videos: (video_id, cow_id or None, timestamp or None); every video gets the four result files, some with fields missing"""
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


def test_service_mirror_on_a_results_tree(models, tmp_path):
    from lmx.services import GraphTransformerPipeline
    from lmx.services.runtime import InProcessBus

    cfg, w, host, _ = models["shipped"]
    rng = np.random.default_rng(3)
    videos = [(f"a{i}", "cow_A", "2024-05-%02dT10:00:00Z" % (i + 1)) for i in range(6)] + [(f"b{i}", "cow_B", 1.7e9 + 3600.0 * i) for i in range(3)]
    videos += [("loose", None, None), ("a_bad_time", "cow_A", "yesterday")]
    _results_tree(tmp_path, videos, rng)
    bus = InProcessBus()
    got = []

    async def run():
        await bus.subscribe("pipeline.graph_transformer", lambda m: got.append(m))
        svc = GraphTransformerPipeline(host, bus, config={}, data_dir=tmp_path)
        await svc.process_video({"video_id": "a3"})
        await svc.process_video({})
        await svc.process_videos([{"video_id": "b1"}, {"video_id": "loose"}, {"video_id": "a3"}, {"video_id": "new_video"}])
        return svc

    svc = asyncio.run(run())
    assert [m["video_id"] for m in got] == ["a3", "b1", "loose", "a3", "new_video"]
    res = json.loads((tmp_path / "graph_transformer" / "a3_graph_transformer.json").read_text())
    assert list(res) == ["video_id", "cow_id", "pipeline", "model", "graph_prediction", "node_prediction", "cow_severity_score", "uncertainty",
                         "prediction", "cow_prediction", "confidence", "graph_info", "attention_info", "videos_in_graph"]
    assert list(res["graph_info"]) == ["num_nodes", "num_edges", "num_layers", "num_heads", "hidden_dim", "has_temporal_edges", "per_cow_graph"]
    assert res["cow_id"] == "cow_A" and res["model"] == "CowLamenessGraphormer" and sorted(res["videos_in_graph"]) == sorted(
        [f"a{i}" for i in range(6)] + ["a_bad_time"])
    info = res["graph_info"]
    assert (info["num_nodes"], info["num_layers"], info["num_heads"], info["hidden_dim"], info["has_temporal_edges"], info["per_cow_graph"]) == (
        7, 6, 8, 128, True, True) and info["num_edges"] == 7 * 5 + 2 * 6
    top = res["attention_info"]["top_attending_nodes"]
    assert 4 <= len(top) <= 5 and all(t["video_id"] != "a3" for t in top) and [t["attention"] for t in top] == sorted((t["attention"] for t in top), reverse=True)
    assert res["confidence"] == 1.0 - res["uncertainty"] and res["prediction"] == int(res["node_prediction"] > 0.5)
    assert got[0] == {"video_id": "a3", "cow_id": "cow_A", "pipeline": "graph_transformer", "results_path": str(tmp_path / "graph_transformer" / "a3_graph_transformer.json"),
                      "severity_score": res["node_prediction"], "cow_severity_score": res["cow_severity_score"], "uncertainty": res["uncertainty"]}
    assert got[3] == got[0]  # in a backlog a graph scores to the same bytes
    # the target index, the features and the scores are those of the scorer on the mirror's own graph
    item = svc._graph("a3")
    assert item["video_ids"][item["target"]] == "a3" and item["graph"]["timestamps"] is not None
    x = item["graph"]["x"]
    assert x.shape == (7, 50) and (x[:, 47:] == np.array([0.5, 1.0, 0.5], np.float32)).all() and (x[:, 12] == 1.0).all()  # meta; aspect ratio's default
    assert svc.video_timestamps["a_bad_time"] == 0.0 and svc.video_timestamps["b2"] == 1.7e9 + 7200.0
    mean, std, _ = host.score([item["graph"]], [gfm.graph_seed("a3")], 10)
    _, nodes, attn = host.node_scores([item["graph"]], [item["target"]])
    assert res["graph_prediction"] == float(mean[0]) and res["uncertainty"] == float(std[0]) and res["node_prediction"] == float(nodes[0][item["target"]])
    assert {t["video_id"]: t["attention"] for t in top} == {item["video_ids"][i]: float(attn[0][i]) for i in np.argsort(attn[0].numpy())[-5:] if i != item["target"]}
    # a video without a cow: the global graph over every analysed video, no temporal edges; an unknown video joins with the defaults
    loose = json.loads((tmp_path / "graph_transformer" / "loose_graph_transformer.json").read_text())
    assert loose["cow_id"] is None and loose["graph_info"]["num_nodes"] == 11 and not loose["graph_info"]["has_temporal_edges"]
    assert loose["graph_info"]["num_edges"] == 11 * 5
    new = json.loads((tmp_path / "graph_transformer" / "new_video_graph_transformer.json").read_text())
    assert new["graph_info"]["num_nodes"] == 12 and new["videos_in_graph"][-1] == "new_video"


def test_service_mirror_refuses_a_graph_above_the_limit(models, tmp_path, capsys):
    from lmx.services import GraphTransformerPipeline
    from lmx.services.runtime import InProcessBus

    host = models["shipped"][2]
    n = gfm.MAX_NODES + 1
    _results_tree(tmp_path, [(f"v{i}", "cow_A", 1.7e9 + i) for i in range(n)], np.random.default_rng(1))
    svc = GraphTransformerPipeline(host, InProcessBus(), config={}, data_dir=tmp_path)
    with pytest.raises(K.LmxError, match=f"{n} nodes.*{gfm.MAX_NODES}"):
        svc._graph("v0")
    asyncio.run(svc.process_video({"video_id": "v0"}))
    asyncio.run(svc.process_videos([{"video_id": "v1"}]))
    assert f"{n} nodes" in capsys.readouterr().out and not list((tmp_path / "graph_transformer").iterdir())
