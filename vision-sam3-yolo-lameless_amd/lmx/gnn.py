"""GraphGPS of services/gnn-pipeline (app/main.py: EnhancedGraphGPS, the default of GNNPipeline) on liblmx: node scores and their
MC-dropout spread, the cow score and the head's attention weights from one graph per cow, for a batch of graphs of differing size in
ONE launch (csrc/gnn.hip; include/lmx.h "GraphGPS" has the live network, the graph rules, both encodings and the keep bits).

``GnnConfig`` is the live network's shape, ``pack_tensors`` turns the weights (``lmx.checkpoints.gnn_from_state_dict``) into the
tensors the kernel reads, ``build_graph`` prepares a graph and its two raw encodings on the host (``lmx_h_gnn_graph``), ``GnnScorer``
scores graphs on the device or, with ``backend="host"``, through the plain C++ forward ``lmx_h_gnn_forward`` without a GPU.  There is
no torch arithmetic here."""
import dataclasses

import numpy as np

from . import kernels as K
from ._lib import LmxError
from .gait import GaitScorer, checked_arrays, graph_features, graph_seed  # noqa: F401 (graph_seed: the seed of a graph)
from .xfm import pack_linear

MAX_NODES = K.GNN_MAX_NODES
MAX_EDGES = K.GNN_MAX_EDGES
MAX_LAYERS = K.GNN_MAX_LAYERS
LAP_K = K.GNN_LAP_K
RW_K = K.GNN_RW_K


@dataclasses.dataclass(frozen=True)
class GnnConfig:
    """services/gnn-pipeline/app/main.py:1148-1158 by default.  n_layers counts the LIVE layers: num_layers // 2 of the reference, whose
    post-pool half never reaches an output."""
    input_dim: int = 50
    d_model: int = 128
    n_heads: int = 8
    n_layers: int = 2
    pe_dim: int = 16
    ff: int = 512
    edge_dim: int = 3
    dropout: float = 0.1

    @property
    def n_sites(self):
        return 5 * self.n_layers + 1

    @property
    def head_dim(self):
        return self.d_model // self.n_heads

    def shape(self):
        return (self.input_dim, self.d_model, self.n_heads, self.n_layers, self.pe_dim, self.ff, self.edge_dim)

    def validate(self, who="GnnConfig"):
        """The list of include/lmx.h; LmxError names the field."""
        K.gnn_check_config(who, *self.shape())
        if not 0.0 <= self.dropout < 1.0:
            raise LmxError(f"{who}: p {self.dropout} outside [0, 1)")
        return self


def pack_tensors(cfg, weights):
    """Ordered {field of lmx_gnn_weights_t: f32 numpy array} from the weights under gnn_from_state_dict's names (torch's layouts)."""
    cfg.validate("pack_tensors")
    take = checked_arrays(weights)
    D, H, dh, L, P = cfg.d_model, cfg.n_heads, cfg.head_dim, cfg.n_layers, cfg.pe_dim

    out = {"in_w": pack_linear(take("in.weight", (D - 2 * P, cfg.input_dim))), "in_b": take("in.bias", (D - 2 * P,))}
    for enc, k in (("lap", LAP_K), ("rw", RW_K)):
        out[f"{enc}1_w"], out[f"{enc}1_b"] = take(f"{enc}1.weight", (2 * P, k)), take(f"{enc}1.bias", (2 * P,))
        out[f"{enc}2_w"], out[f"{enc}2_b"] = take(f"{enc}2.weight", (P, 2 * P)), take(f"{enc}2.bias", (P,))
        out[f"{enc}_g"], out[f"{enc}_beta"] = take(f"{enc}_norm.weight", (P,)), take(f"{enc}_norm.bias", (P,))
    out["ee1_w"], out["ee1_b"] = take("ee1.weight", (D // 2, 3)), take("ee1.bias", (D // 2,))
    out["ee2_w"], out["ee2_b"] = pack_linear(take("ee2.weight", (D, D // 2))), take("ee2.bias", (D,))
    out["ee_g"], out["ee_beta"] = take("ee_norm.weight", (D,)), take("ee_norm.bias", (D,))
    for l in range(L):
        p = f"layer.{l}."

        def norm(ours, theirs):
            out[p + ours + "_g"], out[p + ours + "_b"] = take(p + theirs + ".weight", (D,)), take(p + theirs + ".bias", (D,))

        def bn(ours, theirs):
            norm(ours, theirs)
            out[p + ours + "_mean"], out[p + ours + "_var"] = take(p + theirs + ".running_mean", (D,)), take(p + theirs + ".running_var", (D,))

        norm("ln1", "ln1")
        out[p + "abde_w"] = pack_linear(np.concatenate([take(p + n + ".weight", (D, D)) for n in "ABDE"], 0))
        out[p + "abde_b"] = np.concatenate([take(p + n + ".bias", (D,)) for n in "ABDE"])
        out[p + "c_w"], out[p + "c_b"] = pack_linear(take(p + "C.weight", (D, D))), take(p + "C.bias", (D,))
        if l < L - 1:  # the last live layer's edge update feeds nothing
            out[p + "eu1_w"], out[p + "eu1_b"] = pack_linear(take(p + "eu1.weight", (D, 3 * D))), take(p + "eu1.bias", (D,))
            out[p + "eu2_w"], out[p + "eu2_b"] = pack_linear(take(p + "eu2.weight", (D, D))), take(p + "eu2.bias", (D,))
            bn("bne", "bne")
        bn("bnn", "bnn")
        norm("ln2", "ln2")
        wq, bq = take(p + "in_proj.weight", (3 * D, D)), take(p + "in_proj.bias", (3 * D,))
        # head i: the rows q_i | k_i | v_i of in_proj as ONE linear layer of 3 dh outputs
        rows = [np.concatenate([np.arange(j * D + i * dh, j * D + (i + 1) * dh) for j in range(3)]) for i in range(H)]
        out[p + "qkv_w"] = np.concatenate([pack_linear(wq[r]) for r in rows], 0)
        out[p + "qkv_b"] = np.stack([bq[r] for r in rows], 0)
        out[p + "out_w"], out[p + "out_b"] = pack_linear(take(p + "out.weight", (D, D))), take(p + "out.bias", (D,))
        norm("lna", "lna"), norm("ln3", "ln3")
        out[p + "ff1_w"], out[p + "ff1_b"] = pack_linear(take(p + "ff1.weight", (cfg.ff, D))), take(p + "ff1.bias", (cfg.ff,))
        out[p + "ff2_w"], out[p + "ff2_b"] = pack_linear(take(p + "ff2.weight", (D, cfg.ff))), take(p + "ff2.bias", (D,))
    out["lnf_g"], out["lnf_b"] = take("lnf.weight", (D,)), take("lnf.bias", (D,))
    for ours in ("nh", "na"):
        out[ours + "1_w"], out[ours + "1_b"] = pack_linear(take(ours + "1.weight", (D // 2, D))), take(ours + "1.bias", (D // 2,))
        out[ours + "2_w"], out[ours + "2_b"] = take(ours + "2.weight", (1, D // 2)).reshape(-1), take(ours + "2.bias", (1,))
    out["cl1_w"], out["cl1_b"] = take("cl1.weight", (D, 2 * D)).T, take("cl1.bias", (D,))
    out["cl2_w"], out["cl2_b"] = take("cl2.weight", (D // 2, D)).T, take("cl2.bias", (D // 2,))
    out["cl3_w"], out["cl3_b"] = take("cl3.weight", (1, D // 2)).reshape(-1), take("cl3.bias", (1,))
    shapes = K.gnn_tensor_shapes(*cfg.shape())
    return {k: np.ascontiguousarray(out[k], np.float32) for k in shapes}


def build_graph(cfg, x, embeddings, timestamps=None, k=5):
    """A graph as GraphBuilder(k).build_graph makes it, with the two raw encodings, by lmx_h_gnn_graph's pinned rules (include/lmx.h): a
    dict with x f32 [N, input_dim], edges int32 [E, 2], edge_attr f32 [E, 3], csr_ptr, csr_edge, deg, lap f32 [N, 8], rw f32 [N, 16].
    timestamps: those of a known cow in seconds, float64 as the reference keeps them (temporal edges), or None.  More than MAX_NODES nodes are refused."""
    x = graph_features(cfg, x, embeddings, MAX_NODES)
    g = K.gnn_graph(embeddings, timestamps, k)
    g["x"] = x
    return g


class GnnScorer(GaitScorer):
    """The network on `device` (backend "device", default) or on the host (backend "host": lmx_h_gnn_forward, no GPU)."""
    _pack = staticmethod(pack_tensors)

    _weights = staticmethod(lambda cfg, tensors: K.gnn_weights(*cfg.shape(), tensors))

    def batch(self, graphs):
        """The graphs (build_graph's dicts) concatenated where the network lives."""
        return K.GnnBatch(graphs, self.device)

    def forward(self, graphs, seeds=None, n_samples=10, trunk=False):
        """graphs: build_graph's dicts or a GnnBatch -> (node_mc [sum N, S], stats [sum N, 2], graph_pred [n], node_pred [sum N],
        attn_weights [sum N], trunk); the first two are None in eval mode (n_samples = 0), the next three with n_samples > 0."""
        b = graphs if isinstance(graphs, K.GnnBatch) else self.batch(graphs)
        fn = K.gnn_forward_host if self.backend == "host" else K.gnn_forward
        return fn(self.weights, b, seeds, n_samples, self.cfg.dropout, trunk=trunk)

    def score(self, graphs, seeds, n_samples=10):
        """predict_with_uncertainty: per graph (mean [N_g], unbiased std [N_g]) of the node scores over n_samples train-mode samples."""
        b = graphs if isinstance(graphs, K.GnnBatch) else self.batch(graphs)
        stats = self.forward(b, seeds, n_samples)[1]
        cut = [int(v) for v in b.node_off]
        return [(stats[cut[i]:cut[i + 1], 0], stats[cut[i]:cut[i + 1], 1]) for i in range(b.n)]

    def evaluate(self, graphs):
        """The eval-mode forward: (graph_pred [n], a list of node_pred [N_g], a list of attention_weights [N_g])."""
        b = graphs if isinstance(graphs, K.GnnBatch) else self.batch(graphs)
        _, _, gp, npred, attw, _ = self.forward(b, None, 0)
        cut = [int(v) for v in b.node_off]
        split = lambda t: [t[cut[i]:cut[i + 1]] for i in range(b.n)]  # noqa: E731
        return gp, split(npred), split(attw)
