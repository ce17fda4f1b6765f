"""The graph transformer of services/graph-transformer-pipeline (app/model/*.py: CowLamenessGraphormer) on liblmx: a cow's lameness
score and its MC-dropout spread, node scores and the attention towards a target video from one graph per cow, for a batch of graphs
of differing size in ONE launch behind a small bias kernel (csrc/gfm.hip; include/lmx.h "The graph transformer" has the network, the
graph rules and the keep bits).

``GfmConfig`` is the network's shape, ``pack_tensors`` turns the weights (``lmx.checkpoints.gfm_from_state_dict``) into the tensors the
kernel reads, ``build_graph`` prepares a graph on the host (``lmx_h_gfm_graph``), ``GfmScorer`` scores graphs on the device or, with
``backend="host"``, through the plain C++ forward ``lmx_h_gfm_forward`` without a GPU.  There is no torch arithmetic here."""
import dataclasses

import numpy as np

from . import kernels as K
from ._lib import LmxError
from .gait import GaitScorer, checked_arrays, graph_features, graph_seed  # noqa: F401 (graph_seed: the seed of a graph)
from .xfm import pack_linear

MAX_NODES = K.GFM_MAX_NODES


@dataclasses.dataclass(frozen=True)
class GfmConfig:
    """services/graph-transformer-pipeline/app/model/graphormer.py:41-54 by default."""
    input_dim: int = 50
    d_model: int = 128
    n_heads: int = 8
    n_layers: int = 6
    ff: int = 512
    edge_dim: int = 3
    max_degree: int = 50
    max_spd: int = 10
    dropout: float = 0.1

    @property
    def n_sites(self):
        return 6 * self.n_layers + 4

    @property
    def head_dim(self):
        return self.d_model // self.n_heads

    @property
    def pool_dim(self):
        """D / 2 rounded up to a column tile: the attention pool and the node head run on the MFMA"""
        return (self.d_model // 2 + 15) // 16 * 16

    def shape(self):
        return (self.input_dim, self.d_model, self.n_heads, self.n_layers, self.ff, self.edge_dim, self.max_degree, self.max_spd)

    def validate(self, who="GfmConfig"):
        """The list of include/lmx.h; LmxError names the field."""
        K.gfm_check_config(who, *self.shape())
        if not 0.0 <= self.dropout < 1.0:
            raise LmxError(f"{who}: p {self.dropout} outside [0, 1)")
        return self


def pack_tensors(cfg, weights):
    """Ordered {field of lmx_gfm_weights_t: f32 numpy array} from the weights under gfm_from_state_dict's names (torch's layouts)."""
    cfg.validate("pack_tensors")
    take = checked_arrays(weights)
    D, H, dh, L, pd = cfg.d_model, cfg.n_heads, cfg.head_dim, cfg.n_layers, cfg.pool_dim

    def padded(w, b, w2):
        """a D -> D / 2 layer and the D / 2 -> 1 layer behind it, widened to pool_dim outputs with zeros"""
        wp, bp, w2p = np.zeros((pd, D), np.float32), np.zeros((pd,), np.float32), np.zeros((pd,), np.float32)
        wp[:D // 2], bp[:D // 2], w2p[:D // 2] = w, b, w2.reshape(-1)
        return pack_linear(wp), bp, w2p

    def qkv(p, names):
        ws, bs = [take(p + n + ".weight", (D, D)) for n in names], [take(p + n + ".bias", (D,)) for n in names]
        # head i: the rows q_i | k_i | v_i as ONE linear layer of 3 dh outputs
        w = np.concatenate([pack_linear(np.concatenate([m[i * dh:(i + 1) * dh] for m in ws], 0)) for i in range(H)], 0)
        return w, np.stack([np.concatenate([b[i * dh:(i + 1) * dh] for b in bs]) for i in range(H)], 0)

    out = {"in_w": pack_linear(take("in.weight", (D, cfg.input_dim))), "in_b": take("in.bias", (D,)), "in_g": take("in_norm.weight", (D,)),
           "in_beta": take("in_norm.bias", (D,)), "deg_in": take("deg_in", (cfg.max_degree + 1, D)), "deg_out": take("deg_out", (cfg.max_degree + 1, D)),
           "time_w": pack_linear(take("time.weight", (D, D))), "time_b": take("time.bias", (D,)), "div_term": take("div_term", (D // 2,)),
           "spd": take("spd", (cfg.max_spd + 2, H)), "e1_w": take("edge1.weight", (2 * H, 3)), "e1_b": take("edge1.bias", (2 * H,)),
           "e2_w": take("edge2.weight", (H, 2 * H)), "e2_b": take("edge2.bias", (H,))}
    for l in range(L):
        p = f"layer.{l}."
        out[p + "ln1_g"], out[p + "ln1_b"] = take(p + "ln1.weight", (D,)), take(p + "ln1.bias", (D,))
        out[p + "qkv_w"], out[p + "qkv_b"] = qkv(p, ("q", "k", "v"))
        out[p + "out_w"], out[p + "out_b"] = pack_linear(take(p + "out.weight", (D, D))), take(p + "out.bias", (D,))
        out[p + "ln2_g"], out[p + "ln2_b"] = take(p + "ln2.weight", (D,)), take(p + "ln2.bias", (D,))
        out[p + "ff1_w"], out[p + "ff1_b"] = pack_linear(take(p + "ff1.weight", (cfg.ff, D))), take(p + "ff1.bias", (cfg.ff,))
        out[p + "ff2_w"], out[p + "ff2_b"] = pack_linear(take(p + "ff2.weight", (D, cfg.ff))), take(p + "ff2.bias", (D,))
        out[p + "vn"] = take(p + "vn", (D,))
        out[p + "vqkv_w"], out[p + "vqkv_b"] = qkv(p, ("vq", "vk", "vv"))
        out[p + "vout_w"], out[p + "vout_b"] = pack_linear(take(p + "vout.weight", (D, D))), take(p + "vout.bias", (D,))
        # vn_update of every layer is checked, the last one's is kept: the earlier virtual nodes are dead
        vu = (take(p + "vu1.weight", (2 * D, D)), take(p + "vu1.bias", (2 * D,)), take(p + "vu2.weight", (D, 2 * D)), take(p + "vu2.bias", (D,)),
              take(p + "vu_norm.weight", (D,)), take(p + "vu_norm.bias", (D,)))
    out["vu1_w"], out["vu1_b"], out["vu2_w"], out["vu2_b"], out["vu_g"], out["vu_beta"] = vu[0].T, vu[1], vu[2].T, vu[3], vu[4], vu[5]
    out["lnf_g"], out["lnf_b"] = take("lnf.weight", (D,)), take("lnf.bias", (D,))
    out["pool1_w"], out["pool1_b"], out["pool2_w"] = padded(take("pool1.weight", (D // 2, D)), take("pool1.bias", (D // 2,)),
                                                            take("pool2.weight", (1, D // 2)))
    out["pool2_b"] = take("pool2.bias", (1,))
    out["comb_w"], out["comb_b"] = take("comb.weight", (D, 3 * D)).T, take("comb.bias", (D,))
    out["comb_g"], out["comb_beta"] = take("comb_norm.weight", (D,)), take("comb_norm.bias", (D,))
    out["ph1_w"], out["ph1_b"] = take("ph1.weight", (D // 2, D)).T, take("ph1.bias", (D // 2,))
    out["ph2_w"], out["ph2_b"] = take("ph2.weight", (D // 4, D // 2)).T, take("ph2.bias", (D // 4,))
    out["ph3_w"], out["ph3_b"] = take("ph3.weight", (1, D // 4)).reshape(-1), take("ph3.bias", (1,))
    out["nh1_w"], out["nh1_b"], out["nh2_w"] = padded(take("nh1.weight", (D // 2, D)), take("nh1.bias", (D // 2,)), take("nh2.weight", (1, D // 2)))
    out["nh2_b"] = take("nh2.bias", (1,))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


def build_graph(cfg, x, embeddings, timestamps=None, k=5):
    """A graph as GraphormerGraphBuilder(k).build_graph makes it, by lmx_h_gfm_graph's pinned rules (include/lmx.h): a dict with x f32
    [N, input_dim], timestamps (None or f32 [N]), edges int32 [E, 2], edge_attr f32 [E, 3], deg_in / deg_out uint8 [N] clamped to
    cfg.max_degree, idx uint8 [N, N] and win int32 [N, N].  More than MAX_NODES nodes are refused."""
    x = graph_features(cfg, x, embeddings, MAX_NODES)
    g = K.gfm_graph(embeddings, timestamps, k, cfg.max_degree, cfg.max_spd)
    g["x"] = x
    g["timestamps"] = None if timestamps is None else np.ascontiguousarray(timestamps, np.float32)
    return g


class GfmScorer(GaitScorer):
    """The network on `device` (backend "device", default) or on the host (backend "host": lmx_h_gfm_forward, no GPU)."""
    _pack = staticmethod(pack_tensors)

    _weights = staticmethod(lambda cfg, tensors: K.gfm_weights(*cfg.shape(), tensors))

    def batch(self, graphs, targets=None):
        """The graphs (build_graph's dicts) concatenated where the network lives."""
        return K.GfmBatch(graphs, self.device, targets)

    def forward(self, graphs, seeds=None, n_samples=10, targets=None, node=False, trunk=False, vn=False):
        """graphs: build_graph's dicts or a GfmBatch -> (pred [n, max(S, 1)], stats [n, 2], node_pred [sum N] or None, attn_to_target
        [sum N] or None (with targets, S = 0), trunk: a list of [max(S, 1), N_g, D] or None, vn [n, max(S, 1), D] or None)."""
        b = graphs if isinstance(graphs, K.GfmBatch) else self.batch(graphs, targets)
        fn = K.gfm_forward_host if self.backend == "host" else K.gfm_forward
        return fn(self.weights, b, seeds, n_samples, self.cfg.dropout, node=node, attn=b.target is not None and n_samples == 0, trunk=trunk, vn=vn)

    def score(self, graphs, seeds=None, n_samples=10):
        """(mean [n], unbiased std [n], pred [n, max(S, 1)]); n_samples = 0: eval mode, std = 0."""
        pred, stats = self.forward(graphs, seeds, n_samples)[:2]
        return stats[:, 0], stats[:, 1], pred

    def node_scores(self, graphs, targets=None):
        """Eval mode: (pred [n], a list of node_pred [N_g], a list of attn_to_target [N_g] or None without targets)."""
        b = graphs if isinstance(graphs, K.GfmBatch) else self.batch(graphs, targets)
        pred, _, npred, at, _, _ = self.forward(b, None, 0, node=True)
        cut = [int(v) for v in b.node_off]
        split = lambda t: [t[cut[i]:cut[i + 1]] for i in range(b.n)]  # noqa: E731
        return pred[:, 0], split(npred), None if at is None else split(at)
