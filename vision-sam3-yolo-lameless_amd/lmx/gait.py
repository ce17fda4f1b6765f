"""What the gait sequence models (``lmx.tcn``, ``lmx.xfm``) have in common on the Python side: the operand order of a packed
convolution (csrc/gait.h), the seed of a clip, and the scorer that holds a network's packed tensors on the device or on the host; and
what the two graph models (``lmx.gfm``, ``lmx.gnn``) share on top: the seed of a graph, the weights as checked f32 arrays and the node
features of a graph."""
import hashlib

import numpy as np
import torch

from ._lib import LmxError


def pack_conv(w):
    """f32 [N, Cin, k] -> f32 [k * Q, N / 16, 64, 4], the MFMA B-operand order of csrc/gait.h:
    entry [j * Q + q][nt][l][e] = W[16 nt + (l & 15)][16 q + 4 (l >> 4) + e][j], zeros where the input channel is >= Cin."""
    w = np.asarray(w, np.float32)
    n, cin, k = w.shape
    q = (cin + 15) // 16
    wp = np.zeros((n, 16 * q, k), np.float32)
    wp[:, :cin] = w
    # (nt, r, q, g, e, j) -> (j, q, nt, g, r, e); the lane is l = 16 g + r
    return np.ascontiguousarray(wp.reshape(n // 16, 16, q, 4, 4, k).transpose(5, 2, 0, 3, 1, 4)).reshape(k * q, n // 16, 64, 4)


def clip_seed(video_id):
    """The seed of a clip: the first 8 bytes of the SHA-256 of its video_id, little-endian."""
    return int.from_bytes(hashlib.sha256(str(video_id).encode()).digest()[:8], "little")


def graph_seed(video_id):
    """The seed of a graph: that of a clip, from the video the graph is scored for."""
    return clip_seed(video_id)


def checked_arrays(weights):
    """take(name, shape) over the weights (torch tensors or arrays): the f32 numpy array of that name, which must have that shape."""
    f = {k: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32) for k, v in weights.items()}

    def take(name, shape):
        a = f.get(name)
        if a is None or a.shape != shape:
            raise LmxError(f"pack_tensors: {name} has shape {None if a is None else a.shape}, the configuration calls for {shape}")
        return a

    return take


def graph_features(cfg, x, embeddings, max_nodes):
    """The node features of a graph as f32 [N, cfg.input_dim], one embedding per node; more than max_nodes nodes are refused."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2 or x.shape[1] != cfg.input_dim:
        raise LmxError(f"build_graph: x must be [N, {cfg.input_dim}], got {x.shape}")
    if x.shape[0] > max_nodes:
        raise LmxError(f"build_graph: a graph of {x.shape[0]} nodes; one workgroup holds at most {max_nodes}")
    if len(embeddings) != x.shape[0]:
        raise LmxError(f"build_graph: {len(embeddings)} embeddings for {x.shape[0]} nodes")
    return x


class GaitScorer:
    """A network on `device` (backend "device", default) or on the host (backend "host": the plain C++ forward, no GPU): its
    configuration, its packed tensors and the weights struct over them.  A subclass says how to pack (`_pack(cfg, weights)`) and how
    to build the struct (`_weights(cfg, tensors)`)."""

    def __init__(self, cfg, weights, device=None, backend="device"):
        name = type(self).__name__
        if backend not in ("device", "host"):
            raise LmxError(f"{name}: backend {backend!r} is neither 'device' nor 'host'")
        self.cfg, self.backend = cfg.validate(name), backend
        self.device = torch.device("cpu") if backend == "host" else torch.device("cuda" if device is None else device)
        self.tensors = {k: torch.from_numpy(v).to(self.device) for k, v in self._pack(cfg, weights).items()}
        self.weights = self._weights(cfg, self.tensors)
