"""The gait transformer of services/transformer-pipeline (main.py:24-237) on liblmx: a lameness severity score, its MC-dropout spread
and a temporal saliency from a pose series, in ONE launch for a batch of clips (csrc/xfm.hip; include/lmx.h "The gait transformer" has
the network, the masking rules and the keep bits).

``XfmConfig`` is the network's shape, ``pack_tensors`` turns the weights (``lmx.checkpoints.xfm_from_state_dict``) into the tensors the
kernel and the weight image hold, ``XfmScorer`` scores clips on the device or, with ``backend="host"``, through the plain C++ forward
``lmx_h_xfm_forward`` without a GPU.  There is no torch arithmetic here."""
import dataclasses

import numpy as np
import torch

from . import kernels as K
from ._lib import LmxError
from .gait import GaitScorer, clip_seed, pack_conv  # noqa: F401 — the seeds and the operand order are every gait model's


@dataclasses.dataclass(frozen=True)
class XfmConfig:
    """services/transformer-pipeline/app/main.py:276-284 by default."""
    input_dim: int = 44
    d_model: int = 64
    n_heads: int = 4
    n_layers: int = 4
    ff: int = 256
    head: int = 32
    dropout: float = 0.1
    max_len: int = 150

    @property
    def n_sites(self):
        return 4 * self.n_layers + 2

    @property
    def head_dim(self):
        return self.d_model // self.n_heads

    def shape(self):
        return (self.input_dim, self.d_model, self.n_heads, self.n_layers, self.ff, self.head, self.max_len)

    def validate(self, who="XfmConfig"):
        """The list of include/lmx.h; LmxError names the field."""
        K.xfm_check_config(who, *self.shape())
        if not 0.0 <= self.dropout < 1.0:
            raise LmxError(f"{who}: p {self.dropout} outside [0, 1)")
        return self


def pack_linear(w):
    """f32 [N, K] -> f32 [Q, N / 16, 64, 4]: a convolution with one tap in the shared operand order (lmx.gait.pack_conv)."""
    w = np.asarray(w, np.float32)
    return pack_conv(w.reshape(w.shape[0], w.shape[1], 1))


def pack_tensors(cfg, weights):
    """Ordered {image tensor name: f32 numpy array} from the weights under xfm_from_state_dict's names (torch's layouts)."""
    cfg.validate("pack_tensors")
    f = {k: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32) for k, v in weights.items()}
    D, H, dh = cfg.d_model, cfg.n_heads, cfg.head_dim

    def take(name, shape):
        a = f.get(name)
        if a is None or a.shape != shape:
            raise LmxError(f"pack_tensors: {name} has shape {None if a is None else a.shape}, the configuration calls for {shape}")
        return a

    out = {"in.w": pack_linear(take("in.weight", (D, cfg.input_dim))), "in.b": take("in.bias", (D,)), "pe": take("pe", (cfg.max_len, D))}
    for l in range(cfg.n_layers):
        p = f"layer.{l}."
        wqkv, bqkv = take(p + "qkv.weight", (3 * D, D)), take(p + "qkv.bias", (3 * D,))
        # head i: the rows q_i | k_i | v_i as ONE linear layer of 3 dh outputs
        rows = [np.concatenate([np.arange(s * D + i * dh, s * D + (i + 1) * dh) for s in range(3)]) for i in range(H)]
        out[p + "ln1.g"], out[p + "ln1.b"] = take(p + "ln1.weight", (D,)), take(p + "ln1.bias", (D,))
        out[p + "qkv.w"] = np.concatenate([pack_linear(wqkv[r]) for r in rows], 0)
        out[p + "qkv.b"] = np.stack([bqkv[r] for r in rows], 0)
        out[p + "out.w"], out[p + "out.b"] = pack_linear(take(p + "out.weight", (D, D))), take(p + "out.bias", (D,))
        out[p + "ln2.g"], out[p + "ln2.b"] = take(p + "ln2.weight", (D,)), take(p + "ln2.bias", (D,))
        out[p + "ff1.w"], out[p + "ff1.b"] = pack_linear(take(p + "ff1.weight", (cfg.ff, D))), take(p + "ff1.bias", (cfg.ff,))
        out[p + "ff2.w"], out[p + "ff2.b"] = pack_linear(take(p + "ff2.weight", (D, cfg.ff))), take(p + "ff2.bias", (D,))
    out["lnf.g"], out["lnf.b"] = take("lnf.weight", (D,)), take("lnf.bias", (D,))
    out["head.fc1.w"], out["head.fc1.b"] = take("head.fc1.weight", (cfg.head, D)), take("head.fc1.bias", (cfg.head,))
    out["head.fc2.w"], out["head.fc2.b"] = take("head.fc2.weight", (1, cfg.head)).reshape(cfg.head), take("head.fc2.bias", (1,))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


class XfmScorer(GaitScorer):
    """The network on `device` (backend "device", default) or on the host (backend "host": lmx_h_xfm_forward, no GPU)."""
    _pack = staticmethod(pack_tensors)

    _weights = staticmethod(lambda cfg, tensors: K.xfm_weights(*cfg.shape(), tensors))

    def forward(self, x, mask=None, seeds=None, n_samples=10, trunk=False, saliency=False):
        """x f32 [n, T, input_dim], mask None or uint8 / bool [n, T] (nonzero = masked) -> (pred [n, max(S, 1)], stats [n, 2],
        saliency [n, T] or None, trunk [n, max(S, 1), T, D] or None)."""
        if mask is not None and mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        fn = K.xfm_forward_host if self.backend == "host" else K.xfm_forward
        return fn(self.weights, x, mask, seeds, n_samples, self.cfg.dropout, saliency=saliency, trunk=trunk)

    def score(self, x, mask=None, seeds=None, n_samples=10):
        """(mean [n], unbiased std [n], pred [n, max(S, 1)]); n_samples = 0: eval mode, std = 0."""
        pred, stats, _, _ = self.forward(x, mask, seeds, n_samples)
        return stats[:, 0], stats[:, 1], pred

    def saliency(self, x):
        """f32 [n, T]: the column sums of the last layer's head-averaged attention weights in eval mode WITHOUT a mask, which is what
        the reference's get_attention_weights(x) computes (main.py:435 passes no mask)."""
        return self.forward(x, None, None, 0, saliency=True)[2]
