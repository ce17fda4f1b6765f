"""The TCN gait model of services/tcn-pipeline (main.py:22-195) on liblmx: a lameness severity score and its MC-dropout spread from a
pose series, in ONE launch for a batch of clips (csrc/tcn.hip; include/lmx.h "The TCN gait model" has the network and the keep bits).

``TcnConfig`` is the network's shape, ``pack_tensors`` turns the FOLDED weights (``lmx.checkpoints.tcn_from_state_dict``) into the
tensors the kernel and the weight image hold, ``TcnScorer`` scores clips on the device or, with ``backend="host"``, through the
plain C++ forward ``lmx_h_tcn_forward`` without a GPU.  There is no torch arithmetic here."""
import dataclasses

import numpy as np
import torch

from . import kernels as K
from ._lib import LmxError
from .gait import GaitScorer, clip_seed, pack_conv  # noqa: F401 — the seeds and the operand order are every gait model's

MAX_BLOCKS, MAX_CH, MAX_T, MAX_HEAD = 8, 64, 256, 64


@dataclasses.dataclass(frozen=True)
class TcnConfig:
    """services/tcn-pipeline/app/main.py:232-239 by default: 44 features, four blocks of 64 channels, k = 3, p = 0.2, a head of 32."""
    input_dim: int = 44
    channels: tuple = (64, 64, 64, 64)
    kernel_size: int = 3
    dropout: float = 0.2
    head: int = 32

    @property
    def n_blocks(self):
        return len(self.channels)

    @property
    def n_sites(self):
        return 2 * len(self.channels) + 1

    @property
    def receptive_field(self):
        return 1 + 2 * (self.kernel_size - 1) * (2 ** len(self.channels) - 1)

    def block_inputs(self, i):
        return self.channels[i - 1] if i else self.input_dim

    def validate(self, who="TcnConfig"):
        """The list of include/lmx.h; LmxError names the field."""
        K.tcn_check_config(who, self.input_dim, self.channels, self.kernel_size, self.head)
        if not 0.0 <= self.dropout < 1.0:
            raise LmxError(f"{who}: p {self.dropout} outside [0, 1)")
        return self


def pack_tensors(cfg, folded):
    """Ordered {image tensor name: f32 numpy array} from the folded weights (checkpoints.tcn_from_state_dict)."""
    cfg.validate("pack_tensors")
    out = {}
    f = {k: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32) for k, v in folded.items()}
    for i, n in enumerate(cfg.channels):
        cin = cfg.block_inputs(i)
        for s, c_in in (("conv1", cin), ("conv2", n)):
            w = f[f"block.{i}.{s}.weight"]
            if w.shape != (n, c_in, cfg.kernel_size):
                raise LmxError(f"pack_tensors: block.{i}.{s}.weight has shape {w.shape}, the configuration calls for {(n, c_in, cfg.kernel_size)}")
            out[f"block.{i}.{s}.w"] = pack_conv(w)
            out[f"block.{i}.{s}.b"] = f[f"block.{i}.{s}.bias"].reshape(n)
        if cin != n:
            out[f"block.{i}.res.w"] = pack_conv(f[f"block.{i}.res.weight"].reshape(n, cin, 1))
            out[f"block.{i}.res.b"] = f[f"block.{i}.res.bias"].reshape(n)
    c = cfg.channels[-1]
    out["head.fc1.w"] = f["head.fc1.weight"].reshape(cfg.head, c)
    out["head.fc1.b"] = f["head.fc1.bias"].reshape(cfg.head)
    out["head.fc2.w"] = f["head.fc2.weight"].reshape(cfg.head)
    out["head.fc2.b"] = f["head.fc2.bias"].reshape(1)
    return out


class TcnScorer(GaitScorer):
    """The network on `device` (backend "device", default) or on the host (backend "host": lmx_h_tcn_forward, no GPU)."""
    _pack = staticmethod(pack_tensors)

    _weights = staticmethod(lambda cfg, tensors: K.tcn_weights(cfg.input_dim, cfg.channels, cfg.kernel_size, cfg.head, tensors))

    def forward(self, x, seeds, n_samples=10, trunk=False):
        """x f32 [n, T, input_dim] -> (pred [n, max(S, 1)], stats [n, 2], trunk [n, max(S, 1), T, C] or None)."""
        if self.backend == "host":
            return K.tcn_forward_host(self.weights, x, seeds, n_samples, self.cfg.dropout, trunk=trunk)
        return K.tcn_forward(self.weights, x, seeds, n_samples, self.cfg.dropout, trunk=trunk)

    def score(self, x, seeds, n_samples=10):
        """(mean [n], unbiased std [n], pred [n, max(S, 1)]); n_samples = 0: eval mode, std = 0."""
        pred, stats, _ = self.forward(x, seeds, n_samples)
        return stats[:, 0], stats[:, 1], pred
