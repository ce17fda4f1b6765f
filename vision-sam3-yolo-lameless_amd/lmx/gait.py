"""What the gait sequence models (``lmx.tcn``, ``lmx.xfm``) have in common on the Python side: the operand order of a packed
convolution (csrc/gait.h), the seed of a clip, and the scorer that holds a network's packed tensors on the device or on the host."""
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
