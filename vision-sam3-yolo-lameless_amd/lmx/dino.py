"""DINO ViT embedder on liblmx — the model call of services/dinov3-pipeline/app/main.py:95-115
(``processor(images=...)`` -> ``model(**inputs).last_hidden_state.mean(dim=1)``).

Two architectures behind one launch sequence:
  * ``dinov2``  — what the service loads by default (facebook/dinov2-base): patch 14, learned position table
                   (bicubic-interpolated to the input grid once, at load), separate q/k/v with bias, eps 1e-6;
                   ``registers > 0`` is dinov2_with_registers (tokens [CLS, registers, patches], the position table
                   added to CLS and patches only).
  * ``dinov3``  — the BASELINE config (ViT-L/16): patch 16, CLS + 4 register tokens, no position table, RoPE on the
                   patch tokens of q/k, key without bias, eps 1e-5.
Layer = LN -> fused qkv GEMM -> (RoPE) -> flash attention -> out-proj GEMM with LayerScale+residual epilogue ->
LN -> fc1 GEMM with GELU epilogue -> fc2 GEMM with LayerScale+residual epilogue.  The residual stream is f32 in
HBM; every GEMM/attention operand is f16 with f32 accumulation.
``gated`` MLPs (DINOv3 ViT-S+/H+ ``down(silu(gate(x)) * up(x))``, DINOv2 giant's SwiGLU FFN): fc1 is ONE GEMM over the
gate and up rows interleaved by 16 (``pack_gated``) whose epilogue is the gate (lmx_k_gemm LMX_ACT_SWIGLU): the
2 x mlp wide intermediate is never written.  Head dims up to 96 (every ViT up to H+ / giant has 64); DINOv3-7B's 128 is refused at load.
Preprocessing is the recipe of the model directory's preprocessor_config.json (``DinoPreprocess``): BitImageProcessor's PIL
u8 path or DINOv3ViTImageProcessor's float antialiased resize; a configuration without one runs dinov2-base's.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from . import resample


@dataclass(frozen=True)
class DinoPreprocess:
    """The computation of the image processor a model directory names (lmx.checkpoints.read_dino_preprocess turns
    ``preprocessor_config.json`` into one).  Two families, two different computations:
      * ``pil``   — BitImageProcessor (dinov2, dinov2_with_registers): Pillow resize on u8 -> centre crop -> rescale -> normalize,
                     bit-exact (lmx_k_pil_resize_* + lmx_k_patchify_norm).
      * ``float`` — DINOv3ViTImageProcessor: rescale -> float32 antialiased resize -> (centre crop) -> normalize
                     (lmx_k_float_resize_patchify).
    The resize target is ``shortest_edge`` (aspect kept, the other side truncated) or ``size_hw`` (the whole frame squashed).
    The defaults are the dinov2-base recipe, the one a DinoConfig without ``preproc`` gets."""
    kind: str = "pil"
    filt: str = resample.BICUBIC  # lmx.resample.BILINEAR | BICUBIC (`resample` 2 | 3)
    shortest_edge: Optional[int] = 256
    size_hw: Optional[Tuple[int, int]] = None
    crop: Optional[int] = 224
    rescale: float = 1.0 / 255.0
    mean: Tuple[float, float, float] = resample.IMAGENET_MEAN
    std: Tuple[float, float, float] = resample.IMAGENET_STD

    @property
    def input_size(self):
        """Side of the square the network is fed: the crop, or the resize target when nothing is cropped."""
        return self.crop if self.crop is not None else self.size_hw[0]

    def resized(self, h, w):
        """(height, width) a frame of h x w is resized to."""
        return tuple(self.size_hw) if self.size_hw is not None else resample.shortest_edge_size(h, w, self.shortest_edge)


@dataclass
class DinoConfig:
    arch: str = "dinov3"          # "dinov3" | "dinov2"
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    mlp: int = 4096
    patch: int = 16
    registers: int = 4
    eps: float = 1e-5
    rope_theta: float = 100.0
    image: int = 224              # crop size fed to the network
    resize_edge: int = 256        # shortest-edge resize before the crop
    pos_grid: int = 37            # dinov2 only: side of the learned position grid (518/14)
    gated: bool = False           # MLP form: down(silu(gate(x)) * up(x)) instead of down(gelu(up(x)))
    # dinov3 only (DINOv3ViTConfig query_bias / key_bias / value_bias / proj_bias / mlp_bias): which projections have a bias
    q_bias: bool = True
    k_bias: bool = False
    v_bias: bool = True
    proj_bias: bool = True
    mlp_bias: bool = True
    # the model directory's preprocessing recipe; None: the dinov2-base recipe with `resize_edge` and `image` (what a config
    # built by hand gets).  When set, `image` is the recipe's input_size
    preproc: Optional[DinoPreprocess] = None

    @property
    def head_dim(self):
        return self.hidden // self.heads

    @property
    def n_prefix(self):
        return 1 + self.registers

    @property
    def grid(self):
        return self.image // self.patch

    @property
    def tokens(self):
        return self.n_prefix + self.grid * self.grid


def dinov3_vitl16():
    return DinoConfig()


def dinov2_base():
    return DinoConfig(arch="dinov2", hidden=768, layers=12, heads=12, mlp=3072, patch=14, registers=0, eps=1e-6)


def dinov3_vitsplus16(**kw):
    """DINOv3 ViT-S+/16: gated MLP."""
    return DinoConfig(**{**dict(hidden=384, layers=12, heads=6, mlp=1536, gated=True), **kw})


def dinov3_vithplus16(**kw):
    """DINOv3 ViT-H+/16: gated MLP."""
    return DinoConfig(**{**dict(hidden=1280, layers=32, heads=20, mlp=5120, gated=True), **kw})


def swiglu_hidden(hidden, mlp_ratio=4):
    """Dinov2SwiGLUFFN's hidden_features (TF:models/dinov2/modeling_dinov2.py): 2/3 of the plain width, rounded up to 8."""
    return (int(int(hidden * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def dinov2_giant(**kw):
    """DINOv2 giant: SwiGLU FFN (hidden_features 4096)."""
    return DinoConfig(**{**dict(arch="dinov2", hidden=1536, layers=40, heads=24, mlp=swiglu_hidden(1536), patch=14, registers=0,
                              eps=1e-6, gated=True), **kw})


def dinov2_reg_base(**kw):
    """DINOv2-with-registers base: 4 register tokens."""
    return DinoConfig(**{**dict(arch="dinov2", hidden=768, layers=12, heads=12, mlp=3072, patch=14, registers=4, eps=1e-6), **kw})


def check_head_dim(cfg):
    """The attention kernels serve head dims up to 96 in multiples of 8; every released DINOv2 / DINOv3 ViT up to H+ has 64.
    DINOv3-7B (128) is refused here rather than mis-run."""
    hd = cfg.head_dim
    if cfg.hidden % cfg.heads or hd % 8 or hd > 96:
        raise K.LmxError(f"head dim {hd} (hidden_size {cfg.hidden} / num_attention_heads {cfg.heads}) is not supported: the attention "
                         "kernels serve multiples of 8 up to 96 (DINOv3-7B, head dim 128, is out of scope)")


def pack_gated(gate, up):
    """Gate and up rows ([I, ...] each) -> the [2I, ...] operand of lmx_k_gemm's LMX_ACT_SWIGLU: blocks of 16 gate rows alternate
    with the 16 up rows of the same channels (g0..g15, u0..u15, g16..), so that a lane of the 16x16 MFMA holds gate and up of
    one output channel in two accumulators of its own.  Works for the [I] biases too."""
    gate, up = np.asarray(gate), np.asarray(up)
    I = gate.shape[0]
    if gate.shape != up.shape or I % 16:
        raise ValueError(f"pack_gated: gate {gate.shape} / up {up.shape}: equal shapes with a multiple of 16 rows")
    rest = gate.shape[1:]
    return np.stack([gate.reshape((I // 16, 16) + rest), up.reshape((I // 16, 16) + rest)], axis=1).reshape((2 * I,) + rest)


def param_spec(cfg):
    """Ordered {HF parameter name: (shape, init kind)} — exactly the tensors transformers' DINOv3ViTModel / Dinov2Model /
    Dinov2WithRegistersModel have for this configuration."""
    D, I, P = cfg.hidden, cfg.mlp, cfg.patch
    s = {}
    if cfg.arch == "dinov3":
        s["embeddings.cls_token"] = ((1, 1, D), "tok")
        s["embeddings.mask_token"] = ((1, 1, D), "zero")
        s["embeddings.register_tokens"] = ((1, cfg.registers, D), "tok")
        s["embeddings.patch_embeddings.weight"] = ((D, 3, P, P), "w")
        s["embeddings.patch_embeddings.bias"] = ((D,), "b")
        for i in range(cfg.layers):
            p = f"model.layer.{i}."
            s[p + "norm1.weight"] = ((D,), "g")
            s[p + "norm1.bias"] = ((D,), "b")
            s[p + "attention.k_proj.weight"] = ((D, D), "w")
            if cfg.k_bias:
                s[p + "attention.k_proj.bias"] = ((D,), "b")
            s[p + "attention.v_proj.weight"] = ((D, D), "w")
            if cfg.v_bias:
                s[p + "attention.v_proj.bias"] = ((D,), "b")
            s[p + "attention.q_proj.weight"] = ((D, D), "w")
            if cfg.q_bias:
                s[p + "attention.q_proj.bias"] = ((D,), "b")
            s[p + "attention.o_proj.weight"] = ((D, D), "w")
            if cfg.proj_bias:
                s[p + "attention.o_proj.bias"] = ((D,), "b")
            s[p + "layer_scale1.lambda1"] = ((D,), "ls")
            s[p + "norm2.weight"] = ((D,), "g")
            s[p + "norm2.bias"] = ((D,), "b")
            for n, shp in ((("gate_proj", (I, D)),) if cfg.gated else ()) + (("up_proj", (I, D)), ("down_proj", (D, I))):
                s[p + f"mlp.{n}.weight"] = (shp, "w")
                if cfg.mlp_bias:
                    s[p + f"mlp.{n}.bias"] = ((shp[0],), "b")
            s[p + "layer_scale2.lambda1"] = ((D,), "ls")
        s["norm.weight"] = ((D,), "g")
        s["norm.bias"] = ((D,), "b")
    else:
        s["embeddings.cls_token"] = ((1, 1, D), "tok")
        s["embeddings.mask_token"] = ((1, D), "zero")
        if cfg.registers:
            s["embeddings.register_tokens"] = ((1, cfg.registers, D), "tok")
        s["embeddings.position_embeddings"] = ((1, 1 + cfg.pos_grid * cfg.pos_grid, D), "tok")
        s["embeddings.patch_embeddings.projection.weight"] = ((D, 3, P, P), "w")
        s["embeddings.patch_embeddings.projection.bias"] = ((D,), "b")
        for i in range(cfg.layers):
            p = f"encoder.layer.{i}."
            s[p + "norm1.weight"] = ((D,), "g")
            s[p + "norm1.bias"] = ((D,), "b")
            for n in ("query", "key", "value"):
                s[p + f"attention.attention.{n}.weight"] = ((D, D), "w")
                s[p + f"attention.attention.{n}.bias"] = ((D,), "b")
            s[p + "attention.output.dense.weight"] = ((D, D), "w")
            s[p + "attention.output.dense.bias"] = ((D,), "b")
            s[p + "layer_scale1.lambda1"] = ((D,), "ls")
            s[p + "norm2.weight"] = ((D,), "g")
            s[p + "norm2.bias"] = ((D,), "b")
            if cfg.gated:  # Dinov2SwiGLUFFN: weights_in = [gate; up] (x1, x2 = chunk(2); silu(x1) * x2)
                s[p + "mlp.weights_in.weight"] = ((2 * I, D), "w")
                s[p + "mlp.weights_in.bias"] = ((2 * I,), "b")
                s[p + "mlp.weights_out.weight"] = ((D, I), "w")
                s[p + "mlp.weights_out.bias"] = ((D,), "b")
            else:
                s[p + "mlp.fc1.weight"] = ((I, D), "w")
                s[p + "mlp.fc1.bias"] = ((I,), "b")
                s[p + "mlp.fc2.weight"] = ((D, I), "w")
                s[p + "mlp.fc2.bias"] = ((D,), "b")
            s[p + "layer_scale2.lambda1"] = ((D,), "ls")
        s["layernorm.weight"] = ((D,), "g")
        s["layernorm.bias"] = ((D,), "b")
    return s


def rope_tables(cfg, gh, gw):
    """cos/sin f32 [gh*gw, head_dim] exactly as DINOv3ViTRopePositionEmbedding.forward builds them
    (TF:models/dinov3_vit/modeling_dinov3_vit.py:153-200): f32 torch ops on the host, once per grid shape."""
    hd = cfg.head_dim
    inv_freq = 1 / cfg.rope_theta ** torch.arange(0, 1, 4 / hd, dtype=torch.float32)
    ch = torch.arange(0.5, gh, dtype=torch.float32) / gh
    cw = torch.arange(0.5, gw, dtype=torch.float32) / gw
    coords = torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1)
    coords = 2.0 * coords - 1.0
    angles = 2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]
    angles = angles.flatten(1, 2).tile(2)
    return torch.cos(angles).contiguous(), torch.sin(angles).contiguous()


def interpolate_pos_embed(pos, grid_in, grid_out, antialias=False):
    """Dinov2Embeddings.interpolate_pos_encoding (TF:models/dinov2/modeling_dinov2.py:57-95): bicubic,
    align_corners=False, computed in f32 on the host once at load.  pos: torch [1, 1+gi*gi, D].
    antialias=True: Dinov2WithRegistersEmbeddings' form (TF:models/dinov2_with_registers/modeling_dinov2_with_registers.py:128-134),
    which low-pass filters the table when it shrinks it."""
    if grid_in == grid_out:
        return pos
    cls, patch = pos[:, :1], pos[:, 1:]
    D = pos.shape[-1]
    patch = patch.reshape(1, grid_in, grid_in, D).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch.to(torch.float32), size=(grid_out, grid_out), mode="bicubic",
                                            align_corners=False, antialias=antialias)
    patch = patch.permute(0, 2, 3, 1).reshape(1, -1, D)
    return torch.cat((cls, patch), dim=1)


class DinoEmbedder:
    """Device-resident DINO ViT.  ``embed_patches`` is the network proper (cfg#4 input: already-preprocessed
    frames as a patch matrix), ``embed_frames`` adds the service's preprocessing from raw BGR u8 frames."""

    def __init__(self, cfg, state_dict, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        dev = self.device
        D, P = cfg.hidden, cfg.patch

        def t32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def t16(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(torch.float16).contiguous()

        sd = state_dict
        v3 = cfg.arch == "dinov3"
        check_head_dim(cfg)
        gate_key = ("model.layer.0.mlp.gate_proj.weight" if v3 else "encoder.layer.0.mlp.weights_in.weight")
        if cfg.gated != (gate_key in sd):
            raise K.LmxError(f"DinoEmbedder: gated={cfg.gated} but the state dict {'has' if gate_key in sd else 'lacks'} {gate_key}")

        def zeros(n):
            return np.zeros(n, np.float32)
        pe_w = sd["embeddings.patch_embeddings.weight" if v3 else "embeddings.patch_embeddings.projection.weight"]
        pe_b = sd["embeddings.patch_embeddings.bias" if v3 else "embeddings.patch_embeddings.projection.bias"]
        # conv weight [D,3,P,P] -> GEMM weight [D, (ky,kx,c)], K padded to a multiple of 8 with zero columns
        k_raw = P * P * 3
        self.k_pad = (k_raw + 7) // 8 * 8
        w = np.transpose(pe_w, (0, 2, 3, 1)).reshape(D, k_raw)
        if self.k_pad != k_raw:
            w = np.concatenate([w, np.zeros((D, self.k_pad - k_raw), np.float32)], axis=1)
        self.pe_w, self.pe_b = t16(w), t32(pe_b)
        if v3:
            prefix = np.concatenate([sd["embeddings.cls_token"][0], sd["embeddings.register_tokens"][0]], axis=0)
            self.pos = None
            self.rope = tuple(t.to(dev) for t in rope_tables(cfg, cfg.grid, cfg.grid))
        else:
            prefix = sd["embeddings.cls_token"][0]
            pos = interpolate_pos_embed(torch.from_numpy(sd["embeddings.position_embeddings"]), cfg.pos_grid, cfg.grid,
                                        antialias=cfg.registers > 0)
            pos = pos[0].to(torch.float32).contiguous()
            if cfg.registers:
                # Dinov2WithRegistersEmbeddings.forward: the position table is added to [CLS, patches] BEFORE the registers are
                # inserted behind CLS.  Prefix rows = CLS + pos[0] (the same f32 sum), then the registers; the table handed to
                # assemble_tokens is zero over the prefix rows and pos[1:] over the patches
                prefix = np.concatenate([prefix + pos[:1].numpy(), sd["embeddings.register_tokens"][0]], axis=0)
                pos = torch.cat([torch.zeros((cfg.n_prefix, D), dtype=torch.float32), pos[1:]], dim=0)
            self.pos = pos.contiguous().to(dev)
            self.rope = None
        self.prefix = t32(prefix)
        self.layers = []
        for i in range(cfg.layers):
            if v3:
                p = f"model.layer.{i}."
                qw, kw, vw = (sd[p + f"attention.{n}_proj.weight"] for n in "qkv")
                # absent biases (query_bias / key_bias / value_bias / proj_bias / mlp_bias false) are zeros
                qb, kb, vb = (sd.get(p + f"attention.{n}_proj.bias", zeros(D)) for n in "qkv")
                ow, ob = sd[p + "attention.o_proj.weight"], sd.get(p + "attention.o_proj.bias", zeros(D))
                w1, b1 = sd[p + "mlp.up_proj.weight"], sd.get(p + "mlp.up_proj.bias", zeros(cfg.mlp))
                w2, b2 = sd[p + "mlp.down_proj.weight"], sd.get(p + "mlp.down_proj.bias", zeros(D))
                if cfg.gated:
                    w1 = pack_gated(sd[p + "mlp.gate_proj.weight"], w1)
                    b1 = pack_gated(sd.get(p + "mlp.gate_proj.bias", zeros(cfg.mlp)), b1)
            else:
                p = f"encoder.layer.{i}."
                qw, kw, vw = (sd[p + f"attention.attention.{n}.weight"] for n in ("query", "key", "value"))
                qb, kb, vb = (sd[p + f"attention.attention.{n}.bias"] for n in ("query", "key", "value"))
                ow, ob = sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"]
                if cfg.gated:
                    wi, bi = sd[p + "mlp.weights_in.weight"], sd[p + "mlp.weights_in.bias"]
                    w1, b1 = pack_gated(wi[:cfg.mlp], wi[cfg.mlp:]), pack_gated(bi[:cfg.mlp], bi[cfg.mlp:])
                    w2, b2 = sd[p + "mlp.weights_out.weight"], sd[p + "mlp.weights_out.bias"]
                else:
                    w1, b1 = sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]
                    w2, b2 = sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]
            self.layers.append(dict(
                g1=t32(sd[p + "norm1.weight"]), b1=t32(sd[p + "norm1.bias"]),
                wqkv=t16(np.concatenate([qw, kw, vw], 0)), bqkv=t32(np.concatenate([qb, kb, vb], 0)),
                wo=t16(ow), bo=t32(ob), ls1=t32(sd[p + "layer_scale1.lambda1"]),
                g2=t32(sd[p + "norm2.weight"]), b2=t32(sd[p + "norm2.bias"]),
                w1=t16(w1), bb1=t32(b1), w2=t16(w2), bb2=t32(b2), ls2=t32(sd[p + "layer_scale2.lambda1"])))
        self.gf = t32(sd["norm.weight" if v3 else "layernorm.weight"])
        self.bf = t32(sd["norm.bias" if v3 else "layernorm.bias"])
        self.recipe = cfg.preproc if cfg.preproc is not None else DinoPreprocess(shortest_edge=cfg.resize_edge, crop=cfg.image)
        if self.recipe.kind not in ("pil", "float") or self.recipe.input_size != cfg.image:
            raise K.LmxError(f"DinoEmbedder: the preprocessing recipe ({self.recipe.kind}) feeds {self.recipe.input_size} x "
                             f"{self.recipe.input_size}, the configuration's image is {cfg.image}")
        self.lut = t32(resample.norm_lut(self.recipe.mean, self.recipe.std, self.recipe.rescale))
        self._tabs = {}

    # ---- the network --------------------------------------------------------------------------------------
    def hidden_states(self, patches, B):
        """patches f16 [B*np, k_pad] -> final-LayerNorm'ed tokens f32 [B*T, D]."""
        cfg = self.cfg
        D, H, hd, T = cfg.hidden, cfg.heads, cfg.head_dim, cfg.tokens
        np_ = cfg.grid * cfg.grid
        xp = K.gemm(patches, self.pe_w, bias=self.pe_b)
        x = K.assemble_tokens(xp, self.prefix, self.pos, B, np_, cfg.n_prefix, D)
        scale = hd ** -0.5
        act1 = K.ACT_SWIGLU if cfg.gated else K.ACT_GELU
        for L in self.layers:
            h = K.layernorm(x, L["g1"], L["b1"], cfg.eps)
            qkv = K.gemm(h, L["wqkv"], bias=L["bqkv"])
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            if self.rope is not None:
                K.rope(q, B, T, H, hd, cfg.n_prefix, *self.rope)
                K.rope(k, B, T, H, hd, cfg.n_prefix, *self.rope)
            a = torch.empty((B * T, D), dtype=torch.float16, device=x.device)
            K.attention(q, k, v, a, B, H, T, T, hd, scale)
            K.gemm(a, L["wo"], bias=L["bo"], scale=L["ls1"], res=x, out=x)
            h = K.layernorm(x, L["g2"], L["b2"], cfg.eps)
            u = K.gemm(h, L["w1"], bias=L["bb1"], act=act1)
            K.gemm(u, L["w2"], bias=L["bb2"], scale=L["ls2"], res=x, out=x)
        return K.layernorm(x, self.gf, self.bf, cfg.eps, out_dtype=torch.float32)

    def embed_patches(self, patches, B):
        """-> f32 [B, D]: mean over ALL tokens of last_hidden_state (dinov3 main.py:113)."""
        y = self.hidden_states(patches, B)
        return K.token_mean(y, B, self.cfg.tokens, self.cfg.hidden)

    # ---- preprocessing (K21) ------------------------------------------------------------------------------
    def _tables(self, h, w):
        key = (h, w)
        if key not in self._tabs:
            rc = self.recipe
            nh, nw = rc.resized(h, w)
            if nh < self.cfg.image or nw < self.cfg.image:
                raise K.LmxError(f"frame {h}x{w} resizes to {nh}x{nw}, smaller than the {self.cfg.image} crop")
            dev = self.device

            def up(tab):
                b, k, ks = tab
                return (torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), ks)

            if rc.kind == "pil":
                # the horizontal pass always runs: it also does the BGR->RGB swap (identity table if the width is kept)
                th = up(resample.coeff_tables(w, nw, rc.filt)) if nw != w else up(_identity_table(w))
                tv = up(resample.coeff_tables(h, nh, rc.filt)) if nh != h else None
                self._tabs[key] = (nh, nw, th, tv)
            else:
                # the centre crop of the resized image (TorchvisionBackend.center_crop: int((size - crop) / 2)) is a slice of
                # the tables: only the rows and columns that survive it are ever computed
                S = self.cfg.image

                def cut(tab, n_out):
                    b, k, ks = tab
                    o = int((n_out - S) / 2.0)
                    return np.ascontiguousarray(b.reshape(-1, 2)[o:o + S]).reshape(-1), np.ascontiguousarray(k.reshape(-1, ks)[o:o + S]).reshape(-1), ks

                th, tv = cut(resample.aa_tables(w, nw, rc.filt), nw), cut(resample.aa_tables(h, nh, rc.filt), nh)
                self._tabs[key] = (up(th), up(tv), resample.segment_cols(th[0]))
        return self._tabs[key]

    def preprocess(self, frames_bgr, rgb=False):
        """u8 [B,H,W,3] BGR (cv2 order; `rgb=True`: already RGB, as the PIL image the glue hands the processor) on device
        -> f16 patch matrix [B*np, k_pad], by the recipe of the model directory (`cfg.preproc`; none: dinov2-base's):
          pil   : cvtColor(BGR2RGB) -> PIL resize on u8 -> center crop -> rescale -> normalise
          float : cvtColor(BGR2RGB) -> rescale -> float32 antialiased resize -> (center crop) -> normalise, one kernel."""
        cfg, rc = self.cfg, self.recipe
        B, h, w, _ = frames_bgr.shape
        if rc.kind == "float":
            th, tv, seg = self._tables(h, w)
            return K.float_resize_patchify(frames_bgr, cfg.grid, cfg.grid, cfg.patch, th, tv, seg, rc.rescale, rc.mean, rc.std,
                                           swap_rb=not rgb, k_pad=self.k_pad)
        nh, nw, th, tv = self._tables(h, w)
        img = K.pil_resize(frames_bgr, nw, nh, th, tv, swap_rb=not rgb)
        top, left = (nh - cfg.image) // 2, (nw - cfg.image) // 2
        return K.patchify_norm(img, top, left, cfg.grid, cfg.grid, cfg.patch, self.lut, k_pad=self.k_pad)

    def embed_frames(self, frames_bgr):
        return self.embed_patches(self.preprocess(frames_bgr), frames_bgr.shape[0])


def _identity_table(n):
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], 1).reshape(-1)
    kk = np.full((n,), 1 << resample.PRECISION_BITS, dtype=np.int32)
    return bounds, kk, 1
