"""Regenerates the golden vectors of the gated-MLP / register-token DINO configurations (tests/test_gpu_dino_family.py).
Run on a CPU box:  python tests/golden/make_golden_dino_family.py [name ...]

As tests/golden/make_golden.py does for ViT-L/16 and DINOv2-B: transformers' DINOv3ViTModel / Dinov2Model /
Dinov2WithRegistersModel built from config objects (eager attention, fp32, CPU), filled with the build's deterministic
synthetic weights (lmx.weights, seed in the file name), fed by the PIL image processor.  Stored: seeds, frame ids, the
configuration (factory name in lmx.dino + keyword arguments), the token-mean embedding, and last_hidden_state on a token
subset (all prefix tokens and every 16th patch token: the full tensor of a 1280-wide model is 2 MB) — no weights.

For the DINOv3 gated configurations the file also records `plain_mlp_cos`: the cosine between the golden embedding and the
embedding of the SAME weights evaluated as a plain MLP, down(gelu(up(x))), gate ignored — what a loader that does not
know `use_gated_mlp` computes.  It must miss the 1 - 1e-4 bar (asserted here), i.e. the bar can tell the two apart."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), HERE]

from lmx import dino, synth, weights  # noqa: E402
from make_golden import hf_pixel_values  # noqa: E402

BAR = 1 - 1e-4

# name -> (factory in lmx.dino, kwargs, weight seed, clip seed, frame ids).  Real widths and full depth everywhere.
CONFIGS = {
    "dinov3_vithplus16_w11": ("dinov3_vithplus16", {}, 11, 31, (5, 120)),
    # every bias the config can switch off is off (key_bias is off by default)
    "dinov3_vitsplus16_nobias_w12": ("dinov3_vitsplus16", dict(q_bias=False, v_bias=False, proj_bias=False, mlp_bias=False),
                                     12, 32, (17, 88)),
    "dinov2_giant_w13": ("dinov2_giant", {}, 13, 33, (2, 140)),
    "dinov2_reg_base_w14": ("dinov2_reg_base", {}, 14, 34, (60, 61)),
}


def hf_model(cfg, gated=None):
    gated = cfg.gated if gated is None else gated
    if cfg.arch == "dinov3":
        from transformers import DINOv3ViTConfig, DINOv3ViTModel

        c = DINOv3ViTConfig(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers,
                            num_attention_heads=cfg.heads, num_register_tokens=cfg.registers, patch_size=cfg.patch,
                            layer_norm_eps=cfg.eps, rope_theta=cfg.rope_theta, image_size=cfg.image, use_gated_mlp=gated,
                            hidden_act="silu" if gated else "gelu", query_bias=cfg.q_bias, key_bias=cfg.k_bias,
                            value_bias=cfg.v_bias, proj_bias=cfg.proj_bias, mlp_bias=cfg.mlp_bias, attn_implementation="eager")
        return DINOv3ViTModel(c).eval()
    kw = dict(hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, mlp_ratio=4,
              use_swiglu_ffn=gated, patch_size=cfg.patch, image_size=cfg.pos_grid * cfg.patch, layer_norm_eps=cfg.eps,
              attn_implementation="eager")
    if cfg.registers:
        from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel

        return Dinov2WithRegistersModel(Dinov2WithRegistersConfig(num_register_tokens=cfg.registers, **kw)).eval()
    from transformers import Dinov2Config, Dinov2Model

    return Dinov2Model(Dinov2Config(**kw)).eval()


def token_subset(cfg):
    return np.concatenate([np.arange(cfg.n_prefix), np.arange(cfg.n_prefix, cfg.tokens, 16)])


def make(name):
    factory, kw, seed, clip_seed, frame_ids = CONFIGS[name]
    cfg = getattr(dino, factory)(**kw)
    sd = weights.synth_state_dict(dino.param_spec(cfg), seed)
    frames = np.stack([synth.synth_frame(clip_seed, i) for i in frame_ids], 0)
    pv = hf_pixel_values(frames)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        m = hf_model(cfg)
        m.load_state_dict(tsd, strict=True)
        hs = m(pixel_values=pv).last_hidden_state
        emb = hs.mean(dim=1)  # services/dinov3-pipeline/app/main.py:113
    assert tuple(hs.shape) == (len(frame_ids), cfg.tokens, cfg.hidden), hs.shape
    out = dict(embedding=emb.numpy(), token_ids=token_subset(cfg), hidden_tokens=hs[:, token_subset(cfg)].numpy(),
               factory=factory, kwargs=json.dumps(kw), weight_seed=seed, clip_seed=clip_seed, frame_ids=np.asarray(frame_ids),
               pixel_checksum=np.asarray([int(pv.double().abs().sum() * 1000)]))
    if cfg.arch == "dinov3" and cfg.gated:
        with torch.no_grad():
            del m
            pm = hf_model(cfg, gated=False)
            pm.load_state_dict({k: v for k, v in tsd.items() if ".mlp.gate_proj." not in k}, strict=True)
            pe = pm(pixel_values=pv).last_hidden_state.mean(dim=1)
        cos = torch.nn.functional.cosine_similarity(emb.double(), pe.double(), dim=1)
        print(name, "plain-MLP evaluation of the gated weights: cos", cos.tolist())
        assert float(cos.max()) < BAR, f"{name}: the bar does not detect the ignored gate, pick another seed ({cos.tolist()})"
        out["plain_mlp_cos"] = cos.numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "tokens", cfg.tokens, "embedding norm", emb.norm(dim=1).tolist(), "->", os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    for n in sys.argv[1:] or CONFIGS:
        make(n)
