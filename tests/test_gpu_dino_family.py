"""The gated-MLP / register-token DINO configurations on the GPU against transformers' fp32 outputs
(tests/golden/make_golden_dino_family.py): DINOv3 ViT-H+/16 and ViT-S+/16 (gated MLP; S+ with every optional bias off), DINOv2
giant (SwiGLU FFN) and DINOv2-with-registers base — real widths, full depth, synthetic weights, raw 1080p frames.
Bar as in tests/test_gpu_dino.py (BASELINE.json north_star): embedding cosine >= 1 - 1e-4; per token, max abs error < 3e-2 and
cosine > 1 - 1e-4 on the stored token subset."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["dinov3_vithplus16_w11", "dinov3_vitsplus16_nobias_w12", "dinov2_giant_w13", "dinov2_reg_base_w14"]
BAR = 1 - 1e-4


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


def _load(name):
    from lmx import dino, synth, weights

    g = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = getattr(dino, str(g["factory"]))(**json.loads(str(g["kwargs"])))
    sd = weights.synth_state_dict(dino.param_spec(cfg), int(g["weight_seed"]))
    frames = np.stack([synth.synth_frame(int(g["clip_seed"]), int(i)) for i in g["frame_ids"]], 0)
    return g, cfg, sd, frames


@pytest.mark.parametrize("name", NAMES)
def test_family_matches_golden(cuda, name):
    """Embedding from raw frames against the stored token mean; hidden states per token; frame 0 alone against frame 0 in a batch
    of 8 (fc1 then runs in the register-staged kernel and in the LDS-DMA kernel: M = tokens vs 8 x tokens >= 512)."""
    from lmx import dino

    g, cfg, sd, frames = _load(name)
    assert cfg.head_dim == 64
    m = dino.DinoEmbedder(cfg, sd, cuda)
    d_frames = torch.from_numpy(frames).to(cuda)
    emb = m.embed_frames(d_frames).cpu()
    ref = torch.from_numpy(g["embedding"])
    cos = _cos(emb, ref)
    print(name, "embedding cos", cos.tolist(), "1 - cos", (1 - cos).tolist(), "max abs", float((emb - ref).abs().max()))
    hs = m.hidden_states(m.preprocess(d_frames), len(frames)).cpu().view(len(frames), cfg.tokens, cfg.hidden)
    sub = hs[:, torch.from_numpy(g["token_ids"]).long()]
    href = torch.from_numpy(g["hidden_tokens"])
    err, tcos = float((sub - href).abs().max()), float(_cos(sub, href).min())
    print(name, "per-token max abs err", err, "min cos", tcos)
    assert float(cos.min()) >= BAR, cos.tolist()
    assert err < 3e-2, err
    assert tcos > BAR, tcos
    batch = d_frames[[0, 1, 0, 1, 1, 0, 1, 1]].contiguous()
    e8 = m.embed_frames(batch)
    e1 = m.embed_frames(d_frames[:1].contiguous())
    assert torch.equal(e1[0], e8[0]) and torch.equal(e8[0], e8[2]) and torch.equal(e8[0].cpu(), emb[0]), \
        "the embedding of a frame depends on the batch it rides in"


@pytest.mark.parametrize("name", ["dinov3_vithplus16_w11", "dinov3_vitsplus16_nobias_w12"])
def test_bar_detects_an_ignored_gate(cuda, name):
    """Negative control.  (a) recorded when the fixture was made: transformers' plain-MLP evaluation of the gated weights misses
    the bar on the CPU; (b) here: the embedder built as a plain MLP from the same weights minus the gate tensors — what the loader
    did before it read use_gated_mlp — misses it too, so a pass of test_family_matches_golden is not blind to the MLP form."""
    import dataclasses

    from lmx import dino

    g, cfg, sd, frames = _load(name)
    assert float(g["plain_mlp_cos"].max()) < BAR, g["plain_mlp_cos"]
    plain = dataclasses.replace(cfg, gated=False, layers=cfg.layers)
    sd_plain = {k: v for k, v in sd.items() if ".mlp.gate_proj." not in k}
    emb = dino.DinoEmbedder(plain, sd_plain, cuda).embed_frames(torch.from_numpy(frames).to(cuda)).cpu()
    cos = _cos(emb, torch.from_numpy(g["embedding"]))
    print(name, "plain-MLP plan on gated weights: cos", cos.tolist(), "(transformers, fp32:", g["plain_mlp_cos"].tolist(), ")")
    assert float(cos.max()) < BAR
    with pytest.raises(RuntimeError, match="gate_proj"):
        dino.DinoEmbedder(plain, sd, cuda)  # gated tensors into a plain plan: refused, not mis-run


def test_adapter_from_a_gated_model_dir(cuda, tmp_path):
    """LmxDinoModel.from_pretrained + LmxImageProcessor on a directory holding a gated DINOv3 config (ViT-S+/16 widths, 2 layers)
    give the tensor the embedder gives."""
    from safetensors.numpy import save_file

    from lmx import adapters, dino, synth, weights

    cfg = dino.dinov3_vitsplus16(layers=2)
    sd = weights.synth_state_dict(dino.param_spec(cfg), 5)
    hf = {"model_type": "dinov3_vit", "hidden_size": 384, "num_hidden_layers": 2, "num_attention_heads": 6, "intermediate_size": 1536,
          "patch_size": 16, "num_register_tokens": 4, "layer_norm_eps": 1e-5, "rope_theta": 100.0, "use_gated_mlp": True,
          "hidden_act": "silu"}
    (tmp_path / "config.json").write_text(json.dumps(hf))
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    model = adapters.LmxDinoModel.from_pretrained(str(tmp_path), device=cuda)
    assert model.config == cfg
    proc = adapters.LmxImageProcessor.from_pretrained(model)
    frame = synth.synth_frame(6, 3)
    rgb = np.ascontiguousarray(frame[:, :, ::-1])
    out = model(**proc(images=rgb, return_tensors="pt")).last_hidden_state
    m = dino.DinoEmbedder(cfg, sd, cuda)
    d = torch.from_numpy(frame[None]).to(cuda)
    want = m.hidden_states(m.preprocess(d), 1).view(1, cfg.tokens, cfg.hidden)
    assert torch.equal(out, want)
    assert torch.equal(out.mean(dim=1), want.mean(dim=1))
