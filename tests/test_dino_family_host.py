"""Host side of the gated-MLP / register-token DINO support (no GPU): param_spec against transformers' own models, what
load_dino_dir reads from config.json and what it refuses, and the interleaved fc1 packing against a float64 model of
lmx_k_gemm's LMX_ACT_SWIGLU epilogue."""
import json

import numpy as np
import pytest
import torch

from lmx import checkpoints as CK
from lmx import dino, weights

V3 = dict(model_type="dinov3_vit", patch_size=16, num_register_tokens=4, layer_norm_eps=1e-5, rope_theta=100.0)
V2 = dict(patch_size=14, image_size=518, layer_norm_eps=1e-6, mlp_ratio=4)
NOBIAS = dict(q_bias=False, v_bias=False, proj_bias=False, mlp_bias=False)

# name -> (DinoConfig at 2 layers, config.json of the same model)
FAMILY = {
    "dinov3_vithplus16": (dino.dinov3_vithplus16(layers=2),
                          dict(V3, hidden_size=1280, num_hidden_layers=2, num_attention_heads=20, intermediate_size=5120,
                               use_gated_mlp=True, hidden_act="silu")),
    "dinov3_vitsplus16_nobias": (dino.dinov3_vitsplus16(layers=2, **NOBIAS),
                                 dict(V3, hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=1536,
                                      use_gated_mlp=True, hidden_act="silu", query_bias=False, key_bias=False, value_bias=False,
                                      proj_bias=False, mlp_bias=False)),
    "dinov3_plain_keybias": (dino.DinoConfig(hidden=384, layers=2, heads=6, mlp=1536, k_bias=True),
                             dict(V3, hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=1536,
                                  key_bias=True, hidden_act="gelu")),
    "dinov2_giant": (dino.dinov2_giant(layers=2),
                     dict(V2, model_type="dinov2", hidden_size=1536, num_hidden_layers=2, num_attention_heads=24, use_swiglu_ffn=True)),
    "dinov2_reg_base": (dino.dinov2_reg_base(layers=2),
                        dict(V2, model_type="dinov2_with_registers", hidden_size=768, num_hidden_layers=2, num_attention_heads=12,
                             num_register_tokens=4)),
    "dinov2_reg_giant": (dino.dinov2_giant(layers=2, registers=4),
                         dict(V2, model_type="dinov2_with_registers", hidden_size=1536, num_hidden_layers=2, num_attention_heads=24,
                              num_register_tokens=4, use_swiglu_ffn=True)),
}


def _hf_meta(hf):
    import transformers as T

    cls = {"dinov3_vit": (T.DINOv3ViTConfig, T.DINOv3ViTModel), "dinov2": (T.Dinov2Config, T.Dinov2Model),
           "dinov2_with_registers": (T.Dinov2WithRegistersConfig, T.Dinov2WithRegistersModel)}[hf["model_type"]]
    kw = {k: v for k, v in hf.items() if k != "model_type"}
    with torch.device("meta"):
        return cls[1](cls[0](**kw))


@pytest.mark.parametrize("name", list(FAMILY))
def test_param_spec_is_transformers_state_dict(name):
    cfg, hf = FAMILY[name]
    sd = _hf_meta(hf).state_dict()
    spec = dino.param_spec(cfg)
    assert set(spec) == set(sd), sorted(set(spec) ^ set(sd))[:6]
    for k, (shape, _) in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k


def test_real_sizes_of_the_factories():
    """The table of the model cards: width / heads / depth and the MLP's inner width."""
    f = [dino.dinov3_vitsplus16(), dino.dinov3_vithplus16(), dino.dinov2_giant(), dino.dinov2_reg_base()]
    assert [(c.hidden, c.heads, c.layers, c.mlp, c.gated, c.registers) for c in f] == [
        (384, 6, 12, 1536, True, 4), (1280, 20, 32, 5120, True, 4), (1536, 24, 40, 4096, True, 0), (768, 12, 12, 3072, False, 4)]
    assert all(c.head_dim == 64 for c in f)
    assert dino.dinov2_reg_base().tokens == 1 + 4 + 16 * 16 and dino.dinov2_giant().n_prefix == 1


def _small(hf, **over):
    """A narrow model of the same form (the loader reads every size from config.json)."""
    h = dict(hf, hidden_size=128, num_attention_heads=2, num_hidden_layers=1)
    if "intermediate_size" in h:
        h["intermediate_size"] = 256
    h.update(over)
    return h


def _write(tmp_path, hf, sd):
    from safetensors.numpy import save_file

    (tmp_path / "config.json").write_text(json.dumps(hf))
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(tmp_path / "model.safetensors"))


@pytest.mark.parametrize("name", list(FAMILY))
def test_load_dino_dir_reads_the_form_from_config(tmp_path, name):
    cfg_full, hf_full = FAMILY[name]
    hf = _small(hf_full)
    sd_meta = _hf_meta(hf).state_dict()
    sd = {k: np.full(tuple(v.shape), 0.01, np.float32) for k, v in sd_meta.items()}
    _write(tmp_path, hf, sd)
    cfg, sd2 = CK.load_dino_dir(tmp_path)
    assert (cfg.arch, cfg.gated, cfg.registers) == (cfg_full.arch, cfg_full.gated, cfg_full.registers)
    assert (cfg.q_bias, cfg.k_bias, cfg.v_bias, cfg.proj_bias, cfg.mlp_bias) == \
        (cfg_full.q_bias, cfg_full.k_bias, cfg_full.v_bias, cfg_full.proj_bias, cfg_full.mlp_bias)
    assert (cfg.hidden, cfg.heads, cfg.layers) == (128, 2, 1)
    assert cfg.mlp == (344 if (cfg.arch == "dinov2" and cfg.gated) else 256 if cfg.arch == "dinov3" else 512)  # (int(512*2/3)+7)//8*8
    assert set(dino.param_spec(cfg)) == set(sd2) == set(sd)


def test_head_dim_128_is_refused(tmp_path):
    hf = _small(FAMILY["dinov3_vithplus16"][1], hidden_size=256, num_attention_heads=2)
    _write(tmp_path, hf, {})
    with pytest.raises(RuntimeError, match=r"head dim 128.*hidden_size 256.*num_attention_heads 2"):
        CK.load_dino_dir(tmp_path)


@pytest.mark.parametrize("name", ["dinov3_vithplus16", "dinov2_giant"])
def test_gated_config_without_gate_tensor_is_refused(tmp_path, name):
    """Gated config, plain checkpoint.  (For DINOv3 the up / down tensors alone satisfy every other check.)"""
    hf = _small(FAMILY[name][1])
    plain = dict(hf, use_gated_mlp=False, use_swiglu_ffn=False, hidden_act="gelu")
    sd = {k: np.zeros(tuple(v.shape), np.float32) for k, v in _hf_meta(plain).state_dict().items()}
    _write(tmp_path, hf, sd)
    with pytest.raises(RuntimeError, match=r"(use_gated_mlp|use_swiglu_ffn)=true.*no gate tensor"):
        CK.load_dino_dir(tmp_path)


@pytest.mark.parametrize("name", ["dinov3_vithplus16", "dinov2_giant"])
def test_plain_config_with_gate_tensor_is_refused(tmp_path, name):
    """Plain config, gated checkpoint: for DINOv3 this loaded and ran down(gelu(up(x))) before — wrong embeddings, silently."""
    hf = _small(FAMILY[name][1])
    sd = {k: np.zeros(tuple(v.shape), np.float32) for k, v in _hf_meta(hf).state_dict().items()}
    _write(tmp_path, dict(hf, use_gated_mlp=False, use_swiglu_ffn=False, hidden_act="gelu"), sd)
    with pytest.raises(RuntimeError, match=r"(use_gated_mlp|use_swiglu_ffn)=false.*has a gate tensor"):
        CK.load_dino_dir(tmp_path)


@pytest.mark.parametrize("name,act", [("dinov3_vithplus16", "gelu"), ("dinov3_vithplus16", "relu"), ("dinov3_plain_keybias", "silu"),
                                      ("dinov2_reg_base", "relu")])
def test_unknown_hidden_act_is_refused(tmp_path, name, act):
    _write(tmp_path, _small(FAMILY[name][1], hidden_act=act), {})
    with pytest.raises(RuntimeError, match=f"hidden_act '{act}'"):
        CK.load_dino_dir(tmp_path)


def test_unknown_model_type_is_refused(tmp_path):
    _write(tmp_path, dict(model_type="dinov3_convnext"), {})
    with pytest.raises(RuntimeError, match="model_type 'dinov3_convnext'"):
        CK.load_dino_dir(tmp_path)


def _swiglu_epilogue_f64(acc, bias, scale=None):
    """float64 model of LMX_ACT_SWIGLU (include/lmx.h) on the [M, 2I] accumulators of the PACKED operand:
    C[m][j] = scale[j] * silu(acc[m][g(j)] + bias[g(j)]) * (acc[m][u(j)] + bias[u(j)]), g(j) = 32 (j // 16) + j % 16, u(j) = g(j) + 16."""
    I = acc.shape[1] // 2
    j = np.arange(I)
    g = 32 * (j // 16) + j % 16
    x = acc.astype(np.float64) + bias.astype(np.float64)
    gv, uv = x[:, g], x[:, g + 16]
    out = gv / (1 + np.exp(-gv)) * uv
    return out * scale if scale is not None else out


@pytest.mark.parametrize("I,K", [(16, 8), (48, 24), (1536, 64)])
def test_packing_reproduces_the_gated_mlp_exactly(I, K):
    """Integer-valued inputs: every product and sum below is exact in float64, so the packed form must EQUAL
    silu(x Wg^T + bg) * (x Wu^T + bu) — any misplaced row or bias changes it."""
    r = np.random.default_rng(I)
    x = r.integers(-4, 5, (7, K)).astype(np.float64)
    wg, wu = r.integers(-3, 4, (I, K)).astype(np.float64), r.integers(-3, 4, (I, K)).astype(np.float64)
    bg, bu = r.integers(-5, 6, I).astype(np.float64), r.integers(-5, 6, I).astype(np.float64)
    w, b = dino.pack_gated(wg, wu), dino.pack_gated(bg, bu)
    assert w.shape == (2 * I, K) and b.shape == (2 * I,)
    assert np.array_equal(w[:16], wg[:16]) and np.array_equal(w[16:32], wu[:16])  # g0..g15, u0..u15, g16..
    got = _swiglu_epilogue_f64(x @ w.T, b)
    g, u = x @ wg.T + bg, x @ wu.T + bu
    assert np.array_equal(got, g / (1 + np.exp(-g)) * u)
    with pytest.raises(ValueError):
        dino.pack_gated(wg[:I - 8], wu[:I - 8])


def test_dinov2_weights_in_first_half_is_the_gate():
    """Dinov2SwiGLUFFN: x1, x2 = weights_in(x).chunk(2); silu(x1) * x2 — the embedder packs weights_in[:I] as gate rows.  Checked
    against transformers' module itself (fp32) through the float64 epilogue model."""
    from transformers import Dinov2Config
    from transformers.models.dinov2.modeling_dinov2 import Dinov2SwiGLUFFN

    torch.manual_seed(0)
    ffn = Dinov2SwiGLUFFN(Dinov2Config(hidden_size=48, mlp_ratio=4, use_swiglu_ffn=True)).eval()
    I = ffn.weights_out.in_features
    assert I == dino.swiglu_hidden(48) == 128
    wi, bi = ffn.weights_in.weight.detach().numpy(), ffn.weights_in.bias.detach().numpy()
    x = torch.randn(5, 48)
    with torch.no_grad():
        ref = ffn(x).numpy()
    h = _swiglu_epilogue_f64(x.numpy().astype(np.float64) @ dino.pack_gated(wi[:I], wi[I:]).astype(np.float64).T, dino.pack_gated(bi[:I], bi[I:]))
    got = h @ ffn.weights_out.weight.detach().numpy().astype(np.float64).T + ffn.weights_out.bias.detach().numpy()
    assert np.abs(got - ref).max() < 1e-5


def test_registers_prefix_and_position_rows():
    """dinov2_with_registers: what the embedder hands lmx_k_assemble_tokens reproduces Dinov2WithRegistersEmbeddings.forward
    (position table on CLS and patches, registers inserted afterwards) — a numpy model of the kernel's `prefix | patches + pos`."""
    cfg = dino.dinov2_reg_base(layers=1, hidden=64, heads=1, mlp=256)
    sd = weights.synth_state_dict(dino.param_spec(cfg), 3)
    pos = dino.interpolate_pos_embed(torch.from_numpy(sd["embeddings.position_embeddings"]), cfg.pos_grid, cfg.grid,
                                     antialias=True)[0].numpy()
    r = np.random.default_rng(0)
    patches = r.standard_normal((cfg.grid ** 2, 64)).astype(np.float32)
    want = np.concatenate([sd["embeddings.cls_token"][0] + pos[:1], sd["embeddings.register_tokens"][0], patches + pos[1:]], 0)
    prefix = np.concatenate([sd["embeddings.cls_token"][0] + pos[:1], sd["embeddings.register_tokens"][0]], 0)
    table = np.concatenate([np.zeros((cfg.n_prefix, 64), np.float32), pos[1:]], 0)
    assert cfg.n_prefix == 5 and cfg.tokens == 261
    assert np.array_equal(np.concatenate([prefix, patches], 0) + table, want)
