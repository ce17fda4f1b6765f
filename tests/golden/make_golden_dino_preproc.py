"""Regenerates the golden vectors of the DINOv3 float preprocessing path (tests/test_gpu_dino_preprocess.py).
Run on a CPU box:  python tests/golden/make_golden_dino_preproc.py [name ...]

As tests/golden/make_golden_dino_family.py: transformers' DINOv3ViTModel built from a config object (eager attention, fp32,
CPU), filled with the build's deterministic synthetic weights (lmx.weights, seed in the file name) — but fed by
DINOv3ViTImageProcessor's computation (tests/dinopre.py: rescale -> float32 antialiased bilinear resize of the whole frame
-> normalize) instead of the dinov2-base PIL recipe.  Stored: seeds, frame ids, the configuration (factory name in lmx.dino +
keyword arguments), the processor's size, the token-mean embedding and last_hidden_state on a token subset — no weights.

Each file also records `old_recipe_cos`: the cosine between the golden embedding and the embedding of the SAME weights fed
by the dinov2-base recipe (make_golden.hf_pixel_values: bicubic shortest-edge 256 on u8, centre crop 224) — what the embedder
computed before it read preprocessor_config.json.  It must miss the 1 - 1e-4 bar (asserted here), i.e. the bar can tell the
two recipes apart."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd"), os.path.join(ROOT, "tests"), HERE]

import dinopre  # noqa: E402
from lmx import dino, synth, weights  # noqa: E402
from make_golden import hf_pixel_values  # noqa: E402
from make_golden_dino_family import hf_model, token_subset  # noqa: E402

BAR = 1 - 1e-4

# name -> (factory in lmx.dino, kwargs, processor size, weight seed, clip seed, frame ids).  Real widths and full depth.
CONFIGS = {
    "dinov3_vitl16_pre224_w21": ("dinov3_vitl16", {}, 224, 21, 41, (4, 97)),          # BASELINE's model
    "dinov3_vitsplus16_pre256_w22": ("dinov3_vitsplus16", {}, 256, 22, 42, (11, 130)),
}


def make(name):
    factory, kw, size, seed, clip_seed, frame_ids = CONFIGS[name]
    cfg = getattr(dino, factory)(**kw)
    cfg.image = size
    sd = weights.synth_state_dict(dino.param_spec(cfg), seed)
    frames = np.stack([synth.synth_frame(clip_seed, i) for i in frame_ids], 0)  # BGR, 1080p
    pv = dinopre.dinov3_pixel_values(np.ascontiguousarray(frames[..., ::-1]), size_hw=(size, size))
    assert tuple(pv.shape) == (len(frame_ids), 3, size, size)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        m = hf_model(cfg)
        m.load_state_dict(tsd, strict=True)
        hs = m(pixel_values=pv).last_hidden_state
        emb = hs.mean(dim=1)  # services/dinov3-pipeline/app/main.py:113
        old = m(pixel_values=hf_pixel_values(frames)).last_hidden_state.mean(dim=1)
    assert tuple(hs.shape) == (len(frame_ids), cfg.tokens, cfg.hidden), hs.shape
    cos = torch.nn.functional.cosine_similarity(emb.double(), old.double(), dim=1)
    print(name, "dinov2-base recipe on the same weights: cos", cos.tolist())
    assert float(cos.max()) < BAR, f"{name}: the bar does not tell the recipes apart, pick another seed ({cos.tolist()})"
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, embedding=emb.numpy(), token_ids=token_subset(cfg), hidden_tokens=hs[:, token_subset(cfg)].numpy(),
                        factory=factory, kwargs=json.dumps(kw), size=size, weight_seed=seed, clip_seed=clip_seed,
                        frame_ids=np.asarray(frame_ids), old_recipe_cos=cos.numpy(),
                        pixel_checksum=np.asarray([int(pv.double().abs().sum() * 1000)]))
    print(name, "tokens", cfg.tokens, "embedding norm", emb.norm(dim=1).tolist(), "->", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for n in sys.argv[1:] or CONFIGS:
        make(n)
