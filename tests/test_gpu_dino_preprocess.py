"""The preprocessing recipe of the model directory on the GPU: lmx_k_float_resize_patchify (DINOv3ViTImageProcessor's rescale ->
float32 antialiased resize -> normalize) against its torch CPU restatement (tests/dinopre.py), the unchanged PIL path, and a
DINOv3 directory with a preprocessor_config.json end to end against transformers' fp32 outputs
(tests/golden/make_golden_dino_preproc.py) through the adapters and the DINOv3 service mirror."""
import asyncio
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import dinopre

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1 - 1e-4
GEOMETRIES = [(1080, 1920), (1920, 1080), (720, 1280), (333, 517), (150, 200)]


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


def _f16_order(t):
    """f16 -> integers whose difference counts representable values between two numbers (sign-magnitude made monotone)."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("out", [224, 448])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_float_kernel_matches_torch(cuda, geo, out, filt):
    """The f16 patch matrix against the torch CPU restatement rounded to f16: every element within one f16 ulp and at least 99 %
    bit-equal, for RGB and BGR input and n = 1 and n = 5 (frame 0 alone is frame 0 of the batch).  Bilinear runs with patch 16,
    bicubic with patch 14 and the row stride padded to 592: the 4 columns beyond 14*14*3 stay zero."""
    from lmx import kernels as K
    from lmx import resample as R

    h, w = geo
    P, k_pad = (16, None) if filt == "bilinear" else (14, 592)
    g = out // P
    rng = np.random.default_rng(h + 3 * out + len(filt))
    rgb = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ref = dinopre.patch_matrix(dinopre.dinov3_pixel_values(rgb, (out, out), 2 if filt == "bilinear" else 3, 1 / 255, mean, std), P)
    ref16 = ref.to(torch.float16)

    def up(tab):
        return torch.from_numpy(tab[0]).to(cuda), torch.from_numpy(tab[1]).to(cuda), tab[2]

    th, tv = R.aa_tables(w, out, filt), R.aa_tables(h, out, filt)
    seg = R.segment_cols(th[0])
    th, tv = up(th), up(tv)
    np_ = g * g
    for n, swap in ((5, False), (1, False), (5, True), (1, True)):
        src = rgb[:n, :, :, ::-1] if swap else rgb[:n]
        d_src = torch.from_numpy(np.ascontiguousarray(src)).to(cuda)
        got = K.float_resize_patchify(d_src, g, g, P, th, tv, seg, 1 / 255, mean, std, swap_rb=swap, k_pad=k_pad).cpu()
        assert got.dtype == torch.float16 and tuple(got.shape) == (n * np_, k_pad or P * P * 3)
        if k_pad:
            assert not got[:, P * P * 3:].any(), "padding columns were written"
            got = got[:, :P * P * 3]
        want = ref16[:n * np_]
        ulps = (_f16_order(got) - _f16_order(want)).abs()
        equal = float((ulps == 0).float().mean())
        print(geo, out, filt, "n", n, "bgr" if swap else "rgb", "max f16 ulps", int(ulps.max()), "bit-equal", equal,
              "max abs vs f32 reference", float((got.float() - ref[:n * np_]).abs().max()))
        assert int(ulps.max()) <= 1, int(ulps.max())
        assert equal >= 0.99, equal


def test_float_kernel_centre_crop_and_refusals(cuda):
    """A centre crop is a slice of the tables: resize to 256 x 320, crop 224.  Malformed calls are refused by the launcher."""
    from lmx import dino, weights
    from lmx import kernels as K

    rc = dino.DinoPreprocess(kind="float", filt="bilinear", shortest_edge=None, size_hw=(256, 320), crop=224)
    cfg = dino.DinoConfig(hidden=256, layers=1, heads=4, mlp=1024, preproc=rc)
    m = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 2), cuda)
    rgb = np.random.default_rng(8).integers(0, 256, (2, 540, 960, 3), dtype=np.uint8)
    got = m.preprocess(torch.from_numpy(rgb).to(cuda), rgb=True).cpu()
    ref = dinopre.patch_matrix(dinopre.dinov3_pixel_values(rgb, (256, 320), crop=224), 16).to(torch.float16)
    ulps = (_f16_order(got) - _f16_order(ref)).abs()
    assert int(ulps.max()) <= 1 and float((ulps == 0).float().mean()) >= 0.99
    with pytest.raises(K.LmxError, match="smaller than the 224 crop"):
        dino.DinoEmbedder(dataclasses.replace(cfg, preproc=dataclasses.replace(rc, size_hw=(192, 320))),
                          weights.synth_state_dict(dino.param_spec(cfg), 2), cuda).preprocess(torch.from_numpy(rgb).to(cuda))
    with pytest.raises(K.LmxError, match="feeds 224 x 224"):
        dino.DinoEmbedder(dataclasses.replace(cfg, image=256), weights.synth_state_dict(dino.param_spec(cfg), 2), cuda)
    th, tv, seg = m._tables(540, 960)
    d = torch.from_numpy(rgb).to(cuda)
    with pytest.raises(K.LmxError, match="tables do not describe"):
        K.float_resize_patchify(d, 16, 14, 16, th, tv, seg, 1 / 255, rc.mean, rc.std)
    with pytest.raises(K.LmxError, match="seg_cols"):
        K.float_resize_patchify(d, 14, 14, 16, th, tv, 961, 1 / 255, rc.mean, rc.std)
    with pytest.raises(K.LmxError, match="uint8"):
        K.float_resize_patchify(d.float(), 14, 14, 16, th, tv, seg, 1 / 255, rc.mean, rc.std)


def test_old_path_is_untouched(cuda):
    """An embedder built from a configuration without a recipe (bench.py, the fused extractor) gives the bits of the
    parameterised PIL path handed the dinov2-base numbers explicitly, BGR and RGB."""
    from lmx import dino, synth, weights
    from lmx import resample as R

    cfg = dino.DinoConfig(hidden=256, layers=1, heads=4, mlp=1024)
    assert cfg.preproc is None
    sd = weights.synth_state_dict(dino.param_spec(cfg), 9)
    explicit = dino.DinoPreprocess(kind="pil", filt=R.BICUBIC, shortest_edge=256, size_hw=None, crop=224, rescale=1 / 255,
                                   mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    a, b = dino.DinoEmbedder(cfg, sd, cuda), dino.DinoEmbedder(dataclasses.replace(cfg, preproc=explicit), sd, cuda)
    assert a.recipe == explicit
    frames = torch.from_numpy(np.stack([synth.synth_frame(2, i) for i in (0, 7)], 0)).to(cuda)
    for rgb in (False, True):
        assert torch.equal(a.preprocess(frames, rgb=rgb), b.preprocess(frames, rgb=rgb))
    assert torch.equal(a.embed_frames(frames), b.embed_frames(frames))


def _golden(name):
    from lmx import dino, synth, weights

    g = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = getattr(dino, str(g["factory"]))(**json.loads(str(g["kwargs"])))
    sd = weights.synth_state_dict(dino.param_spec(cfg), int(g["weight_seed"]))
    frames = np.stack([synth.synth_frame(int(g["clip_seed"]), int(i)) for i in g["frame_ids"]], 0)
    return g, cfg, sd, frames


@pytest.mark.parametrize("name", ["dinov3_vitl16_pre224_w21", "dinov3_vitsplus16_pre256_w22"])
def test_model_dir_with_preprocessor_config_matches_transformers(cuda, tmp_path, name):
    """A dinov3_vit directory (config.json, model.safetensors, preprocessor_config.json) loaded through
    LmxDinoModel.from_pretrained + LmxImageProcessor, fed raw 1080p frames, against transformers fed by DINOv3ViTImageProcessor's
    computation: embedding cosine >= 1 - 1e-4, per token max abs error < 3e-2 and cosine > 1 - 1e-4 on the stored subset
    (the bars of tests/test_gpu_dino_family.py).  The golden's `old_recipe_cos` (the same weights fed by the dinov2-base recipe,
    transformers fp32) misses the bar, and so does this build's embedder without the recipe: the pass is not blind to it."""
    from lmx import adapters, dino

    g, cfg, sd, frames = _golden(name)
    size = int(g["size"])
    dinopre.write_model_dir(tmp_path, dinopre.dinov3_hf_config(cfg), sd, dinopre.dinov3_preprocessor_config(size=size))
    model = adapters.LmxDinoModel.from_pretrained(str(tmp_path), device=cuda)
    assert model.config.preproc.kind == "float" and model.config.image == size and model.config.tokens == (size // 16) ** 2 + 5
    proc = adapters.LmxImageProcessor.from_pretrained(model)
    rgb = [np.ascontiguousarray(f[:, :, ::-1]) for f in frames]
    hs = torch.cat([model(**proc(images=im, return_tensors="pt").to(cuda)).last_hidden_state for im in rgb], 0).cpu()
    emb = hs.mean(dim=1)  # dinov3 main.py:113
    ref = torch.from_numpy(g["embedding"])
    cos = _cos(emb, ref)
    print(name, "embedding cos", cos.tolist(), "1 - cos", (1 - cos).tolist(), "max abs", float((emb - ref).abs().max()))
    sub, href = hs[:, torch.from_numpy(g["token_ids"]).long()], torch.from_numpy(g["hidden_tokens"])
    err, tcos = float((sub - href).abs().max()), float(_cos(sub, href).min())
    print(name, "per-token max abs err", err, "min cos", tcos)
    assert float(cos.min()) >= BAR, cos.tolist()
    assert err < 3e-2, err
    assert tcos > BAR, tcos
    # the list form of the processor call and the embedder's own entry point give the same embedding
    both = model(**proc(images=rgb, return_tensors="pt")).last_hidden_state.mean(dim=1).cpu()
    assert float(_cos(both, ref).min()) >= BAR
    direct = model.embedder.embed_frames(torch.from_numpy(frames).to(cuda)).cpu()
    assert float(_cos(direct, ref).min()) >= BAR
    # negative control: the same weights without the recipe
    assert float(g["old_recipe_cos"].max()) < BAR, g["old_recipe_cos"]
    old = dino.DinoEmbedder(dataclasses.replace(model.config, preproc=None, image=224), sd, cuda)
    ocos = _cos(old.embed_frames(torch.from_numpy(frames).to(cuda)).cpu(), ref)
    print(name, "dinov2-base recipe on the same weights: cos", ocos.tolist(), "(transformers, fp32:", g["old_recipe_cos"].tolist(), ")")
    assert float(ocos.max()) < BAR


def test_dinov3_service_picks_up_the_recipe(cuda, tmp_path):
    """The DINOv3Pipeline mirror over a short clip, its embedder loaded from a directory with a preprocessor_config.json
    (256 x 256): the JSON file holds embed_frames of the sampled frames, and they are not what the old recipe gives."""
    from lmx import checkpoints, dino, services, synth, weights
    from lmx.services import runtime as R

    cfg = dino.dinov3_vitsplus16(layers=2)
    sd = weights.synth_state_dict(dino.param_spec(cfg), 5)
    mdir = tmp_path / "model"
    mdir.mkdir()
    dinopre.write_model_dir(mdir, dinopre.dinov3_hf_config(cfg), sd, dinopre.dinov3_preprocessor_config(size=256))
    lcfg, lsd = checkpoints.load_dino_dir(mdir)
    emb = dino.DinoEmbedder(lcfg, lsd, cuda)
    assert emb.recipe.kind == "float" and lcfg.image == 256
    frames = np.stack([synth.synth_frame(3, 40 + 3 * i) for i in range(9)], 0)
    clip = tmp_path / "clip.npz"
    R.save_npz_clip(clip, frames, 8.0)  # DINO samples frames 0 and 8
    bus = R.InProcessBus()
    conf = {"nats": {"subjects": dict(R.DEFAULT_SUBJECTS)}}
    svc = services.DINOv3Pipeline(emb, bus, None, conf, results_dir=tmp_path / "dino")
    asyncio.run(svc.process_video({"video_id": "clip1", "processed_path": str(clip), "filename": "clip1.mp4"}))
    out = json.load(open(tmp_path / "dino" / "clip1_dinov3.json"))
    want = emb.embed_frames(torch.from_numpy(frames[[0, 8]]).to(cuda)).cpu().numpy()
    assert [c["frame"] for c in out["canonical_frames"]] == [0, 8, 8]
    assert out["canonical_frames"][0]["embedding"] == want[0].tolist() and out["canonical_frames"][2]["embedding"] == want[1].tolist()
    pv = dinopre.patch_matrix(dinopre.dinov3_pixel_values(np.ascontiguousarray(frames[[0, 8]][..., ::-1]), (256, 256)), 16)
    assert float((emb.preprocess(torch.from_numpy(frames[[0, 8]]).to(cuda)).cpu().float() - pv).abs().max()) < 2e-3
    old = dino.DinoEmbedder(cfg, sd, cuda).embed_frames(torch.from_numpy(frames[[0, 8]]).to(cuda)).cpu()
    assert float(_cos(old, torch.from_numpy(want)).max()) < BAR
