"""Pins tests/samprompt.py (points, mask input, all four masks) to transformers' SamModel, built as
tests/test_oracle_sam_decoder.py builds it and held to that test's tolerances, and shows that models of four defects miss
those tolerances by at least 10x.  The mask-embedding bound of the GPU test is checked here against a float32 run."""
import numpy as np
import pytest
import torch

import samprompt as SP
from lmx import sam_decoder, weights

transformers = pytest.importorskip("transformers")

HW, RHW = (1080, 1920), (576, 1024)


def _state(seed=41):
    sd = sam_decoder.synthetic_state_dict(seed)
    sd.update(weights.synth_state_dict(sam_decoder.mask_embed_param_spec(), seed + 1))
    return sd


def _hf(sd):
    from transformers import SamConfig, SamModel

    c = SamConfig()
    c.vision_config.num_hidden_layers = 1
    c.vision_config.hidden_size = 64
    c.vision_config.num_attention_heads = 2
    c.vision_config.mlp_dim = 128
    c.vision_config.global_attn_indexes = [0]
    c.mask_decoder_config._attn_implementation = "eager"
    m = SamModel(c).eval()
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("vision_encoder.") for k in missing), (missing, unexpected)
    return m


def _emb(seed, n=1):
    rng = np.random.default_rng(seed)
    base = torch.from_numpy(rng.standard_normal((n, 256, 8, 8)).astype(np.float32))
    emb = torch.nn.functional.interpolate(base, size=(64, 64), mode="bilinear", align_corners=False) * 2.0
    return emb + 0.1 * torch.from_numpy(rng.standard_normal(emb.shape).astype(np.float32))


def _mask_input(seed):
    rng = np.random.default_rng(seed)
    m = torch.nn.functional.interpolate(torch.from_numpy(rng.standard_normal((1, 1, 16, 16)).astype(np.float32)) * 8, size=(256, 256),
                                        mode="bilinear", align_corners=False)
    return m[:, 0]


# (name, points [Np,2] frame pixels, labels, box, mask_input seed, multimask)
CASES = [
    ("one positive point", [[700.0, 400.0]], [1], None, None, False),
    ("pos + neg + ignored", [[700.0, 400.0], [1200.0, 650.0], [30.0, 900.0]], [1, 0, -1], None, None, True),
    ("2 points + box", [[600.0, 300.0], [900.0, 600.0]], [1, 0], [300.0, 150.0, 1200.0, 900.0], None, False),
    ("box only, multimask", None, None, [300.0, 150.0, 1200.0, 900.0], None, True),
    ("points + mask_input", [[700.0, 400.0], [1300.0, 800.0]], [1, 1], None, 7, True),
    ("14 points, no box (T=20)", [[100.0 + 120 * i, 80.0 + 60 * i] for i in range(14)], [1, 0, -1, 1, 1, 0, 0, 1, -1, 1, 0, 1, 1, 0], None,
     None, True),
]


def _hf_run(m, emb, pts, lab, box, mk, multimask):
    ip = None if pts is None else torch.from_numpy(SP.scale_coords(np.asarray(pts)[None, None], HW, RHW))
    il = None if lab is None else torch.tensor(lab)[None, None]
    ib = None if box is None else torch.from_numpy(SP.scale_coords(np.asarray(box, np.float64).reshape(1, 2, 2), HW, RHW).reshape(1, 1, 4))
    im = None if mk is None else mk[:, None]
    with torch.no_grad():
        sparse, dense = m.prompt_encoder(input_points=ip, input_labels=il, input_boxes=ib, input_masks=im)
        pe = m.get_image_wide_positional_embeddings()
        masks, iou = m.mask_decoder(image_embeddings=emb, image_positional_embeddings=pe, sparse_prompt_embeddings=sparse,
                                    dense_prompt_embeddings=dense, multimask_output=multimask)
    return sparse[:, 0], dense, masks[:, 0], iou[:, 0]


def _miss(a, b, atol, rtol=0.0):
    """max |a - b| / (atol + rtol |b|): <= 1 within the tolerance."""
    return float(((a.double() - b.double()).abs() / (atol + rtol * b.double().abs())).max())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_matches_transformers(case):
    name, pts, lab, box, mseed, multimask = case
    sd = _state()
    m = _hf(sd)
    emb = _emb(5)
    mk = None if mseed is None else _mask_input(mseed)
    sparse_ref, dense_ref, low_ref, iou_ref = _hf_run(m, emb, pts, lab, box, mk, multimask)
    sd32 = SP.sd_as(sd, torch.float32)
    with torch.no_grad():
        low, iou, sparse, dense = SP.predict(sd32, emb, HW, RHW, None if pts is None else [pts], None if lab is None else [lab],
                                             None if box is None else [box], mk, multimask)
    assert sparse.shape == sparse_ref.shape and low.shape == low_ref.shape and iou.shape == iou_ref.shape
    assert _miss(sparse, sparse_ref, 1e-5) <= 1
    if mk is not None:
        assert _miss(dense, dense_ref, 1e-5) <= 1
    assert _miss(low, low_ref, 2e-4, 1e-4) <= 1, _miss(low, low_ref, 2e-4, 1e-4)
    assert _miss(iou, iou_ref, 1e-4) <= 1


def test_defect_models_miss_by_10x():
    sd = _state()
    m = _hf(sd)
    emb = _emb(5)
    sd32 = SP.sd_as(sd, torch.float32)
    pts, lab = CASES[1][1], CASES[1][2]
    sp_ref, _, _, _ = _hf_run(m, emb, pts, lab, None, None, True)
    sp_bad = SP.encode_prompts(sd32, SP.scale_coords([pts], HW, RHW), [lab], None, defect="neg1_zero")
    r = _miss(sp_bad, sp_ref, 1e-5)
    print("-1 as a zero token: miss", r)
    assert r >= 10
    mk = _mask_input(7)
    _, dense_ref, _, _ = _hf_run(m, emb, CASES[4][1], CASES[4][2], None, mk, True)
    for defect in ("no_ln1", "no_ln2", "tanh_gelu"):
        with torch.no_grad():
            r = _miss(SP.mask_embed(sd32, mk, defect=defect), dense_ref, 1e-5)
        print(defect, "dense: miss", r)
        assert r >= 10, defect
    box = CASES[3][3]
    _, _, low_ref, iou_ref = _hf_run(m, emb, None, None, box, None, True)
    with torch.no_grad():
        low, iou, _, _ = SP.predict(sd32, emb, HW, RHW, box=[box], multimask=True, defect="slice012")
    r = min(_miss(low, low_ref, 2e-4, 1e-4), _miss(iou, iou_ref, 1e-4))
    print("multimask slice 0..2: miss", r)
    assert r >= 10


@pytest.mark.parametrize("kind", ["random", "pm20", "constant"])
def test_mask_embed_bound_holds_for_float32(kind):
    """The per-element bound of tests/test_gpu_sam_prompts.py covers a float32 evaluation (torch's order, not the kernel's) with
    room to spare, and a LayerNorm skipped misses it by far."""
    sd = _state()
    mk = {"random": _mask_input(3), "pm20": torch.where(_mask_input(4) > 0, 20.0, -20.0), "constant": torch.full((1, 256, 256), 0.75)}[kind]
    emb = _emb(6).permute(0, 2, 3, 1).reshape(4096, 256)
    sd64, sd32 = SP.sd_as(sd, torch.float64), SP.sd_as(sd, torch.float32)
    ref, bound = SP.mask_embed_bound(sd64, mk.double(), emb)
    got = emb + SP.mask_embed(sd32, mk).permute(0, 2, 3, 1).reshape(4096, 256)
    r = float(((got.double() - ref).abs() / bound).max())
    print(kind, "float32 torch: max ratio", r)
    assert r <= 0.5
    for defect in ("no_ln1", "no_ln2"):
        bad = emb.double() + SP.mask_embed(sd64, mk.double(), defect=defect).permute(0, 2, 3, 1).reshape(4096, 256)
        assert float(((bad - ref).abs() / bound).max()) >= 30, defect
