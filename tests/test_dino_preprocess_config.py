"""preprocessor_config.json -> lmx.dino.DinoPreprocess (lmx.checkpoints.read_dino_preprocess / load_dino_dir): what is read,
what is refused (with the field's name), and the parameterised PIL recipe against BitImageProcessorPil.  CPU only."""
import dataclasses
import json

import numpy as np
import pytest

import dinopre
from lmx import checkpoints as CK
from lmx import dino, weights
from lmx import resample as R

OTHER_MEAN, OTHER_STD = [0.5, 0.45, 0.4], [0.25, 0.2, 0.3]


def _read(tmp_path, pre, patch=16):
    (tmp_path / "preprocessor_config.json").write_text(json.dumps(pre))
    return CK.read_dino_preprocess(tmp_path, patch)


def test_no_file_is_todays_recipe(tmp_path):
    assert CK.read_dino_preprocess(tmp_path, 16) is None
    assert dino.DinoConfig().preproc is None
    # the recipe an embedder derives for a hand-built configuration is dinov2-base's
    assert dino.DinoPreprocess() == dino.DinoPreprocess(kind="pil", filt=R.BICUBIC, shortest_edge=256, size_hw=None, crop=224,
                                                        rescale=1 / 255, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)


def test_dinov3_file(tmp_path):
    """The class defaults of the installed transformers' DINOv3ViTImageProcessor: bilinear, 224 x 224, ImageNet, 1/255."""
    want = dino.DinoPreprocess(kind="float", filt=R.BILINEAR, shortest_edge=None, size_hw=(224, 224), crop=None, rescale=1 / 255,
                               mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
    assert _read(tmp_path, dinopre.dinov3_preprocessor_config()) == want
    assert want.input_size == 224 and want.resized(1080, 1920) == (224, 224)
    # a file that only names the class gets the class defaults; the Fast alias is the same processor
    assert _read(tmp_path, {"image_processor_type": "DINOv3ViTImageProcessorFast"}) == want
    p = _read(tmp_path, dinopre.dinov3_preprocessor_config(size=256, resample=3))
    assert (p.size_hw, p.filt, p.input_size) == ((256, 256), R.BICUBIC, 256)
    # resize to a larger rectangle, then a centre crop
    p = _read(tmp_path, {**dinopre.dinov3_preprocessor_config(), "size": {"height": 256, "width": 320}, "do_center_crop": True,
                         "crop_size": {"height": 224, "width": 224}})
    assert (p.size_hw, p.crop, p.input_size) == ((256, 320), 224, 224)


def test_dinov2_files(tmp_path):
    p = _read(tmp_path, dinopre.dinov2_preprocessor_config(), patch=14)
    assert p == dino.DinoPreprocess() and p.resized(1080, 1920) == (256, 455)
    p = _read(tmp_path, dinopre.dinov2_preprocessor_config(512, 448, 2, image_mean=OTHER_MEAN, image_std=OTHER_STD), patch=14)
    assert p == dino.DinoPreprocess(kind="pil", filt=R.BILINEAR, shortest_edge=512, crop=448, mean=tuple(OTHER_MEAN), std=tuple(OTHER_STD))
    assert p.input_size == 448 and p.resized(1080, 1920) == (512, 910)
    assert _read(tmp_path, {"image_processor_type": "BitImageProcessorFast", "size": {"shortest_edge": 256}}, patch=14).kind == "pil"


REFUSALS = [
    ("image_processor_type", dict(image_processor_type="ViTImageProcessor")),
    ("image_processor_type", dict(image_processor_type=None)),
    ("resample", dict(resample=1)),
    ("do_resize", dict(do_resize=False)),
    ("do_rescale", dict(do_rescale=False)),
    ("do_normalize", dict(do_normalize=False)),
    ("size", dict(size={"height": 224, "width": 320})),                       # not square, no crop
    ("size", dict(size={"height": 230, "width": 230})),                       # not a multiple of the patch size
    ("size", dict(size={"shortest_edge": 224})),                              # DINOv3 path, no crop: no square input
    ("crop_size", dict(do_center_crop=True, crop_size={"height": 256, "width": 256})),  # larger than the 224 x 224 resize
    ("crop_size", dict(do_center_crop=True, size={"height": 256, "width": 256}, crop_size={"height": 224, "width": 192})),
    ("image_std", dict(image_std=[0.2, 0.0, 0.2])),
    ("image_mean", dict(image_mean=[0.5])),
    ("rescale_factor", dict(rescale_factor=0)),
]


@pytest.mark.parametrize("field,change", REFUSALS, ids=[f"{i}-{f}" for i, (f, _) in enumerate(REFUSALS)])
def test_dinov3_refusals_name_file_and_field(tmp_path, field, change):
    with pytest.raises(RuntimeError, match=rf"preprocessor_config\.json: {field} "):
        _read(tmp_path, {**dinopre.dinov3_preprocessor_config(), **change})


@pytest.mark.parametrize("field,change", [
    ("crop_size", dict(crop_size={"height": 225, "width": 225})),            # not a multiple of 14
    ("crop_size", dict(crop_size={"height": 224, "width": 238})),            # not square
    ("crop_size", dict(size={"shortest_edge": 210}, crop_size={"height": 224, "width": 224})),  # the processor would pad
    ("resample", dict(resample=0)),
    ("do_rescale", dict(do_rescale=False)),
])
def test_dinov2_refusals_name_file_and_field(tmp_path, field, change):
    with pytest.raises(RuntimeError, match=rf"preprocessor_config\.json: {field} "):
        _read(tmp_path, {**dinopre.dinov2_preprocessor_config(), **change}, patch=14)


def test_load_dino_dir_follows_the_file(tmp_path):
    """DinoConfig.image follows the file: DINOv3 at 256 x 256 has 16 x 16 + 5 tokens, dinov2 with crop 448 a 32 x 32 grid; a
    directory without the file loads exactly as before; a refusal surfaces from load_dino_dir."""
    cfg = dino.dinov3_vitsplus16(layers=1)
    sd = weights.synth_state_dict(dino.param_spec(cfg), 5)
    d0, d1, d2, d3 = (tmp_path / n for n in ("plain", "v3_256", "v2_448", "bad"))
    for d in (d0, d1, d2, d3):
        d.mkdir()
    dinopre.write_model_dir(d0, dinopre.dinov3_hf_config(cfg), sd)
    got, _ = CK.load_dino_dir(d0)
    assert got == cfg and got.preproc is None and got.image == 224
    dinopre.write_model_dir(d1, dinopre.dinov3_hf_config(cfg), sd, dinopre.dinov3_preprocessor_config(size=256))
    got, _ = CK.load_dino_dir(d1)
    assert got.preproc.kind == "float" and got.image == 256 and got.tokens == 16 * 16 + 5
    assert dataclasses.replace(got, preproc=None, image=224) == cfg
    c2 = dino.DinoConfig(arch="dinov2", hidden=64, layers=1, heads=1, mlp=256, patch=14, registers=0, eps=1e-6)
    hf2 = {"model_type": "dinov2", "hidden_size": 64, "num_hidden_layers": 1, "num_attention_heads": 1, "mlp_ratio": 4, "patch_size": 14,
           "image_size": 518, "layer_norm_eps": 1e-6}
    dinopre.write_model_dir(d2, hf2, weights.synth_state_dict(dino.param_spec(c2), 6), dinopre.dinov2_preprocessor_config(512, 448))
    got, _ = CK.load_dino_dir(d2)
    assert (got.preproc.kind, got.image, got.resize_edge, got.grid) == ("pil", 448, 512, 32)
    dinopre.write_model_dir(d3, dinopre.dinov3_hf_config(cfg), sd, dinopre.dinov3_preprocessor_config(resample=1))
    with pytest.raises(RuntimeError, match=r"bad.preprocessor_config\.json: resample "):
        CK.load_dino_dir(d3)


def test_parameterised_pil_recipe_equals_bit_image_processor(tmp_path):
    """The host restatement of the device PIL path (lmx.resample tables + norm_lut) with the recipe's numbers — shortest edge
    512, bilinear, crop 448, another mean / std — equals BitImageProcessorPil built with the same numbers, bit for bit."""
    from PIL import Image
    from transformers.models.bit.image_processing_pil_bit import BitImageProcessorPil

    rc = _read(tmp_path, dinopre.dinov2_preprocessor_config(512, 448, 2, image_mean=OTHER_MEAN, image_std=OTHER_STD), patch=14)
    proc = BitImageProcessorPil(size={"shortest_edge": 512}, crop_size={"height": 448, "width": 448}, image_mean=OTHER_MEAN,
                                image_std=OTHER_STD, resample=2)
    rgb = np.random.default_rng(11).integers(0, 256, (540, 960, 3), dtype=np.uint8)
    ref = proc(images=Image.fromarray(rgb), return_tensors="pt")["pixel_values"][0].numpy()
    nh, nw = rc.resized(*rgb.shape[:2])
    assert (nh, nw) == (512, 910)
    img = R.resize_u8_reference(rgb, nw, nh, rc.filt)
    top, left = (nh - rc.crop) // 2, (nw - rc.crop) // 2
    crop = img[top:top + rc.crop, left:left + rc.crop]
    lut = R.norm_lut(rc.mean, rc.std, rc.rescale)
    got = np.stack([lut[c][crop[:, :, c]] for c in range(3)], 0)
    assert got.shape == ref.shape == (3, 448, 448)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
