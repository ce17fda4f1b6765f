"""Model selection and real-checkpoint key maps — the load paths of the three services:

  * services/yolo-pipeline/app/main.py:24-37     first `*.pt` in /app/shared/models/yolo, else the stock yolov8n
  * services/sam3-pipeline/app/main.py:51-72     first `*.pth` in /app/shared/models/sam3; `vit_h` / `vit_l` in the FILE
                                                 NAME pick the architecture, anything else is vit_b; no file -> None
                                                 (the service then segments with the bbox rectangle)
  * services/dinov3-pipeline/app/main.py:30-36   models.dinov3.model_name, default "facebook/dinov2-base"

Checkpoints are read with loaders that execute nothing from the file (lmx.weights.load_state_dict_file: safetensors or
torch.load(weights_only=True)).  segment_anything's `.pth` files are plain tensor dicts and load as they are; their
parameter names (image_encoder.* / prompt_encoder.* / mask_decoder.*) are mapped onto the names lmx uses (transformers'
SamModel names, which is what the oracle is pinned to).  An Ultralytics `.pt` pickles the model OBJECT: it cannot be read
without the ultralytics package, so the detector takes a state dict exported from it (`model.N.*` names, as
`YOLO(p).model.state_dict()` gives) — see INTEGRATION.md."""
import dataclasses
import json
import re
from pathlib import Path

import numpy as np

from . import weights

# ---- SAM v1: segment_anything <-> lmx (transformers SamModel) names ---------------------------------------------------------
_SA_TO_LMX = [
    (r"^image_encoder\.", "vision_encoder."),
    (r"^vision_encoder\.blocks\.", "vision_encoder.layers."),
    (r"^(vision_encoder\.layers\.\d+)\.norm([12])\.", r"\1.layer_norm\2."),
    (r"^vision_encoder\.patch_embed\.proj\.", "vision_encoder.patch_embed.projection."),
    (r"^vision_encoder\.neck\.0\.", "vision_encoder.neck.conv1."),
    (r"^vision_encoder\.neck\.1\.", "vision_encoder.neck.layer_norm1."),
    (r"^vision_encoder\.neck\.2\.", "vision_encoder.neck.conv2."),
    (r"^vision_encoder\.neck\.3\.", "vision_encoder.neck.layer_norm2."),
    (r"^prompt_encoder\.point_embeddings\.", "prompt_encoder.point_embed."),
    (r"^prompt_encoder\.mask_downscaling\.0\.", "prompt_encoder.mask_embed.conv1."),
    (r"^prompt_encoder\.mask_downscaling\.1\.", "prompt_encoder.mask_embed.layer_norm1."),
    (r"^prompt_encoder\.mask_downscaling\.3\.", "prompt_encoder.mask_embed.conv2."),
    (r"^prompt_encoder\.mask_downscaling\.4\.", "prompt_encoder.mask_embed.layer_norm2."),
    (r"^prompt_encoder\.mask_downscaling\.6\.", "prompt_encoder.mask_embed.conv3."),
    (r"^(mask_decoder\.transformer\.layers\.\d+)\.norm([1-4])\.", r"\1.layer_norm\2."),
    (r"^mask_decoder\.transformer\.norm_final_attn\.", "mask_decoder.transformer.layer_norm_final_attn."),
    (r"^mask_decoder\.output_upscaling\.0\.", "mask_decoder.upscale_conv1."),
    (r"^mask_decoder\.output_upscaling\.1\.", "mask_decoder.upscale_layer_norm."),
    (r"^mask_decoder\.output_upscaling\.3\.", "mask_decoder.upscale_conv2."),
    (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.0\.", r"\1.proj_in."),
    (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.2\.", r"\1.proj_out."),
    (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.1\.", r"\1.layers.0."),
]
_PE_SA = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"
_PE_LMX = ("shared_image_embedding.positional_embedding", "prompt_encoder.shared_embedding.positional_embedding")


def segment_anything_to_lmx(sd):
    """{segment_anything parameter name: array} -> {lmx (transformers SamModel) name: array}.  The single random-Fourier
    matrix of segment_anything's pe_layer is stored under both tied transformers names."""
    out = {}
    for k, v in sd.items():
        if k == _PE_SA:
            for name in _PE_LMX:
                out[name] = v
            continue
        name = k
        for pat, rep in _SA_TO_LMX:
            name = re.sub(pat, rep, name)
        out[name] = v
    return out


def lmx_to_segment_anything(sd):
    """Inverse of segment_anything_to_lmx (used to write checkpoints in the reference's naming, e.g. by the tests)."""
    inv = [
        (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.0\.", r"\1.layers.1."),
        (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.proj_in\.", r"\1.layers.0."),
        (r"^(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.proj_out\.", r"\1.layers.2."),
        (r"^mask_decoder\.upscale_conv1\.", "mask_decoder.output_upscaling.0."),
        (r"^mask_decoder\.upscale_layer_norm\.", "mask_decoder.output_upscaling.1."),
        (r"^mask_decoder\.upscale_conv2\.", "mask_decoder.output_upscaling.3."),
        (r"^mask_decoder\.transformer\.layer_norm_final_attn\.", "mask_decoder.transformer.norm_final_attn."),
        (r"^(mask_decoder\.transformer\.layers\.\d+)\.layer_norm([1-4])\.", r"\1.norm\2."),
        (r"^prompt_encoder\.mask_embed\.conv1\.", "prompt_encoder.mask_downscaling.0."),
        (r"^prompt_encoder\.mask_embed\.layer_norm1\.", "prompt_encoder.mask_downscaling.1."),
        (r"^prompt_encoder\.mask_embed\.conv2\.", "prompt_encoder.mask_downscaling.3."),
        (r"^prompt_encoder\.mask_embed\.layer_norm2\.", "prompt_encoder.mask_downscaling.4."),
        (r"^prompt_encoder\.mask_embed\.conv3\.", "prompt_encoder.mask_downscaling.6."),
        (r"^prompt_encoder\.point_embed\.", "prompt_encoder.point_embeddings."),
        (r"^vision_encoder\.neck\.conv1\.", "vision_encoder.neck.0."),
        (r"^vision_encoder\.neck\.layer_norm1\.", "vision_encoder.neck.1."),
        (r"^vision_encoder\.neck\.conv2\.", "vision_encoder.neck.2."),
        (r"^vision_encoder\.neck\.layer_norm2\.", "vision_encoder.neck.3."),
        (r"^vision_encoder\.patch_embed\.projection\.", "vision_encoder.patch_embed.proj."),
        (r"^(vision_encoder\.layers\.\d+)\.layer_norm([12])\.", r"\1.norm\2."),
        (r"^vision_encoder\.layers\.", "vision_encoder.blocks."),
        (r"^vision_encoder\.", "image_encoder."),
    ]
    out = {}
    for k, v in sd.items():
        if k == _PE_LMX[0]:
            out[_PE_SA] = v
            continue
        if k == _PE_LMX[1]:
            continue
        name = k
        for pat, rep in inv:
            name = re.sub(pat, rep, name)
        out[name] = v
    return out


def sam_model_type(filename):
    """sam3 main.py:57-63: "vit_h" in the name -> vit_h, else "vit_l" -> vit_l, else vit_b."""
    name = Path(filename).name
    if "vit_h" in name:
        return "vit_h"
    if "vit_l" in name:
        return "vit_l"
    return "vit_b"


def find_sam_checkpoint(models_dir="/app/shared/models/sam3"):
    """-> (path, model type) of the checkpoint the service would load, or (None, None) (sam3 main.py:54-56,68-69)."""
    d = Path(models_dir)
    if d.exists():
        files = list(d.glob("*.pth"))
        if files:
            return files[0], sam_model_type(files[0])
    return None, None


def sam_vit_config_from_state_dict(sd):
    """Architecture of a (mapped) SAM v1 state dict, read off the tensor shapes."""
    from . import sam

    D = int(sd["vision_encoder.pos_embed"].shape[-1])
    grid = int(sd["vision_encoder.pos_embed"].shape[1])
    patch = int(sd["vision_encoder.patch_embed.projection.weight"].shape[-1])
    layers = 1 + max(int(m.group(1)) for m in (re.match(r"vision_encoder\.layers\.(\d+)\.", k) for k in sd) if m)
    hd = int(sd["vision_encoder.layers.0.attn.rel_pos_h"].shape[1])
    glob = tuple(i for i in range(layers) if int(sd[f"vision_encoder.layers.{i}.attn.rel_pos_h"].shape[0]) == 2 * grid - 1)
    win = [(int(sd[f"vision_encoder.layers.{i}.attn.rel_pos_h"].shape[0]) + 1) // 2 for i in range(layers) if i not in glob]
    return sam.SamVitConfig(hidden=D, layers=layers, heads=D // hd, mlp=int(sd["vision_encoder.layers.0.mlp.lin1.weight"].shape[0]),
                            global_idx=glob, window=win[0] if win else 14, patch=patch, image=grid * patch,
                            out_ch=int(sd["vision_encoder.neck.conv1.weight"].shape[0]))


def load_sam_checkpoint(path, model_type=None):
    """segment_anything `.pth` (or a safetensors file of the same names) -> (SamVitConfig, lmx-named state dict).
    `model_type` (vit_b / vit_l / vit_h), when given, must agree with the tensors — as `sam_model_registry[type](checkpoint=)`
    fails on a mismatch (load_state_dict is strict)."""
    from . import sam

    raw = weights.load_state_dict_file(path)
    sd = segment_anything_to_lmx(raw) if any(k.startswith("image_encoder.") for k in raw) else raw
    cfg = sam_vit_config_from_state_dict(sd)
    if model_type is not None:
        want = {"vit_b": sam.sam_vit_b(), "vit_l": sam.sam_vit_l(), "vit_h": sam.sam_vit_h(), "default": sam.sam_vit_h()}[model_type]
        if (cfg.hidden, cfg.layers, cfg.heads, tuple(cfg.global_idx)) != (want.hidden, want.layers, want.heads, tuple(want.global_idx)):
            raise RuntimeError(f"checkpoint {path} is not a {model_type} model (hidden {cfg.hidden}, {cfg.layers} layers, "
                               f"{cfg.heads} heads, global blocks {cfg.global_idx})")
    missing = [k for k in sam.vit_param_spec(cfg) if k not in sd]
    if missing:
        raise RuntimeError(f"checkpoint {path}: {len(missing)} image-encoder tensors missing, e.g. {missing[:3]}")
    return cfg, sd


# ---- YOLOv8 ------------------------------------------------------------------------------------------------------------------
def find_yolo_weights(models_dir="/app/shared/models/yolo", patterns=("*.pt", "*.safetensors")):
    """First weight file in the service's model directory (yolo main.py:25-29), or None (-> the stock yolov8n)."""
    d = Path(models_dir)
    if d.exists():
        for pat in patterns:
            files = list(d.glob(pat))
            if files:
                return files[0]
    return None


def yolo_config_from_state_dict(sd):
    """(scale, nc, kpt_shape) of an Ultralytics YOLOv8 detection / pose state dict (`model.N.*` names), from the shapes."""
    from . import yolo

    c0 = int(sd["model.0.conv.weight"].shape[0])
    nb = 1 + max(int(m.group(1)) for m in (re.match(r"model\.2\.m\.(\d+)\.", k) for k in sd) if m)
    c9 = int(sd["model.9.cv2.conv.weight"].shape[0])
    scale = None
    for s in yolo.SCALES:
        cfg = yolo.YoloConfig(s)
        if (cfg.ch(64), cfg.depth(3), cfg.ch(1024)) == (c0, nb, c9):
            scale = s
    if scale is None:
        raise RuntimeError(f"not a YOLOv8 n/s/m/l/x state dict (stem width {c0}, {nb} bottlenecks in model.2, SPPF width {c9})")
    nc = int(sd["model.22.cv3.0.2.weight"].shape[0])
    kpt = None
    if "model.22.cv4.0.2.weight" in sd:
        nk = int(sd["model.22.cv4.0.2.weight"].shape[0])
        kpt = (nk // 3, 3) if nk % 3 == 0 else (nk // 2, 2)
    return scale, nc, kpt


def load_yolo_weights(path):
    """-> (YoloConfig, state dict) from a safetensors / weights_only file holding `model.N.*` tensors (optionally prefixed
    `model.model.N.*`, as `YOLO(p).model.state_dict()` may be saved)."""
    from . import yolo

    try:
        sd = weights.load_state_dict_file(path)
    except Exception as e:  # noqa: BLE001 — typically the pickled DetectionModel of a stock Ultralytics .pt
        raise RuntimeError(f"{path}: cannot be read without executing code from the file ({type(e).__name__}). An Ultralytics "
                           ".pt pickles the model object; export `YOLO(path).model.state_dict()` to safetensors "
                           "(INTEGRATION.md) and put that file in the models directory.") from e
    if any(k.startswith("model.model.") for k in sd):
        sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.model.")}
    sd = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    scale, nc, kpt = yolo_config_from_state_dict(sd)
    cfg = yolo.YoloConfig(scale, nc=nc, kpt_shape=kpt)
    missing = [k for k in yolo.param_spec(cfg) if k not in sd]
    if missing:
        raise RuntimeError(f"{path}: {len(missing)} tensors missing for yolov8{scale}, e.g. {missing[:3]}")
    return cfg, sd


# ---- DINOv2 / DINOv3 ---------------------------------------------------------------------------------------------------------
PREPROCESSOR_FILE = "preprocessor_config.json"
_PROCESSOR_KINDS = {"BitImageProcessor": "pil", "BitImageProcessorFast": "pil",
                    "DINOv3ViTImageProcessor": "float", "DINOv3ViTImageProcessorFast": "float"}
# class defaults of the two processors for the keys a file leaves out (transformers BitImageProcessor / DINOv3ViTImageProcessor)
_PROCESSOR_DEFAULTS = {
    "pil": dict(do_resize=True, size={"shortest_edge": 224}, resample=3, do_center_crop=True, crop_size={"height": 224, "width": 224},
                do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=[0.48145466, 0.4578275, 0.40821073],
                image_std=[0.26862954, 0.26130258, 0.27577711]),
    "float": dict(do_resize=True, size={"height": 224, "width": 224}, resample=2, do_center_crop=False, crop_size=None,
                  do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=[0.485, 0.456, 0.406],
                  image_std=[0.229, 0.224, 0.225]),
}


def read_dino_preprocess(model_dir, patch):
    """`<dir>/preprocessor_config.json` -> lmx.dino.DinoPreprocess, or None when the directory has no such file (the embedder
    then runs the dinov2-base recipe).  `AutoImageProcessor.from_pretrained(model_name)` (dinov3 main.py:34) builds the
    processor that file names; here its computation is reproduced exactly or the load is refused, naming the file and the
    field — a recipe silently approximated would feed the model other pixels than the reference's service does.

    image_processor_type BitImageProcessor[Fast]: the PIL u8 path (the project stays pinned to the PIL backend for this
    family).  DINOv3ViTImageProcessor[Fast]: the float path.  Refused: another processor; `resample` other than 2 (bilinear) / 3
    (bicubic); do_resize / do_rescale / do_normalize false; a network input (crop_size, or size without a crop) that is not a
    square multiple of the patch size; a crop larger than the resized image where the file alone decides that."""
    from . import dino, resample

    path = Path(model_dir) / PREPROCESSOR_FILE
    if not path.exists():
        return None
    with open(path) as f:
        p = json.load(f)

    def refuse(field, why):
        raise RuntimeError(f"{path}: {field} {why}")

    kind = _PROCESSOR_KINDS.get(p.get("image_processor_type"))
    if kind is None:
        refuse("image_processor_type", f"{p.get('image_processor_type')!r} is not one of {', '.join(_PROCESSOR_KINDS)}")
    get = {**_PROCESSOR_DEFAULTS[kind], **{k: v for k, v in p.items() if v is not None}}.get
    for flag in ("do_resize", "do_rescale", "do_normalize"):
        if not get(flag):
            refuse(flag, "false is not supported (resize, rescale and normalize always run)")
    filt = {2: resample.BILINEAR, 3: resample.BICUBIC}.get(get("resample"))
    if filt is None:
        refuse("resample", f"{get('resample')!r} is not supported (2 bilinear, 3 bicubic)")

    def square(field, v):
        """transformers' get_size_dict: an int is a square, a dict has height and width."""
        if isinstance(v, int) and not isinstance(v, bool):
            v = {"height": v, "width": v}
        if not isinstance(v, dict) or not all(isinstance(v.get(k), int) and v[k] > 0 for k in ("height", "width")):
            refuse(field, f"{v!r} must give a positive height and width")
        if v["height"] != v["width"]:
            refuse(field, f"{v['height']} x {v['width']} is not square (the network input is a square grid of patches)")
        if v["height"] % patch:
            refuse(field, f"{v['height']} is not a multiple of the patch size {patch}")
        return v["height"]

    size = get("size")
    if isinstance(size, int) and not isinstance(size, bool):  # get_size_dict(default_to_square=False) for Bit, square for DINOv3
        size = {"shortest_edge": size} if kind == "pil" else {"height": size, "width": size}
    if not isinstance(size, dict):
        refuse("size", f"{size!r} must be a dictionary")
    crop = square("crop_size", get("crop_size")) if get("do_center_crop") else None
    edge = hw = None
    if set(size) == {"shortest_edge"} and isinstance(size["shortest_edge"], int) and size["shortest_edge"] > 0:
        edge = size["shortest_edge"]
        if crop is None:
            refuse("size", "with shortest_edge only and do_center_crop false gives no square network input")
        if crop > edge:
            refuse("crop_size", f"{crop} is larger than the resized image's shortest edge {edge} (the processor would pad with zeros)")
    elif set(size) == {"height", "width"}:
        if crop is None:
            square("size", size)
        elif not all(isinstance(size[k], int) and size[k] >= crop for k in ("height", "width")):
            refuse("crop_size", f"{crop} is larger than the resized image {size['height']} x {size['width']} (the processor would "
                                "pad with zeros)")
        hw = (size["height"], size["width"])
    else:
        refuse("size", f"{size!r} must hold shortest_edge, or height and width")
    mean, std = get("image_mean"), get("image_std")
    for field, v in (("image_mean", mean), ("image_std", std)):
        if not isinstance(v, (list, tuple)) or len(v) != 3 or not all(isinstance(x, (int, float)) for x in v):
            refuse(field, f"{v!r} must list three numbers")
    if any(x == 0 for x in std):
        refuse("image_std", "holds a zero")
    scale = get("rescale_factor")
    if not isinstance(scale, (int, float)) or isinstance(scale, bool) or not scale > 0:
        refuse("rescale_factor", f"{scale!r} must be a positive number")
    return dino.DinoPreprocess(kind=kind, filt=filt, shortest_edge=edge, size_hw=hw, crop=crop, rescale=float(scale),
                               mean=tuple(float(x) for x in mean), std=tuple(float(x) for x in std))


def load_dino_dir(model_dir):
    """A local Hugging Face model directory (config.json + model.safetensors, optionally preprocessor_config.json) ->
    (DinoConfig, state dict).  The service asks the hub by name (dinov3 main.py:34-35); offline deployments point
    models.dinov3.model_name at such a directory.  With a preprocessor_config.json the configuration carries its recipe
    (`preproc`, read_dino_preprocess) and `image` is the network input that file sets; without one it is the dinov2-base recipe.

    Loads: dinov2 (plain MLP, or `use_swiglu_ffn` as in giant), dinov2_with_registers, dinov3_vit (plain or `use_gated_mlp`, any
    of query / key / value / proj / mlp bias switched off).  Refuses, naming the config field: a head dim the attention kernels do
    not serve (DINOv3-7B's 128), a `hidden_act` other than gelu (plain) / silu (gated), and a checkpoint whose MLP tensors are
    not those of the configured form — a gated checkpoint must not run as a plain MLP, nor the reverse."""
    from . import dino

    d = Path(model_dir)
    with open(d / "config.json") as f:
        c = json.load(f)
    mt = c.get("model_type", "")
    if mt in ("dinov2", "dinov2_with_registers"):
        gated = bool(c.get("use_swiglu_ffn", False))
        ratio = c.get("mlp_ratio", 4)
        cfg = dino.DinoConfig(arch="dinov2", hidden=c["hidden_size"], layers=c["num_hidden_layers"], heads=c["num_attention_heads"],
                              mlp=dino.swiglu_hidden(c["hidden_size"], ratio) if gated else int(c["hidden_size"] * ratio),
                              patch=c["patch_size"], registers=c.get("num_register_tokens", 4) if mt == "dinov2_with_registers" else 0,
                              eps=c.get("layer_norm_eps", 1e-6), pos_grid=c.get("image_size", 518) // c["patch_size"], gated=gated)
        # (Dinov2SwiGLUFFN hard-codes SiLU; hidden_act configures the plain MLP only)
        if not gated and c.get("hidden_act", "gelu") != "gelu":
            raise RuntimeError(f"{d}: hidden_act {c['hidden_act']!r} is not supported (the plain MLP is built with gelu)")
        gate_key, form = "encoder.layer.0.mlp.weights_in.weight", "use_swiglu_ffn"
    elif mt == "dinov3_vit":
        gated = bool(c.get("use_gated_mlp", False))
        cfg = dino.DinoConfig(arch="dinov3", hidden=c["hidden_size"], layers=c["num_hidden_layers"], heads=c["num_attention_heads"],
                              mlp=c["intermediate_size"], patch=c["patch_size"], registers=c.get("num_register_tokens", 4),
                              eps=c.get("layer_norm_eps", 1e-5), rope_theta=c.get("rope_theta", 100.0), gated=gated,
                              q_bias=bool(c.get("query_bias", True)), k_bias=bool(c.get("key_bias", False)),
                              v_bias=bool(c.get("value_bias", True)), proj_bias=bool(c.get("proj_bias", True)),
                              mlp_bias=bool(c.get("mlp_bias", True)))
        want = "silu" if gated else "gelu"
        if c.get("hidden_act", want) != want:
            raise RuntimeError(f"{d}: hidden_act {c['hidden_act']!r} with use_gated_mlp={gated} is not supported (built: gelu for the "
                               "plain MLP, silu for the gated one)")
        gate_key, form = "model.layer.0.mlp.gate_proj.weight", "use_gated_mlp"
    else:
        raise RuntimeError(f"{d}: model_type {mt!r} is not one of dinov2, dinov2_with_registers, dinov3_vit")
    try:
        dino.check_head_dim(cfg)
    except RuntimeError as e:
        raise RuntimeError(f"{d}: {e}") from None
    # the network input follows the file: a dinov2 position table is interpolated to the new grid by DinoEmbedder, RoPE is
    # built for it, and no kernel of the layer sequence bounds the token count, so any multiple of the patch size is served
    pre = read_dino_preprocess(d, cfg.patch)
    if pre is not None:
        cfg = dataclasses.replace(cfg, preproc=pre, image=pre.input_size, resize_edge=pre.shortest_edge or cfg.resize_edge)
    sd = weights.load_state_dict_file(str(d / "model.safetensors"))
    if gated and gate_key not in sd:
        raise RuntimeError(f"{d}: config says {form}=true but the checkpoint has no gate tensor ({gate_key})")
    if not gated and gate_key in sd:
        raise RuntimeError(f"{d}: config says {form}=false but the checkpoint has a gate tensor ({gate_key}): it would run as a "
                           "plain MLP and give wrong embeddings")
    missing = [k for k in dino.param_spec(cfg) if k not in sd]
    if missing:
        raise RuntimeError(f"{d}: {len(missing)} tensors missing, e.g. {missing[:3]}")
    return cfg, {k: np.asarray(v, np.float32) for k, v in sd.items()}


# ---- the TCN gait model (services/tcn-pipeline/app/main.py:242-250: `tcn_lameness.pt`, a plain state_dict) --------------------------
def tcn_from_state_dict(sd, dropout=0.2):
    """A TCN state_dict under the reference's key names -> (lmx.tcn.TcnConfig, folded weights).  The convolutions are weight-normalised:
    `network.{i}.conv{1,2}.conv.parametrizations.weight.original0` (g, [Cout, 1, 1]) and `.original1` (v, [Cout, Cin, k]), or
    `...conv.weight_g` / `...conv.weight_v` as older torch writes them.  They are folded HERE, by torch's own `_weight_norm` — what both
    the parametrisation and the old hook evaluate — so the folded bits are the ones torch would convolve with.  The configuration is
    inferred from the shapes (the dropout probability is not in a state_dict); what the kernel refuses is refused here with the field
    named.  Folded keys: block.{i}.conv{1,2}.{weight,bias}, block.{i}.res.{weight,bias}, head.fc{1,2}.{weight,bias}, all float32."""
    import torch

    from . import tcn
    from ._lib import LmxError

    def conv(prefix):
        for g, v in ((f"{prefix}.parametrizations.weight.original0", f"{prefix}.parametrizations.weight.original1"),
                     (f"{prefix}.weight_g", f"{prefix}.weight_v")):
            if g in sd and v in sd:
                return torch._weight_norm(sd[v].detach().float().cpu(), sd[g].detach().float().cpu(), 0).contiguous()
        if f"{prefix}.weight" in sd:  # a convolution saved without weight norm
            return sd[f"{prefix}.weight"].detach().float().cpu().contiguous()
        raise LmxError(f"tcn_from_state_dict: no weights under {prefix} (neither parametrizations.weight.original0/1 nor weight_g/weight_v)")

    def plain(key):
        if key not in sd:
            raise LmxError(f"tcn_from_state_dict: {key} is missing")
        return sd[key].detach().float().cpu().contiguous()

    n_blocks = 0
    while any(k.startswith(f"network.{n_blocks}.conv1.") for k in sd):
        n_blocks += 1
    if n_blocks == 0:
        raise LmxError("tcn_from_state_dict: no network.0.conv1.* keys: not a TCN state_dict")
    folded, channels = {}, []
    for i in range(n_blocks):
        w1, w2 = conv(f"network.{i}.conv1.conv"), conv(f"network.{i}.conv2.conv")
        folded[f"block.{i}.conv1.weight"], folded[f"block.{i}.conv1.bias"] = w1, plain(f"network.{i}.conv1.conv.bias")
        folded[f"block.{i}.conv2.weight"], folded[f"block.{i}.conv2.bias"] = w2, plain(f"network.{i}.conv2.conv.bias")
        channels.append(int(w1.shape[0]))
        if f"network.{i}.residual.weight" in sd:
            folded[f"block.{i}.res.weight"] = plain(f"network.{i}.residual.weight")
            folded[f"block.{i}.res.bias"] = plain(f"network.{i}.residual.bias")
    folded["head.fc1.weight"], folded["head.fc1.bias"] = plain("classifier.2.weight"), plain("classifier.2.bias")
    folded["head.fc2.weight"], folded["head.fc2.bias"] = plain("classifier.5.weight"), plain("classifier.5.bias")
    w0 = folded["block.0.conv1.weight"]
    if folded["head.fc2.weight"].shape[0] != 1:
        raise LmxError(f"tcn_from_state_dict: num_classes {folded['head.fc2.weight'].shape[0]}: one output class is supported")
    cfg = tcn.TcnConfig(input_dim=int(w0.shape[1]), channels=tuple(channels), kernel_size=int(w0.shape[2]), dropout=float(dropout),
                        head=int(folded["head.fc1.weight"].shape[0])).validate("tcn_from_state_dict")
    for i, n in enumerate(channels):
        has = f"block.{i}.res.weight" in folded
        if has != (cfg.block_inputs(i) != n):
            raise LmxError(f"tcn_from_state_dict: network.{i} has {cfg.block_inputs(i)} inputs and {n} outputs, and "
                           f"{'a' if has else 'no'} residual convolution")
    tcn.pack_tensors(cfg, folded)  # every shape against the configuration
    return cfg, folded


# ---- the gait transformer (services/transformer-pipeline/app/main.py:272-295: `transformer_lameness.pt`, a plain state_dict) ----------
def xfm_positional_table(max_len, d_model):
    """The sinusoidal table of main.py:32-37, computed once in torch float32 exactly as the reference's module builds it: f32 [max_len, D]."""
    import math

    import torch

    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def xfm_from_state_dict(sd, n_heads=4, dropout=0.1, max_len=150):
    """A GaitTransformer state_dict under the reference's key names -> (lmx.xfm.XfmConfig, weights).  Keys read: `input_projection.*`,
    `pos_encoder.pe` ([1, max_len, D]; where it is absent the table is computed once by the formula of main.py:32-37 for `max_len`
    rows), `encoder_layers.{i}.self_attn.in_proj_weight` / `in_proj_bias` / `out_proj.*`, `.ffn.0.*`, `.ffn.3.*`, `.norm1.*`, `.norm2.*`,
    `final_norm.*`, `classifier.0.*` and `classifier.3.*`.  The shape is inferred from the tensors; the number of heads and the dropout
    probability are not in a state_dict.  What the kernel refuses is refused here with the field named.  Weights' keys: in.*, pe,
    layer.{i}.{ln1,qkv,out,ln2,ff1,ff2}.{weight,bias}, lnf.*, head.fc{1,2}.*, all float32 in torch's layouts."""
    from . import xfm
    from ._lib import LmxError

    def plain(key):
        if key not in sd:
            raise LmxError(f"xfm_from_state_dict: {key} is missing")
        return sd[key].detach().float().cpu().contiguous()

    n_layers = 0
    while any(k.startswith(f"encoder_layers.{n_layers}.") for k in sd):
        n_layers += 1
    if n_layers == 0 or "input_projection.weight" not in sd:
        raise LmxError("xfm_from_state_dict: no input_projection.weight or encoder_layers.0.* keys: not a GaitTransformer state_dict")
    w = {"in.weight": plain("input_projection.weight"), "in.bias": plain("input_projection.bias")}
    names = (("ln1", "norm1"), ("qkv", None), ("out", "self_attn.out_proj"), ("ln2", "norm2"), ("ff1", "ffn.0"), ("ff2", "ffn.3"))
    for i in range(n_layers):
        for ours, theirs in names:
            if theirs is None:
                w[f"layer.{i}.qkv.weight"] = plain(f"encoder_layers.{i}.self_attn.in_proj_weight")
                w[f"layer.{i}.qkv.bias"] = plain(f"encoder_layers.{i}.self_attn.in_proj_bias")
            else:
                w[f"layer.{i}.{ours}.weight"] = plain(f"encoder_layers.{i}.{theirs}.weight")
                w[f"layer.{i}.{ours}.bias"] = plain(f"encoder_layers.{i}.{theirs}.bias")
    w["lnf.weight"], w["lnf.bias"] = plain("final_norm.weight"), plain("final_norm.bias")
    w["head.fc1.weight"], w["head.fc1.bias"] = plain("classifier.0.weight"), plain("classifier.0.bias")
    w["head.fc2.weight"], w["head.fc2.bias"] = plain("classifier.3.weight"), plain("classifier.3.bias")
    if w["in.weight"].dim() != 2 or w["layer.0.ff1.weight"].dim() != 2 or w["head.fc1.weight"].dim() != 2 or w["head.fc2.weight"].dim() != 2:
        raise LmxError("xfm_from_state_dict: a linear layer's weight is not a matrix")
    if w["head.fc2.weight"].shape[0] != 1:
        raise LmxError(f"xfm_from_state_dict: num_classes {w['head.fc2.weight'].shape[0]}: one output class is supported")
    d_model = int(w["in.weight"].shape[0])
    if "pos_encoder.pe" in sd:
        pe = plain("pos_encoder.pe")
        pe = pe.reshape(-1, pe.shape[-1]).contiguous()
        max_len = int(pe.shape[0])
    else:
        if not 1 <= int(max_len) <= 160 or d_model % 2:
            raise LmxError(f"xfm_from_state_dict: no pos_encoder.pe, and max_len {max_len} / d_model {d_model} give no table")
        pe = xfm_positional_table(int(max_len), d_model)
    w["pe"] = pe
    cfg = xfm.XfmConfig(input_dim=int(w["in.weight"].shape[1]), d_model=d_model, n_heads=int(n_heads), n_layers=n_layers,
                        ff=int(w["layer.0.ff1.weight"].shape[0]), head=int(w["head.fc1.weight"].shape[0]), dropout=float(dropout),
                        max_len=int(max_len)).validate("xfm_from_state_dict")
    xfm.pack_tensors(cfg, w)  # every shape against the configuration
    return cfg, w


# the reference's module paths of CowLamenessGraphormer -> the names of lmx.gfm's weights ({i}: the layer)
GFM_KEYS = (("input_proj.0", "in"), ("input_proj.1", "in_norm"), ("encodings.temporal_enc.time_proj", "time"),
            ("encodings.edge_enc.edge_proj.0", "edge1"), ("encodings.edge_enc.edge_proj.2", "edge2"), ("encoder.final_norm", "lnf"),
            ("readout.attention_pool.0", "pool1"), ("readout.attention_pool.2", "pool2"), ("readout.combine.0", "comb"),
            ("readout.combine.2", "comb_norm"), ("pred_head.0", "ph1"), ("pred_head.3", "ph2"), ("pred_head.6", "ph3"), ("node_pred.0", "nh1"),
            ("node_pred.3", "nh2"))
GFM_LAYER_KEYS = (("layers.{i}.norm1", "ln1"), ("layers.{i}.self_attn.q_proj", "q"), ("layers.{i}.self_attn.k_proj", "k"),
                  ("layers.{i}.self_attn.v_proj", "v"), ("layers.{i}.self_attn.out_proj", "out"), ("layers.{i}.norm2", "ln2"),
                  ("layers.{i}.ffn.0", "ff1"), ("layers.{i}.ffn.3", "ff2"), ("virtual_node_layers.{i}.vn_attention.q_proj", "vq"),
                  ("virtual_node_layers.{i}.vn_attention.k_proj", "vk"), ("virtual_node_layers.{i}.vn_attention.v_proj", "vv"),
                  ("virtual_node_layers.{i}.vn_attention.out_proj", "vout"), ("virtual_node_layers.{i}.vn_update.0", "vu1"),
                  ("virtual_node_layers.{i}.vn_update.2", "vu2"), ("virtual_node_layers.{i}.vn_update.3", "vu_norm"))


def gfm_from_state_dict(sd, num_heads=8, dropout=0.1):
    """A CowLamenessGraphormer state_dict under the reference's key names (220 of them for six layers: `input_proj.0.weight` ...
    `node_pred.3.bias`, the buffer `encodings.temporal_enc.div_term` included) -> (lmx.gfm.GfmConfig, weights).  The shape is inferred
    from the tensors; the number of heads and the dropout probability are not in a state_dict.  What the kernel refuses is refused
    here with the field named.  Weights' keys: the second names of GFM_KEYS with .weight / .bias, deg_in, deg_out, spd, div_term,
    layer.{i}.<second names of GFM_LAYER_KEYS>.{weight,bias} and layer.{i}.vn, all float32 in torch's layouts."""
    from . import gfm
    from ._lib import LmxError

    def plain(key):
        if key not in sd:
            raise LmxError(f"gfm_from_state_dict: {key} is missing")
        return sd[key].detach().float().cpu().contiguous()

    n_layers = 0
    while any(k.startswith(f"encoder.layers.{n_layers}.") for k in sd):
        n_layers += 1
    if n_layers == 0 or "input_proj.0.weight" not in sd:
        raise LmxError("gfm_from_state_dict: no input_proj.0.weight or encoder.layers.0.* keys: not a CowLamenessGraphormer state_dict")
    w = {}
    for theirs, ours in GFM_KEYS:
        w[f"{ours}.weight"], w[f"{ours}.bias"] = plain(f"{theirs}.weight"), plain(f"{theirs}.bias")
    w["deg_in"] = plain("encodings.centrality_enc.degree_encoder.weight")
    w["deg_out"] = plain("encodings.centrality_enc.out_degree_encoder.weight")
    w["spd"] = plain("encodings.spatial_enc.spd_bias.weight")
    w["div_term"] = plain("encodings.temporal_enc.div_term")
    for i in range(n_layers):
        for theirs, ours in GFM_LAYER_KEYS:
            key = "encoder." + theirs.format(i=i)
            w[f"layer.{i}.{ours}.weight"], w[f"layer.{i}.{ours}.bias"] = plain(key + ".weight"), plain(key + ".bias")
        w[f"layer.{i}.vn"] = plain(f"encoder.virtual_node_layers.{i}.virtual_node").reshape(-1)
    for name in ("in.weight", "layer.0.ff1.weight", "edge1.weight", "spd", "deg_in", "ph3.weight"):
        if w[name].dim() != 2:
            raise LmxError(f"gfm_from_state_dict: {name} is not a matrix")
    if w["ph3.weight"].shape[0] != 1:
        raise LmxError(f"gfm_from_state_dict: {w['ph3.weight'].shape[0]} outputs of the graph head: one is supported")
    cfg = gfm.GfmConfig(input_dim=int(w["in.weight"].shape[1]), d_model=int(w["in.weight"].shape[0]), n_heads=int(num_heads), n_layers=n_layers,
                        ff=int(w["layer.0.ff1.weight"].shape[0]), edge_dim=int(w["edge1.weight"].shape[1]),
                        max_degree=int(w["deg_in"].shape[0]) - 1, max_spd=int(w["spd"].shape[0]) - 2,
                        dropout=float(dropout)).validate("gfm_from_state_dict")
    gfm.pack_tensors(cfg, w)  # every shape against the configuration
    return cfg, w


# EnhancedGraphGPS (services/gnn-pipeline/app/main.py): the reference's module paths and the names lmx.gnn.pack_tensors reads
GNN_KEYS = (("input_proj", "in"), ("lap_pe.transform.0", "lap1"), ("lap_pe.transform.2", "lap2"), ("lap_pe.transform.3", "lap_norm"),
            ("rw_pe.transform.0", "rw1"), ("rw_pe.transform.2", "rw2"), ("rw_pe.transform.3", "rw_norm"), ("edge_encoder.encoder.0", "ee1"),
            ("edge_encoder.encoder.2", "ee2"), ("edge_encoder.encoder.3", "ee_norm"), ("final_norm", "lnf"),
            ("pred_head.node_classifier.0", "nh1"), ("pred_head.node_classifier.3", "nh2"), ("pred_head.node_attention.0", "na1"),
            ("pred_head.node_attention.2", "na2"), ("pred_head.classifier.0", "cl1"), ("pred_head.classifier.3", "cl2"),
            ("pred_head.classifier.6", "cl3"))
GNN_LAYER_KEYS = (("norm1", "ln1"), ("local_conv.A", "A"), ("local_conv.B", "B"), ("local_conv.D", "D"), ("local_conv.E", "E"),
                  ("local_conv.C", "C"), ("norm2", "ln2"), ("global_attn.attention.out_proj", "out"), ("global_attn.norm", "lna"),
                  ("norm3", "ln3"), ("ffn.0", "ff1"), ("ffn.3", "ff2"))
GNN_EDGE_KEYS = (("local_conv.edge_update.0", "eu1"), ("local_conv.edge_update.2", "eu2"))
# what never reaches an output of forward(): dropped BY PREFIX, whatever lies below (SAGPooling's inner names are torch_geometric's)
GNN_DEAD_PREFIXES = ("pool_layer.", "post_pool_layers.", "multi_scale_readout.")


def gnn_from_state_dict(sd, num_heads=8, dropout=0.1):
    """An EnhancedGraphGPS state_dict under the reference's key names -> (lmx.gnn.GnnConfig, weights) of the LIVE network: input_proj,
    edge_encoder, the transform MLPs of lap_pe / rw_pe, pre_pool_layers (the last one without its edge update), final_norm, pred_head.
    pool_layer.*, post_pool_layers.*, multi_scale_readout.*, the last live layer's local_conv.edge_update.* / local_conv.bn_edge.* and
    every global_attn.pe_bias.* (a parameter forward never applies) are accepted and dropped by prefix; num_batches_tracked likewise.
    Any other key that is not read is refused by name, and so is the legacy GraphGPS class.  The shape is inferred from the tensors;
    the number of heads and the dropout probability are not in a state_dict.  BatchNorm's running statistics must be there: the eval
    launch normalises with them."""
    from . import gnn
    from ._lib import LmxError

    who = "gnn_from_state_dict"
    if any(k.startswith("layers.") for k in sd) or "pred_head.0.weight" in sd:
        raise LmxError(f"{who}: a GraphGPS state_dict (layers.*, pred_head.0): the legacy class is not served, only EnhancedGraphGPS")
    n_layers = 0
    while any(k.startswith(f"pre_pool_layers.{n_layers}.") for k in sd):
        n_layers += 1
    if n_layers == 0 or "input_proj.weight" not in sd:
        raise LmxError(f"{who}: no input_proj.weight or pre_pool_layers.0.* keys: not an EnhancedGraphGPS state_dict")
    used = set()

    def plain(key):
        if key not in sd:
            raise LmxError(f"{who}: {key} is missing")
        used.add(key)
        return sd[key].detach().float().cpu().contiguous()

    w = {}
    for theirs, ours in GNN_KEYS:
        w[f"{ours}.weight"], w[f"{ours}.bias"] = plain(f"{theirs}.weight"), plain(f"{theirs}.bias")
    for i in range(n_layers):
        p, q = f"pre_pool_layers.{i}.", f"layer.{i}."
        for theirs, ours in GNN_LAYER_KEYS + (GNN_EDGE_KEYS if i < n_layers - 1 else ()):
            w[f"{q}{ours}.weight"], w[f"{q}{ours}.bias"] = plain(f"{p}{theirs}.weight"), plain(f"{p}{theirs}.bias")
        for theirs, ours in (("local_conv.bn_node", "bnn"),) + ((("local_conv.bn_edge", "bne"),) if i < n_layers - 1 else ()):
            for field in ("weight", "bias", "running_mean", "running_var"):
                w[f"{q}{ours}.{field}"] = plain(f"{p}{theirs}.{field}")
        w[q + "in_proj.weight"], w[q + "in_proj.bias"] = plain(p + "global_attn.attention.in_proj_weight"), plain(p + "global_attn.attention.in_proj_bias")
    last = f"pre_pool_layers.{n_layers - 1}.local_conv."
    dead = GNN_DEAD_PREFIXES + (last + "edge_update.", last + "bn_edge.")
    for k in sd:
        if k in used or k.startswith(dead) or ".global_attn.pe_bias." in k or k.endswith(".num_batches_tracked"):
            continue
        raise LmxError(f"{who}: {k} is neither read nor one of the keys that reach no output")
    for name in ("in.weight", "lap1.weight", "layer.0.ff1.weight", "ee1.weight", "cl3.weight", "nh2.weight"):
        if w[name].dim() != 2:
            raise LmxError(f"{who}: {name} is not a matrix")
    if w["cl3.weight"].shape[0] != 1 or w["nh2.weight"].shape[0] != 1:
        raise LmxError(f"{who}: {w['cl3.weight'].shape[0]} outputs of the graph head, {w['nh2.weight'].shape[0]} of the node head: one is supported")
    pe_dim = int(w["lap2.weight"].shape[0])
    cfg = gnn.GnnConfig(input_dim=int(w["in.weight"].shape[1]), d_model=int(w["in.weight"].shape[0]) + 2 * pe_dim, n_heads=int(num_heads),
                        n_layers=n_layers, pe_dim=pe_dim, ff=int(w["layer.0.ff1.weight"].shape[0]), edge_dim=int(w["ee1.weight"].shape[1]),
                        dropout=float(dropout)).validate(who)
    gnn.pack_tensors(cfg, w)  # every shape against the configuration
    return cfg, w
