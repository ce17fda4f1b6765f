"""Test helper: the reference restatement of transformers' DINOv3ViTImageProcessor, and model directories with a
preprocessor_config.json.

DINOv3ViTImageProcessor (transformers/models/dinov3_vit/image_processing_dinov3_vit.py) is a torchvision-backend processor and
cannot be instantiated where torchvision is missing, so its `_preprocess` is restated here step by step on torch CPU float32:
  rescale    image * rescale_factor                      (TorchvisionBackend.rescale on the uint8 tensor)
  resize     tvF.resize(float tensor, antialias=True)   = F.interpolate(x, size, mode, align_corners=False, antialias=True)
  crop       optional centre crop, int((size - crop) / 2)
  normalize  tvF.normalize: (x - mean) / std
The resize line is this project's reading of torchvision (parity is not pinned against torchvision itself)."""
import json

import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MODES = {2: "bilinear", 3: "bicubic"}


def dinov3_pixel_values(frames_rgb, size_hw=(224, 224), resample=2, rescale_factor=1 / 255, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        crop=None):
    """u8 RGB [n,h,w,3] (numpy) -> float32 [n,3,H,W] pixel_values, torch CPU."""
    x = torch.from_numpy(np.ascontiguousarray(frames_rgb)).permute(0, 3, 1, 2).contiguous()
    x = x * rescale_factor
    assert x.dtype == torch.float32
    x = torch.nn.functional.interpolate(x, size=tuple(size_hw), mode=MODES[resample], align_corners=False, antialias=True)
    if crop is not None:
        top, left = int((x.shape[2] - crop) / 2.0), int((x.shape[3] - crop) / 2.0)
        x = x[:, :, top:top + crop, left:left + crop]
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (x - m) / s


def patch_matrix(pv, P):
    """pixel_values [n,3,H,W] -> [n*gh*gw, P*P*3] in the (ky, kx, c) column order of lmx_k_patchify_norm."""
    n, c, H, W = pv.shape
    gh, gw = H // P, W // P
    return pv.view(n, c, gh, P, gw, P).permute(0, 2, 4, 3, 5, 1).reshape(n * gh * gw, P * P * c).contiguous()


def dinov3_preprocessor_config(size=224, resample=2, **extra):
    """A preprocessor_config.json as DINOv3ViTImageProcessor.save_pretrained writes it (the class defaults of the installed
    transformers unless overridden)."""
    d = {"image_processor_type": "DINOv3ViTImageProcessor", "do_resize": True, "size": {"height": size, "width": size},
         "resample": resample, "do_rescale": True, "rescale_factor": 1 / 255, "do_normalize": True,
         "image_mean": list(IMAGENET_MEAN), "image_std": list(IMAGENET_STD)}
    d.update(extra)
    return d


def dinov2_preprocessor_config(shortest_edge=256, crop=224, resample=3, **extra):
    """What facebook/dinov2-* directories carry."""
    d = {"image_processor_type": "BitImageProcessor", "do_resize": True, "size": {"shortest_edge": shortest_edge}, "resample": resample,
         "do_center_crop": True, "crop_size": {"height": crop, "width": crop}, "do_rescale": True, "rescale_factor": 1 / 255,
         "do_normalize": True, "image_mean": list(IMAGENET_MEAN), "image_std": list(IMAGENET_STD), "do_convert_rgb": True}
    d.update(extra)
    return d


def dinov3_hf_config(cfg):
    """config.json of a dinov3_vit directory for an lmx DinoConfig."""
    return {"model_type": "dinov3_vit", "hidden_size": cfg.hidden, "num_hidden_layers": cfg.layers, "num_attention_heads": cfg.heads,
            "intermediate_size": cfg.mlp, "patch_size": cfg.patch, "num_register_tokens": cfg.registers, "layer_norm_eps": cfg.eps,
            "rope_theta": cfg.rope_theta, "use_gated_mlp": cfg.gated, "hidden_act": "silu" if cfg.gated else "gelu",
            "query_bias": cfg.q_bias, "key_bias": cfg.k_bias, "value_bias": cfg.v_bias, "proj_bias": cfg.proj_bias,
            "mlp_bias": cfg.mlp_bias}


def write_model_dir(path, hf_config, state_dict, preprocessor=None):
    """config.json + model.safetensors (+ preprocessor_config.json) in `path`."""
    from safetensors.numpy import save_file

    (path / "config.json").write_text(json.dumps(hf_config))
    save_file({k: np.ascontiguousarray(v) for k, v in state_dict.items()}, str(path / "model.safetensors"))
    if preprocessor is not None:
        (path / "preprocessor_config.json").write_text(json.dumps(preprocessor))
    return path
