"""Float64-capable torch restatement of the SAM prompt paths beyond the box (segment_anything PromptEncoder / MaskDecoder /
Sam.postprocess_masks, public source; pinned to transformers' SamModel by tests/test_sam_prompt_ref_host.py): point encoding,
the mask embedding, the dense override, the all-four-mask decode and the un-thresholded postprocess.  It reuses
oracle.sam_decoder's attention / LayerNorm / MLP helpers, which run in whatever dtype the state dict holds.

`defect` switches build the models of wrong implementations the bounds must reject (tests/test_sam_prompt_ref_host.py):
  "neg1_zero"  label -1 tokens are zeros (a padding token) instead of not_a_point_embed
  "no_ln1" / "no_ln2"  a LayerNorm2d of the mask embedding dropped
  "tanh_gelu"  the tanh approximation of GELU in the mask embedding
  "slice012"  multimask output taken as masks 0..2 instead of 1..3
Also the mask-embedding error bound of the GPU kernel (mask_embed_bound)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sam_decoder as OD

ME = "prompt_encoder.mask_embed."


def sd_as(sd, dtype):
    """{name: tensor of `dtype`} (float64 for the reference)."""
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}


def scale_coords(xy, orig_hw, resized_hw):
    """ResizeLongestSide.apply_coords: x * (new_w / old_w), y * (new_h / old_h) in float64, then the f32 tensor."""
    c = np.asarray(xy, np.float64).copy()
    c[..., 0] = c[..., 0] * (resized_hw[1] / orig_hw[1])
    c[..., 1] = c[..., 1] * (resized_hw[0] / orig_hw[0])
    return c.astype(np.float32)


def _pe(sd, coords01):
    c = 2 * coords01 - 1
    c = 2 * np.pi * (c @ sd["shared_image_embedding.positional_embedding"])
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)


def encode_prompts(sd, points=None, labels=None, boxes=None, image_size=1024, defect=None):
    """sd: sd_as(...) tensors.  points [n,Np,2] / boxes [n,4] in 1024-space (already scaled, f32 values), labels [n,Np] ->
    sparse [n,Ns,256]: [points..., box corners], or [points..., pad (label -1)] without a box."""
    dt = sd["shared_image_embedding.positional_embedding"].dtype
    toks = []
    if points is not None:
        p = torch.as_tensor(np.asarray(points)).to(dt) + 0.5
        lab = torch.as_tensor(np.asarray(labels)).long()
        if boxes is None:
            p = torch.cat([p, torch.zeros_like(p[:, :1])], 1)
            lab = torch.cat([lab, -torch.ones_like(lab[:, :1])], 1)
        pe = _pe(sd, p / image_size)
        neg = (lab == -1)[..., None]
        nap = torch.zeros_like(pe) if defect == "neg1_zero" else sd["prompt_encoder.not_a_point_embed.weight"][0].expand_as(pe)
        pe = torch.where(neg, nap, pe)
        pe = pe + (lab == 0)[..., None] * sd["prompt_encoder.point_embed.0.weight"][0]
        pe = pe + (lab == 1)[..., None] * sd["prompt_encoder.point_embed.1.weight"][0]
        toks.append(pe)
    if boxes is not None:
        b = torch.as_tensor(np.asarray(boxes)).to(dt).reshape(-1, 2, 2) + 0.5
        pe = _pe(sd, b / image_size)
        pe = torch.stack([pe[:, 0] + sd["prompt_encoder.point_embed.2.weight"][0], pe[:, 1] + sd["prompt_encoder.point_embed.3.weight"][0]], 1)
        toks.append(pe)
    return torch.cat(toks, 1)


def _ln2d(x, g, b, eps=1e-6):
    u = x.mean(1, keepdim=True)
    s = ((x - u) ** 2).mean(1, keepdim=True)
    return g[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


def _gelu(x, defect):
    return F.gelu(x, approximate="tanh") if defect == "tanh_gelu" else F.gelu(x)


def mask_embed(sd, mask, defect=None, parts=False):
    """SamMaskEmbedding: mask [n,256,256] -> dense [n,256,64,64] (parts=True: also the intermediates for the bound)."""
    x = torch.as_tensor(mask).to(sd[ME + "conv1.weight"].dtype)[:, None]
    h1 = F.conv2d(x, sd[ME + "conv1.weight"], sd[ME + "conv1.bias"], stride=2)
    y1 = h1 if defect == "no_ln1" else _ln2d(h1, sd[ME + "layer_norm1.weight"], sd[ME + "layer_norm1.bias"])
    a1 = _gelu(y1, defect)
    h2 = F.conv2d(a1, sd[ME + "conv2.weight"], sd[ME + "conv2.bias"], stride=2)
    y2 = h2 if defect == "no_ln2" else _ln2d(h2, sd[ME + "layer_norm2.weight"], sd[ME + "layer_norm2.bias"])
    a2 = _gelu(y2, defect)
    dense = F.conv2d(a2, sd[ME + "conv3.weight"], sd[ME + "conv3.bias"])
    return (dense, dict(x=x, h1=h1, y1=y1, a1=a1, h2=h2, y2=y2, a2=a2)) if parts else dense


def image_pe(sd, size=64):
    dt = sd["shared_image_embedding.positional_embedding"].dtype
    grid = torch.ones((size, size), dtype=dt)
    y = (grid.cumsum(dim=0) - 0.5) / size
    x = (grid.cumsum(dim=1) - 0.5) / size
    return _pe(sd, torch.stack([x, y], dim=-1))  # [64,64,256]


def decode_all(sd, image_emb, sparse, dense=None):
    """MaskDecoder on T = 5 + Ns tokens: image_emb [n,256,64,64], sparse [n,Ns,256], dense [n,256,64,64] or None (the no-mask
    embedding) -> (low-res logits of all four masks [n,4,256,256], iou [n,4])."""
    n, c, h, w = image_emb.shape
    tokens = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]], 0)
    tokens = torch.cat([tokens[None].expand(n, -1, -1), sparse], dim=1)
    if dense is None:
        dense = sd["prompt_encoder.no_mask_embed.weight"].reshape(1, -1, 1, 1)
    keys = (image_emb + dense).flatten(2).transpose(1, 2)
    key_pe = image_pe(sd, h).reshape(1, h * w, c)
    queries, qpe = tokens, tokens
    for i in range(2):
        p = f"mask_decoder.transformer.layers.{i}."
        if i == 0:
            queries = OD._attn(sd, p + "self_attn.", queries, queries, queries)
        else:
            q = queries + qpe
            queries = queries + OD._attn(sd, p + "self_attn.", q, q, queries)
        queries = OD._ln(sd, p + "layer_norm1.", queries)
        queries = queries + OD._attn(sd, p + "cross_attn_token_to_image.", queries + qpe, keys + key_pe, keys)
        queries = OD._ln(sd, p + "layer_norm2.", queries)
        m = F.linear(F.relu(F.linear(queries, sd[p + "mlp.lin1.weight"], sd[p + "mlp.lin1.bias"])), sd[p + "mlp.lin2.weight"], sd[p + "mlp.lin2.bias"])
        queries = OD._ln(sd, p + "layer_norm3.", queries + m)
        keys = keys + OD._attn(sd, p + "cross_attn_image_to_token.", keys + key_pe, queries + qpe, queries)
        keys = OD._ln(sd, p + "layer_norm4.", keys)
    p = "mask_decoder.transformer."
    queries = queries + OD._attn(sd, p + "final_attn_token_to_image.", queries + qpe, keys + key_pe, keys)
    queries = F.layer_norm(queries, (c,), sd[p + "layer_norm_final_attn.weight"], sd[p + "layer_norm_final_attn.bias"], 1e-5)
    iou_tok, mask_tok = queries[:, 0], queries[:, 1:5]
    x = keys.transpose(1, 2).reshape(n, c, h, w)
    x = F.conv_transpose2d(x, sd["mask_decoder.upscale_conv1.weight"], sd["mask_decoder.upscale_conv1.bias"], stride=2)
    x = F.gelu(OD._ln(sd, "mask_decoder.upscale_layer_norm.", x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
    x = F.gelu(F.conv_transpose2d(x, sd["mask_decoder.upscale_conv2.weight"], sd["mask_decoder.upscale_conv2.bias"], stride=2))
    hyper = torch.stack([OD._ffn(sd, f"mask_decoder.output_hypernetworks_mlps.{i}.", mask_tok[:, i], 1) for i in range(4)], 1)
    masks = (hyper @ x.flatten(2)).reshape(n, 4, x.shape[2], x.shape[3])
    return masks, OD._ffn(sd, "mask_decoder.iou_prediction_head.", iou_tok, 1)


def select(masks, iou, multimask, defect=None):
    """segment_anything's output selection: masks 1..3 with multimask, else mask 0 ("slice012": the defect 0..2)."""
    if not multimask:
        return masks[:, :1], iou[:, :1]
    s = slice(0, 3) if defect == "slice012" else slice(1, 4)
    return masks[:, s], iou[:, s]


def postprocess_logits(lowres, resized_hw, orig_hw, target=1024):
    """Sam.postprocess_masks without the threshold: lowres [n,C,256,256] -> logits [n,C,H,W]."""
    m = F.interpolate(lowres, (target, target), mode="bilinear", align_corners=False)
    m = m[..., :resized_hw[0], :resized_hw[1]]
    return F.interpolate(m, orig_hw, mode="bilinear", align_corners=False)


def predict(sd, image_emb, orig_hw, resized_hw, points=None, labels=None, box=None, mask_input=None, multimask=False, defect=None):
    """The whole SamPredictor.predict_torch for n frames in sd's dtype: points [n,Np,2] / box [n,4] in FRAME pixels ->
    (low-res logits [n,C,256,256], iou [n,C], sparse, dense)."""
    pts = None if points is None else scale_coords(points, orig_hw, resized_hw)
    bx = None if box is None else scale_coords(np.asarray(box, np.float64).reshape(-1, 2, 2), orig_hw, resized_hw).reshape(-1, 4)
    sparse = encode_prompts(sd, pts, labels, bx, defect=defect)
    dense = None if mask_input is None else mask_embed(sd, mask_input, defect=defect)
    masks, iou = decode_all(sd, image_emb.to(sparse.dtype), sparse, dense)
    low, sc = select(masks, iou, multimask, defect)
    return low, sc, sparse, dense


U32 = 2.0 ** -24


def mask_embed_bound(sd64, mask, emb, C=4.0):
    """Per-element float64 bound on |kernel - reference| of lmx_k_mask_embed's keys [n*4096,256] (= emb + dense, NHWC rows):
    C u (|emb| + |b3| + sum_c |w3_kc| (|a2_c| + E2_c)), u = 2^-24, with the first-order error of each LayerNorm2d + GELU stage
    carried forward as E:  E1 = 1.13 (|g1| r1 max_c S1 + |y1|),  S2 = |b2| + sum |w2| (|a1| + E1),
    E2 = 1.13 (|g2| r2 max_o S2 + |y2|), S1 = |b1| + sum |w1| |m|; r = 1/sqrt(var + eps) of the LayerNorm, 1.13 = max |GELU'|."""
    dense, P = mask_embed(sd64, mask, parts=True)
    ab = lambda k: sd64[ME + k].abs()  # noqa: E731
    S1 = F.conv2d(P["x"].abs(), ab("conv1.weight"), ab("conv1.bias"), stride=2)
    var1 = ((P["h1"] - P["h1"].mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    E1 = 1.13 * (ab("layer_norm1.weight")[:, None, None] * S1.amax(1, keepdim=True) / torch.sqrt(var1 + 1e-6) + P["y1"].abs())
    S2 = F.conv2d(P["a1"].abs() + E1, ab("conv2.weight"), ab("conv2.bias"), stride=2)
    var2 = ((P["h2"] - P["h2"].mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
    E2 = 1.13 * (ab("layer_norm2.weight")[:, None, None] * S2.amax(1, keepdim=True) / torch.sqrt(var2 + 1e-6) + P["y2"].abs())
    S3 = F.conv2d(P["a2"].abs() + E2, ab("conv3.weight"), ab("conv3.bias"))
    n = dense.shape[0]
    e = torch.as_tensor(emb).double().reshape(n, 64, 64, 256)
    ref = e + dense.permute(0, 2, 3, 1)
    bound = C * U32 * (e.abs() + S3.permute(0, 2, 3, 1))
    return ref.reshape(n * 4096, 256), bound.reshape(n * 4096, 256)
