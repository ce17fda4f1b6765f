"""SAM prompt encoder + mask decoder + mask post-processing on liblmx — ``predictor.predict(...)`` of segment_anything: the
``box=..., multimask_output=False`` call of services/sam3-pipeline/app/main.py:83-89 through
predict(), every other prompt (points, mask input, multimask, logits) through decode().  The decoder is SAM v1's; it consumes a
[n,64,64,256] image embedding, so it serves the Hiera FPN level-2 output (BASELINE cfg#3/#5) and a SAM ViT neck alike.

Launch sequence per batch of n frames (all through the C-ABI; activations f32 in HBM, GEMM operands f16):
  prompt : 2 box corners -> random-Fourier PE + corner embeddings (lmx_k_prompt_box); decode(): points + labels (+ box) ->
           Ns sparse tokens (lmx_k_prompt_points), a mask input -> SamMaskEmbedding + image embedding (lmx_k_mask_embed)
  decoder: two-way transformer on T = 5 + Ns tokens (7 for a box) x 4096 image tokens (GEMMs batched over frames; flash
           attention kernel with Tq=T/Tk=4096 and Tq=4096/Tk=T), then the upscaler as two per-pixel GEMMs (ConvTranspose2d k2 s2
           == a 1x1 GEMM to 4*Cout channels + pixel shuffle, so LayerNorm2d/GELU stay row-wise and the shuffle is folded into the
           final hyper-network dot product), lmx_k_hyper_mask_multi -> 256x256 logits of mask 0 (or of masks 1..3 in one pass)
  post   : lmx_k_mask_post: bilinear 256->1024, crop, bilinear -> frame size, >0, plus area / centroid sums / bounding box
           (lmx_k_mask_logits: the same without the threshold).
"""
import math

import numpy as np
import torch

from . import kernels as K

D = 256
HEADS = 8


def param_spec():
    """Ordered {transformers SamModel parameter name: (shape, init kind)} for the prompt encoder + mask decoder."""
    s = {}
    s["shared_image_embedding.positional_embedding"] = ((2, 128), "tok")
    s["prompt_encoder.shared_embedding.positional_embedding"] = ((2, 128), "tok")
    s["prompt_encoder.no_mask_embed.weight"] = ((1, D), "tok")
    for i in range(4):
        s[f"prompt_encoder.point_embed.{i}.weight"] = ((1, D), "tok")
    s["prompt_encoder.not_a_point_embed.weight"] = ((1, D), "tok")
    s["mask_decoder.iou_token.weight"] = ((1, D), "tok")
    s["mask_decoder.mask_tokens.weight"] = ((4, D), "tok")

    def attn(p, inner):
        for n_ in ("q_proj", "k_proj", "v_proj"):
            s[p + n_ + ".weight"] = ((inner, D), "w")
            s[p + n_ + ".bias"] = ((inner,), "b")
        s[p + "out_proj.weight"] = ((D, inner), "w")
        s[p + "out_proj.bias"] = ((D,), "b")

    def ln(p, d=D):
        s[p + "weight"] = ((d,), "g")
        s[p + "bias"] = ((d,), "b")

    for i in range(2):
        p = f"mask_decoder.transformer.layers.{i}."
        attn(p + "self_attn.", D)
        ln(p + "layer_norm1.")
        attn(p + "cross_attn_token_to_image.", D // 2)
        ln(p + "layer_norm2.")
        s[p + "mlp.lin1.weight"] = ((2048, D), "w")
        s[p + "mlp.lin1.bias"] = ((2048,), "b")
        s[p + "mlp.lin2.weight"] = ((D, 2048), "w")
        s[p + "mlp.lin2.bias"] = ((D,), "b")
        ln(p + "layer_norm3.")
        ln(p + "layer_norm4.")
        attn(p + "cross_attn_image_to_token.", D // 2)
    attn("mask_decoder.transformer.final_attn_token_to_image.", D // 2)
    ln("mask_decoder.transformer.layer_norm_final_attn.")
    s["mask_decoder.upscale_conv1.weight"] = ((D, 64, 2, 2), "w")
    s["mask_decoder.upscale_conv1.bias"] = ((64,), "b")
    s["mask_decoder.upscale_conv2.weight"] = ((64, 32, 2, 2), "w")
    s["mask_decoder.upscale_conv2.bias"] = ((32,), "b")
    ln("mask_decoder.upscale_layer_norm.", 64)

    def ffn(p, hid, out):
        s[p + "proj_in.weight"] = ((hid, D), "w")
        s[p + "proj_in.bias"] = ((hid,), "b")
        s[p + "proj_out.weight"] = ((out, hid), "w")
        s[p + "proj_out.bias"] = ((out,), "b")
        s[p + "layers.0.weight"] = ((hid, hid), "w")
        s[p + "layers.0.bias"] = ((hid,), "b")

    for i in range(4):
        ffn(f"mask_decoder.output_hypernetworks_mlps.{i}.", D, 32)
    ffn("mask_decoder.iou_prediction_head.", 256, 4)
    return s


def mask_embed_param_spec():
    """Ordered {name: (shape, init kind)} of SamMaskEmbedding (the dense prompt of a `mask_input`), in the order
    lmx_k_mask_embed's parameter block packs them.  Kept apart from param_spec(): checkpoints hold these tensors, but a
    decoder built without them still serves every prompt except `mask_input`."""
    p = "prompt_encoder.mask_embed."
    s = {}
    for conv, ln, cin, cout, k in (("conv1", "layer_norm1", 1, 4, 2), ("conv2", "layer_norm2", 4, 16, 2), ("conv3", None, 16, D, 1)):
        s[p + conv + ".weight"] = ((cout, cin, k, k), "w")
        s[p + conv + ".bias"] = ((cout,), "b")
        if ln:
            s[p + ln + ".weight"] = ((cout,), "g")
            s[p + ln + ".bias"] = ((cout,), "b")
    return s


def synthetic_state_dict(seed):
    """Synthetic decoder weights.  SAM has ONE random-Fourier matrix (segment_anything's pe_layer) used for both the
    prompt points and the dense image PE; transformers stores it under two tied names, so both get the same values."""
    from . import weights

    sd = weights.synth_state_dict(param_spec(), seed)
    sd["prompt_encoder.shared_embedding.positional_embedding"] = sd["shared_image_embedding.positional_embedding"].copy()
    return sd


def linear_f32(sd, prefix):
    """(w [N, K], b [N]) of the decoder's Linear `prefix` as a GEMM takes them.  The two upscale ConvTranspose2d(k2, s2) are per-pixel
    GEMMs: Wg[(dy,dx,co), ci] = W[ci,co,dy,dx], the bias repeated per quadrant."""
    w, b = sd[prefix + ".weight"], sd[prefix + ".bias"]
    if prefix.startswith("mask_decoder.upscale_conv"):
        w, b = np.transpose(w, (2, 3, 1, 0)).reshape(4 * w.shape[1], w.shape[0]), np.tile(b, 4)
    return w, b


class _PlanF16:
    """Throughput plan: f16 GEMM operands, one K.gemm per Linear on the uploaded (w f16, b f32), flash attention in f16."""

    def __init__(self, dec):
        self.dec, self.w = dec, dec._w16

    def operand(self, x, pe=None):
        """x (+ pe) f32 in the form linear() takes"""
        return K.cast_f16(x) if pe is None else K.add_bcast(x, pe, out_dtype=torch.float16)

    def linear(self, a, name, act=K.ACT_NONE, res=None, out_dtype=torch.float16):
        w, b = self.w[name]
        return K.gemm(a, w, b, act, None, res, None, out_dtype)  # (positional: this sits in front of every GEMM of the dense schedule)

    def attention(self, q, k, v, n, tq, tk):
        hd = q.shape[1] // HEADS
        a = torch.empty((n * tq, q.shape[1]), dtype=torch.float16, device=q.device)
        K.attention(q, k, v, a, n, HEADS, tq, tk, hd, hd ** -0.5)
        return a

    def upscale_and_mask(self, x, hyper, n):
        """GELUs in the epilogues of the LayerNorm and of the second GEMM; hyper() runs behind the upscaler"""
        dec = self.dec
        u = self.linear(x, "mask_decoder.upscale_conv1", out_dtype=torch.float32)                        # [n*P, 4*64]
        u = K.layernorm(u.view(-1, 64), *dec.up_ln, 1e-6, act=K.ACT_GELU)                                # f16 [n*P*4, 64]
        u = self.linear(u, "mask_decoder.upscale_conv2", act=K.ACT_GELU)                                 # f16 [n*P*4, 4*32]
        return K.hyper_mask_multi(u, hyper(), n, dec.G, 32)                                              # one pass over u for all M masks


class _PlanExact:
    """Exact plan (csrc/exact.hip): f32 activations, 22-bit GEMM operands (MaskDecoder._x3), f32 attention."""

    def __init__(self, dec):
        self.dec = dec

    def operand(self, x, pe=None):
        return x if pe is None else K.add_bcast(x, pe, out_dtype=torch.float32)

    def linear(self, a, name, act=K.ACT_NONE, res=None, out_dtype=torch.float32, act_in=K.ACT_NONE):
        """y = act(act_in(a) @ W^T + b) (+ res): a f32 [rows, K] is split into x3 rows (after act_in), then ONE lmx_k_gemm launch over
        3K with f32 output.  act may be NONE or RELU (it commutes with the positive row scale)."""
        w3, b3, sc = self.dec._x3(name)
        return K.gemm(K.split3_rows(a, act_in), w3, bias=b3, act=act, scale=sc, res=res, out_dtype=torch.float32)

    def attention(self, q, k, v, n, tq, tk):
        hd = q.shape[1] // HEADS
        return K.attention_f32(q, k, v, n, HEADS, tq, tk, hd, hd ** -0.5)

    def upscale_and_mask(self, x, hyper, n):
        """exact GELUs folded into the next split / the final dot product"""
        dec = self.dec
        u = self.linear(x, "mask_decoder.upscale_conv1")                                                  # [n*P, 4*64]
        u = K.layernorm(u.view(-1, 64), *dec.up_ln, 1e-6, out_dtype=torch.float32)
        u = self.linear(u, "mask_decoder.upscale_conv2", act_in=K.ACT_GELU)                              # [n*P*4, 4*32], pre-GELU
        return K.hyper_mask_multi_f32(u, hyper(), n, dec.G, 32, act=K.ACT_GELU)


class MaskDecoder:
    """Device-resident SAM prompt encoder + mask decoder.  ``predict(emb, boxes, frame_hw, resized_hw)`` -> dict(mask u8
    [n,h,w], stats int64 [n,8], iou f32 [n], lowres f32 [n,256,256]); ``decode(...)`` serves every prompt of
    SamPredictor.predict (points, box, mask input, multimask, logits)."""

    def __init__(self, state_dict, device="cuda", image_size=1024, grid=64, precision="exact"):
        """precision: the default plan of predict() — "exact" (services, adapters, the reference schedule: f32 activations,
        22-bit GEMM operands, f32 attention; masks within IoU 0.9995 of the fp32 path) or "f16" (the dense throughput
        schedule: f16 GEMM operands)."""
        self._w16 = {}  # state-dict prefix -> (w f16 [N, K], b f32 [N]): the f16 plan's Linears, which the attributes below hold by role
        self._plans = {"f16": _PlanF16(self), "exact": _PlanExact(self)}
        self.precision = precision
        self._plan(None)
        self.device = torch.device(device)
        self.S, self.G = image_size, grid
        dev = self.device
        sd = state_dict
        self._sd = {k: np.asarray(v, np.float32) for k, v in sd.items() if k.startswith("mask_decoder.")}
        self._wx = {}

        def t32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def t16(a):
            return t32(a).to(torch.float16).contiguous()

        gauss = sd["shared_image_embedding.positional_embedding"].astype(np.float32)
        self.gauss = t32(gauss)
        self.corner = t32(np.concatenate([sd["prompt_encoder.point_embed.2.weight"], sd["prompt_encoder.point_embed.3.weight"]], 0))
        # dense image PE (get_image_wide_positional_embeddings), a constant of the weights: f32 torch ops on the host once
        g = torch.ones((grid, grid), dtype=torch.float32)
        yx = torch.stack([(g.cumsum(1) - 0.5) / grid, (g.cumsum(0) - 0.5) / grid], -1)
        c = 2 * np.pi * ((2 * yx - 1) @ torch.from_numpy(gauss))
        self.key_pe = torch.cat([torch.sin(c), torch.cos(c)], -1).reshape(grid * grid, D).contiguous().to(dev)
        self.no_mask = t32(sd["prompt_encoder.no_mask_embed.weight"])                          # [1,256]
        self.point_embed = t32(np.concatenate([sd["prompt_encoder.point_embed.0.weight"], sd["prompt_encoder.point_embed.1.weight"]], 0))
        self.not_a_point = t32(sd["prompt_encoder.not_a_point_embed.weight"][0])
        me = mask_embed_param_spec()
        self.mask_params = t32(np.concatenate([np.asarray(sd[k], np.float32).ravel() for k in me])) if all(k in sd for k in me) else None
        self.out_tokens = t32(np.concatenate([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]], 0))

        def lin(prefix):
            w, b = linear_f32(self._sd, prefix)
            self._w16[prefix] = (t16(w), t32(b))
            return self._w16[prefix]

        def attn(p):
            return {n_: lin(p + n_) for n_ in ("q_proj", "k_proj", "v_proj", "out_proj")}

        def ln(p):
            return t32(sd[p + "weight"]), t32(sd[p + "bias"])

        self.layers = []
        for i in range(2):
            p = f"mask_decoder.transformer.layers.{i}."
            self.layers.append(dict(sa=attn(p + "self_attn."), ln1=ln(p + "layer_norm1."),
                                    t2i=attn(p + "cross_attn_token_to_image."), ln2=ln(p + "layer_norm2."),
                                    w1=lin(p + "mlp.lin1"), w2=lin(p + "mlp.lin2"),
                                    ln3=ln(p + "layer_norm3."), ln4=ln(p + "layer_norm4."),
                                    i2t=attn(p + "cross_attn_image_to_token.")))
        self.final = attn("mask_decoder.transformer.final_attn_token_to_image.")
        self.ln_final = ln("mask_decoder.transformer.layer_norm_final_attn.")
        self.up1, self.up2 = lin("mask_decoder.upscale_conv1"), lin("mask_decoder.upscale_conv2")
        self.up_ln = ln("mask_decoder.upscale_layer_norm.")

        def ffn(p):
            return [lin(p + n_) for n_ in ("proj_in", "layers.0", "proj_out")]

        self.hypers = [ffn(f"mask_decoder.output_hypernetworks_mlps.{m}.") for m in range(4)]
        self.iou_head = ffn("mask_decoder.iou_prediction_head.")

    # ---- helpers ---------------------------------------------------------------------------------------------
    def _plan(self, precision):
        """the plan object of `precision` (None: this decoder's default)"""
        precision = precision or self.precision
        if precision not in self._plans:
            raise ValueError(f"precision {precision!r}: expected 'exact' or 'f16'")
        return self._plans[precision]

    def _x3(self, name):
        """(x3 weight f16 [N, 3K], shifted bias f32 [N], row scale f32 [N]) of the exact plan's Linear `name`, built on first use: W as
        [whi | whi/2048 | wlo] rows pre-scaled by powers of two (lmx.exact.split_rows_x3), the bias shifted along."""
        from .exact import split_rows_x3

        if name not in self._wx:
            w, b = linear_f32(self._sd, name)
            x3, sc, e = split_rows_x3(w, [w.shape[1]])
            dev = self.device
            self._wx[name] = (torch.from_numpy(x3).to(dev), torch.from_numpy(np.ldexp(b.astype(np.float32), e).astype(np.float32)).to(dev),
                              torch.from_numpy(sc).to(dev))
        return self._wx[name]

    @staticmethod
    def _attn(P, p, q_in, k_in, v_in, n, tq, tk, res):
        """SamAttention: q/k/v projections, attention over 8 heads, out projection (+res) in f32."""
        q = P.linear(q_in, p + "q_proj")
        k = P.linear(k_in, p + "k_proj")
        v = P.linear(v_in, p + "v_proj")
        return P.linear(P.attention(q, k, v, n, tq, tk), p + "out_proj", res=res, out_dtype=torch.float32)

    @staticmethod
    def _ffn(P, p, x):
        h = P.linear(x, p + "proj_in", act=K.ACT_RELU)
        h = P.linear(h, p + "layers.0", act=K.ACT_RELU)
        return P.linear(h, p + "proj_out", out_dtype=torch.float32)

    # ---- forward ---------------------------------------------------------------------------------------------
    def lowres(self, emb, sparse, keys=None, masks=None, precision=None):
        """emb f16/f32 [n*G*G, 256] (NHWC rows), sparse f32 [n,Ns,256] -> (logits f32 [n,4G,4G] of mask 0, iou f32 [n]).
        keys: f32 [n*G*G,256] = emb + the dense prompt of a mask input (lmx_k_mask_embed); None = emb + the no-mask embedding.
        masks: a tuple of mask indices to decode -> (logits f32 [n,len(masks),4G,4G], iou f32 [n,4]); None = mask 0 as above.
        precision: the plan (constructor docstring; None = this decoder's default).  One walk serves both
        (TF:models/sam/modeling_sam.py:432-543): a plan says how an activation becomes a GEMM operand and where the upscaler's
        two GELUs sit."""
        P = self._plan(precision)
        n = sparse.shape[0]
        T, Pn = 5 + sparse.shape[1], self.G * self.G
        sel = (0,) if masks is None else tuple(masks)
        eps = 1e-6
        f32 = torch.float32
        tokens = torch.cat([self.out_tokens[None].expand(n, -1, -1), sparse], dim=1).reshape(n * T, D).contiguous()
        if keys is None:
            keys = K.add_bcast(emb, self.no_mask)             # image embedding + dense no-mask embedding, f32
        queries, qpe = tokens, tokens
        for i, L in enumerate(self.layers):
            p = f"mask_decoder.transformer.layers.{i}."
            if i == 0:
                q_ = P.operand(queries)
                queries = self._attn(P, p + "self_attn.", q_, q_, q_, n, T, T, None)
            else:
                q_ = P.operand(queries, qpe)
                queries = self._attn(P, p + "self_attn.", q_, q_, P.operand(queries), n, T, T, queries)
            queries = K.layernorm(queries, *L["ln1"], eps, out_dtype=f32)
            q_ = P.operand(queries, qpe)
            k_ = P.operand(keys, self.key_pe)
            queries = self._attn(P, p + "cross_attn_token_to_image.", q_, k_, P.operand(keys), n, T, Pn, queries)
            queries = K.layernorm(queries, *L["ln2"], eps, out_dtype=f32)
            h = P.linear(P.operand(queries), p + "mlp.lin1", act=K.ACT_RELU)
            queries = P.linear(h, p + "mlp.lin2", res=queries, out_dtype=f32)
            queries = K.layernorm(queries, *L["ln3"], eps, out_dtype=f32)
            q_ = P.operand(queries, qpe)
            # (keys have not changed since the token-to-image attention above: k_ is still keys + key_pe)
            keys = self._attn(P, p + "cross_attn_image_to_token.", k_, q_, P.operand(queries), n, Pn, T, keys)
            keys = K.layernorm(keys, *L["ln4"], eps, out_dtype=f32)
        q_ = P.operand(queries, qpe)
        k_ = P.operand(keys, self.key_pe)
        v_ = P.operand(keys)  # the final attention's values and the upscaler's input
        queries = self._attn(P, "mask_decoder.transformer.final_attn_token_to_image.", q_, k_, v_, n, T, Pn, queries)
        queries = K.layernorm(queries, *self.ln_final, 1e-5, out_dtype=f32)
        q3 = queries.view(n, T, D)
        iou_tok = P.operand(q3[:, 0].contiguous())

        def hyper():  # f32 [n,M,32]
            hs = [self._ffn(P, f"mask_decoder.output_hypernetworks_mlps.{m}.", P.operand(q3[:, 1 + m].contiguous())) for m in sel]
            return hs[0][:, None] if len(hs) == 1 else torch.stack(hs, 1)

        # upscaler: ConvTranspose2d(k2, s2) as per-pixel GEMMs, LayerNorm2d row-wise on the [.., quadrant, 64] view, the pixel
        # shuffle deferred to the hyper-network dot product
        logits = P.upscale_and_mask(v_, hyper, n)
        iou = self._ffn(P, "mask_decoder.iou_prediction_head.", iou_tok)                                # f32 [n,4]
        return (logits[:, 0], iou[:, 0]) if masks is None else (logits, iou)

    def predict(self, emb, boxes, frame_hw, resized_hw, precision=None):
        """emb [n*G*G,256] rows of the NHWC image embedding; boxes f32 [n,>=4] device, xyxy in FRAME pixels.
        precision: None = this decoder's default plan, "exact" or "f16" (constructor docstring)."""
        h, w = frame_hw
        nh, nw = resized_hw
        sparse = K.prompt_box(boxes, nw / w, nh / h, float(self.S), self.gauss, self.corner)
        logits, iou = self.lowres(emb, sparse, precision=precision)
        mask, stats = K.mask_post(logits, self.S, nh, nw, h, w)
        return dict(mask=mask, stats=stats, iou=iou, lowres=logits)

    def decode_lowres(self, emb, frame_hw, resized_hw, points=None, labels=None, boxes=None, mask_input=None, multimask=False,
                      precision=None, input_frame=False):
        """The prompt encoder and mask decoder of decode() without the post-processing -> (lowres f32 [n,C,4G,4G], iou f32
        [n,C]).  emb holds n*G*G rows (one image per prompt set) or G*G rows: ONE image embedding that serves all n prompt
        sets (SamPredictor.predict_torch's batch of prompts; every prompt gets the keys of that embedding, so prompt i
        decodes to the bits it gets alone).  input_frame: points / boxes are already in the resized input frame (predict_torch's
        convention: scale 1 in lmx_k_prompt_points) instead of frame pixels."""
        h, w = frame_hw
        nh, nw = resized_hw
        if points is None and boxes is None:
            raise ValueError("decode needs points (with labels) or boxes")
        if (points is None) != (labels is None):
            raise ValueError("points and labels go together")
        self._plan(precision)
        sx, sy = (1.0, 1.0) if input_frame else (nw / w, nh / h)
        sparse = K.prompt_points(points, labels, boxes, sx, sy, float(self.S), self.gauss, self.point_embed, self.not_a_point,
                                 self.corner)
        n, P = sparse.shape[0], self.G * self.G
        if emb.shape[0] == P and n > 1:
            emb = emb.repeat(n, 1)  # one image, n prompt sets
        elif emb.shape[0] != n * P:
            raise ValueError(f"emb has {emb.shape[0]} rows: expected {P} (one image) or {n * P} ({n} images)")
        keys = None
        if mask_input is not None:
            if self.mask_params is None:
                raise ValueError("mask_input needs the prompt_encoder.mask_embed.* weights (mask_embed_param_spec()), which this "
                                 "decoder's state dict does not hold")
            keys = K.mask_embed(mask_input, emb, self.mask_params, self.G)
        sel = (1, 2, 3) if multimask else (0,)
        logits, iou = self.lowres(emb, sparse, keys=keys, masks=sel, precision=precision)
        return logits, iou[:, sel[0]:sel[-1] + 1]

    def decode(self, emb, frame_hw, resized_hw, points=None, labels=None, boxes=None, mask_input=None, multimask=False,
               return_logits=False, precision=None, input_frame=False):
        """SamPredictor.predict_torch for n prompt sets (all share Np and whether a box / a mask is given), against n image
        embeddings or one (decode_lowres).  emb [n*G*G,256] or [G*G,256] rows; points f32 [n,Np,2] with labels int32 [n,Np]
        (1 / 0 / -1), boxes f32 [n,>=4], all device tensors in FRAME pixels (in the resized input frame with input_frame);
        mask_input f32 [n,4G,4G] (an earlier call's low-res logits).  Labels outside {-1,0,1} give NaN tokens
        (LmxSamPredictor checks them on the host).
        -> dict(iou f32 [n,C], lowres f32 [n,C,4G,4G], and mask u8 [n,C,h,w] + stats int64 [n,C,8] or, with return_logits,
        logits f32 [n,C,h,w]); C = 3 (masks 1..3) with multimask, else 1 (mask 0)."""
        h, w = frame_hw
        nh, nw = resized_hw
        logits, iou = self.decode_lowres(emb, frame_hw, resized_hw, points=points, labels=labels, boxes=boxes, mask_input=mask_input,
                                         multimask=multimask, precision=precision, input_frame=input_frame)
        n, C, L, _ = logits.shape
        out = dict(iou=iou, lowres=logits)
        flat = logits.view(n * C, L, L)
        if return_logits:
            out["logits"] = K.mask_logits(flat, self.S, nh, nw, h, w).view(n, C, h, w)
        else:
            mask, stats = K.mask_post(flat, self.S, nh, nw, h, w)
            out["mask"], out["stats"] = mask.view(n, C, h, w), stats.view(n, C, 8)
        return out
