"""The model-level C entry points (include/lmx.h, "MODEL level"; csrc/dino_model.hip, csrc/yolo_model.hip) seen from Python.

``write_image`` writes the weight-image container (csrc/image.h has the layout): one little-endian file holding a model's config
block and its tensors bit for bit in their final device form.  ``write_dino_image`` exports a loaded ``DinoEmbedder`` that way
(csrc/dino_image.h has its config block).  A C program opens it with ``lmx_dino_open_host`` and asks ``lmx_dino_embed`` /
``lmx_dino_embed_host`` for embeddings without Python (examples/dino_embed.c).

``NativeDino`` is the thin binding of that handle.  No plan logic lives here: the launch sequence is C++, and it is the launch
sequence of ``DinoEmbedder.embed_frames`` — same entry points, same descriptors, same bits (tests/test_gpu_native_dino.py).
The host table functions (``lmx_h_pil_tables``, ``lmx_h_aa_tables``, ...) are bound too, for the tests that hold them to
lmx/resample.py.

``write_yolo_image`` / ``NativeYolo`` are the same for a ``YoloDetector`` (csrc/yolo_model.hip, csrc/yolo_image.h,
examples/yolo_detect.c): the launch sequence of ``YoloDetector.detect`` / ``detect_pose`` on either precision plan, with the twins of
lmx/letterbox.py and ``kernels.split_k_for`` (``lmx_h_letterbox_geometry``, ``lmx_h_letterbox_tables``, ``lmx_h_conv_split_k``)
bound for the tests (tests/test_native_yolo_host.py, tests/test_gpu_native_yolo.py).

``write_sam_image`` / ``NativeSam`` are the same for a ``SamVitEncoder`` with a ``MaskDecoder`` (csrc/sam_model.hip, csrc/sam_image.h,
examples/sam_segment.c): the launch sequence of ``SamVitEncoder.encode`` and ``MaskDecoder.predict`` for one box per frame on either
precision plan, followed by ``kernels.pack_bits`` / ``kernels.contour_features`` where asked for (tests/test_native_sam_host.py,
tests/test_gpu_native_sam.py).  What the handles share on the C side (csrc/model_handle.h) they share here: ``_NativeHandle``."""
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib, letterbox, resample
from ._lib import DinoInfo, FusedInfo, GfmInfo, GnnInfo, LetterboxGeo, LmxError, RecordLayout, SamInfo, TcnInfo, XfmInfo, YoloInfo, check

MAGIC = b"LMXIMAGE"
VERSION = 1
KIND_DINO, KIND_YOLO, KIND_SAM, KIND_TCN, KIND_XFM, KIND_GFM, KIND_GNN = 1, 2, 3, 4, 5, 6, 7
HEADER_BYTES, ENTRY_BYTES, NAME_BYTES = 48, 88, 48
ARCH = {"dinov2": 0, "dinov3": 1}
RECIPE = {"pil": 0, "float": 1}
FILT = {resample.BILINEAR: 2, resample.BICUBIC: 3}  # Pillow's `resample` codes (LMX_FILT_*)
_DTYPE = {np.dtype(np.float16): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}
PLANS = {"f16": 0, "exact": 1}  # LMX_YOLO_F16, LMX_YOLO_EXACT; an image's plan mask has bit (1 << code) per plan it holds
LAYER_TENSORS = ("g1", "b1", "wqkv", "bqkv", "wo", "bo", "ls1", "g2", "b2", "w1", "bb1", "w2", "bb2", "ls2")


def host(t):
    """A tensor of any device as the contiguous numpy array an image stores."""
    return np.ascontiguousarray(t.detach().cpu().numpy())


def dino_config_block(embedder):
    """The fixed config block of a DINO image: 20 int32 then 8 float64 (LmxDinoCfg, csrc/dino_image.h)."""
    cfg, rc = embedder.cfg, embedder.recipe
    size_h, size_w = rc.size_hw if rc.size_hw is not None else (0, 0)
    ints = (ARCH[cfg.arch], cfg.hidden, cfg.heads, cfg.layers, cfg.mlp, int(cfg.gated), cfg.patch, cfg.image, cfg.grid, cfg.n_prefix,
            cfg.tokens, embedder.k_pad, int(embedder.pos is not None), int(embedder.rope is not None), RECIPE[rc.kind], FILT[rc.filt],
            (rc.shortest_edge or 0) if rc.size_hw is None else 0, size_h, size_w, rc.crop or 0)
    return struct.pack("<20i8d", *ints, cfg.eps, rc.rescale, *rc.mean, *rc.std)


def dino_tensors(embedder):
    """Ordered {name: numpy array}: exactly the tensors the embedder holds, in its dtypes."""
    e = embedder
    out = {"pe_w": host(e.pe_w), "pe_b": host(e.pe_b), "prefix": host(e.prefix)}
    if e.pos is not None:
        out["pos"] = host(e.pos)
    if e.rope is not None:
        out["rope_cos"], out["rope_sin"] = host(e.rope[0]), host(e.rope[1])
    for i, L in enumerate(e.layers):
        for n in LAYER_TENSORS:
            out[f"layer.{i}.{n}"] = host(L[n])
    out["gf"], out["bf"], out["lut"] = host(e.gf), host(e.bf), host(e.lut)
    return out


def write_image(path, kind, config_block, tensors):
    """header | config block | directory | data (64-byte aligned tensors).  Returns the file's size."""
    n = len(tensors)
    dir_offset = HEADER_BYTES + len(config_block)
    data_offset = (dir_offset + n * ENTRY_BYTES + 63) // 64 * 64
    entries, off = [], data_offset
    for name, a in tensors.items():
        raw = name.encode()
        if len(raw) >= NAME_BYTES or a.dtype not in _DTYPE or not 1 <= a.ndim <= 4:
            raise LmxError(f"write_image: tensor {name!r} ({a.dtype}, rank {a.ndim}) does not fit a directory entry")
        shape = tuple(a.shape) + (0,) * (4 - a.ndim)
        entries.append(struct.pack(f"<{NAME_BYTES}sII4iQQ", raw, _DTYPE[a.dtype], a.ndim, *shape, off, a.nbytes))
        off = (off + a.nbytes + 63) // 64 * 64
    file_bytes = off
    with open(path, "wb") as f:
        f.write(struct.pack("<8sIIIIQQQ", MAGIC, VERSION, kind, len(config_block), n, dir_offset, data_offset, file_bytes))
        f.write(config_block)
        f.write(b"".join(entries))
        for a in tensors.values():
            f.write(b"\0" * (-f.tell() % 64))
            f.write(a.tobytes())
        f.write(b"\0" * (file_bytes - f.tell()))
    return file_bytes


def _check_image(Info, fn_name, path):
    """lmx_<kind>_image_check_host: validate an image on the host (no GPU) -> its info struct; LmxError names the offending field."""
    info = Info()
    check(getattr(_lib.load(), fn_name)(str(path).encode(), C.byref(info)), fn_name)
    return info


def write_dino_image(embedder, path):
    """Export a DinoEmbedder (any device) as the weight image lmx_dino_open_host reads.  Returns the file's size in bytes."""
    return write_image(path, KIND_DINO, dino_config_block(embedder), dino_tensors(embedder))


def check_dino_image(path):
    """lmx_dino_image_check_host: validate an image on the host (no GPU) -> DinoInfo; LmxError names the offending field."""
    return _check_image(DinoInfo, "lmx_dino_image_check_host", path)


# ---- the TCN weight image (csrc/tcn_image.h) ----------------------------------------------------------------------------------
def tcn_config_block(cfg):
    """12 int32 (input_dim, n_blocks, k, head, channels[8]) then the dropout probability as one float64."""
    ch = tuple(cfg.channels) + (0,) * (8 - len(cfg.channels))
    return struct.pack("<12id", cfg.input_dim, len(cfg.channels), cfg.kernel_size, cfg.head, *ch, cfg.dropout)


def write_tcn_image(cfg, folded, path):
    """Export a TCN (lmx.checkpoints.tcn_from_state_dict's configuration and folded weights) as the weight image lmx_tcn_open_host
    reads: the tensors in the kernel's operand order (lmx.tcn.pack_tensors).  Returns the file's size in bytes."""
    from . import tcn

    return write_image(path, KIND_TCN, tcn_config_block(cfg.validate("write_tcn_image")), tcn.pack_tensors(cfg, folded))


def check_tcn_image(path):
    """lmx_tcn_image_check_host: validate an image on the host (no GPU) -> TcnInfo; LmxError names the offending field."""
    return _check_image(TcnInfo, "lmx_tcn_image_check_host", path)


# ---- the gait transformer's weight image (csrc/xfm_image.h) ------------------------------------------------------------------------
def xfm_config_block(cfg):
    """8 int32 (input_dim, d_model, n_heads, n_layers, ff, head, max_len, 0) then the dropout probability as one float64."""
    return struct.pack("<8id", cfg.input_dim, cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.ff, cfg.head, cfg.max_len, 0, cfg.dropout)


def write_xfm_image(cfg, weights, path):
    """Export a gait transformer (lmx.checkpoints.xfm_from_state_dict's configuration and weights) as the weight image
    lmx_xfm_open_host reads: the tensors in the kernel's operand order (lmx.xfm.pack_tensors).  Returns the file's size in bytes."""
    from . import xfm

    return write_image(path, KIND_XFM, xfm_config_block(cfg.validate("write_xfm_image")), xfm.pack_tensors(cfg, weights))


def check_xfm_image(path):
    """lmx_xfm_image_check_host: validate an image on the host (no GPU) -> XfmInfo; LmxError names the offending field."""
    return _check_image(XfmInfo, "lmx_xfm_image_check_host", path)


# ---- GraphGPS' weight image (csrc/gnn_image.h) ---------------------------------------------------------------------------------------
def gnn_config_block(cfg):
    """8 int32 (input_dim, d_model, n_heads, n_layers, pe_dim, ff, edge_dim, 0) then the dropout probability as one float64."""
    return struct.pack("<8id", *cfg.shape(), 0, cfg.dropout)


def write_gnn_image(cfg, weights, path):
    """Export the live network of GraphGPS (lmx.checkpoints.gnn_from_state_dict's configuration and weights) as the weight image
    lmx_gnn_open_host reads: the tensors of lmx.gnn.pack_tensors under the names of lmx_gnn_weights_t's fields.  Returns the file's size."""
    from . import gnn

    return write_image(path, KIND_GNN, gnn_config_block(cfg.validate("write_gnn_image")), gnn.pack_tensors(cfg, weights))


def check_gnn_image(path):
    """lmx_gnn_image_check_host: validate an image on the host (no GPU) -> GnnInfo; LmxError names the offending field."""
    return _check_image(GnnInfo, "lmx_gnn_image_check_host", path)


# ---- the graph transformer's weight image (csrc/gfm_image.h) -----------------------------------------------------------------------
def gfm_config_block(cfg):
    """8 int32 (input_dim, d_model, n_heads, n_layers, ff, edge_dim, max_degree, max_spd) then the dropout probability as one float64."""
    return struct.pack("<8id", *cfg.shape(), cfg.dropout)


def write_gfm_image(cfg, weights, path):
    """Export a graph transformer (lmx.checkpoints.gfm_from_state_dict's configuration and weights) as the weight image
    lmx_gfm_open_host reads: the tensors of lmx.gfm.pack_tensors under the names of lmx_gfm_weights_t's fields.  Returns the file's size."""
    from . import gfm

    return write_image(path, KIND_GFM, gfm_config_block(cfg.validate("write_gfm_image")), gfm.pack_tensors(cfg, weights))


def check_gfm_image(path):
    """lmx_gfm_image_check_host: validate an image on the host (no GPU) -> GfmInfo; LmxError names the offending field."""
    return _check_image(GfmInfo, "lmx_gfm_image_check_host", path)


# ---- the YOLO weight image (csrc/yolo_image.h) ------------------------------------------------------------------------------
def yolo_conv_groups(detector):
    """{name of a 1 x 1 convolution: the channel groups its exact-plan weight is split over}: what YoloDetector.forward_letterboxed
    passes to _PlanExact._w at each call site (a C2f cv1 that reads a concat, every C2f cv2, SPPF cv2); absent = one group (the
    Detect / Pose heads, the other cv1) or a 3 x 3 convolution (9 x [Cin], _PlanExact._w's own rule)."""
    T = detector.table
    c_out = [m.get("c2", 0) for m in T]
    cat = {12: [c_out[9], c_out[6]], 15: [c_out[12], c_out[4]], 18: [c_out[16], c_out[12]], 21: [c_out[19], c_out[9]]}
    groups = {}
    for i, m in enumerate(T):
        if m["kind"] == "c2f":
            if i in cat:
                groups[f"model.{i}.cv1"] = cat[i]
            groups[f"model.{i}.cv2"] = [m["c2"] // 2] * (2 + m["n"])
        elif m["kind"] == "sppf":
            groups[f"model.{i}.cv2"] = [m["c1"] // 2] * 4
    return groups


def yolo_config_block(detector, plans):
    """10 int32 (LmxYoloCfg, csrc/yolo_image.h), then the class names: NUL-terminated UTF-8 in class order, zero-padded to 8 bytes."""
    cfg = detector.cfg
    k, ndim = cfg.kpt_shape if cfg.kpt_shape is not None else (0, 0)
    names = [detector.names[i] for i in range(len(detector.names))]
    blob = b"".join(n.encode("utf-8") + b"\0" for n in names)
    if any(b"\0" in n.encode("utf-8") for n in names):
        raise LmxError("write_yolo_image: a class name contains a NUL character")
    mask = sum(1 << PLANS[p] for p in set(plans))
    ints = (ord(cfg.scale), cfg.nc, detector.nc_pad, cfg.imgsz, k, ndim, getattr(detector, "nk_pad", 0) if k else 0, mask, len(names), len(blob))
    return struct.pack("<10i", *ints) + blob + b"\0" * (-len(blob) % 8)


def yolo_tensors(detector, plans):
    """Ordered {name: numpy array}: the stem, then per convolution of detector.w the f16 plan's (w, b) and / or the exact plan's
    (x3 weight, ldexp'd bias, row scale) — exactly the tensors the detector's plans hold, in their dtypes."""
    out = {"stem.w": host(detector.w["model.0"][0]), "stem.b": host(detector.w["model.0"][1])}
    groups = yolo_conv_groups(detector)
    exact = detector._plan("exact") if "exact" in plans else None
    for name, (w, b) in detector.w.items():
        if name == "model.0":
            continue
        if "f16" in plans:
            out[f"f16.{name}.w"], out[f"f16.{name}.b"] = host(w), host(b)
        if exact is not None:
            x3, xb, sc = exact._w(name, groups.get(name))
            out[f"x3.{name}.w"], out[f"x3.{name}.b"], out[f"x3.{name}.s"] = host(x3), host(xb), host(sc)
    return out


def write_yolo_image(detector, path, plans=("f16", "exact")):
    """Export a YoloDetector (any device) as the weight image lmx_yolo_open_host reads, with the tensors of `plans`.  Returns the
    file's size in bytes."""
    plans = tuple(plans)
    if not plans or any(p not in PLANS for p in plans):
        raise LmxError(f"write_yolo_image: plans {plans!r}: a non-empty subset of {tuple(PLANS)}")
    return write_image(path, KIND_YOLO, yolo_config_block(detector, plans), yolo_tensors(detector, plans))


def check_yolo_image(path):
    """lmx_yolo_image_check_host: validate an image on the host (no GPU) -> YoloInfo; LmxError names the offending field or tensor."""
    return _check_image(YoloInfo, "lmx_yolo_image_check_host", path)


# ---- the SAM weight image (csrc/sam_image.h) -------------------------------------------------------------------------------
SAM_ENC_VIT, SAM_ENC_HIERA = 0, 2  # LMX_SAM_ENC_*: the config block's `encoder` field (1 is no encoder's)
_SAM_ATTN = {"sa": "self_attn", "t2i": "cross_attn_token_to_image", "i2t": "cross_attn_image_to_token"}
_SAM_PROJ = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "out_proj"}
_SAM_FFN = {"in": "proj_in", "mid": "layers.0", "out": "proj_out"}


def sam_decoder_linears():
    """Ordered {short name in the image: parameter prefix in the state dict}: every Linear MaskDecoder.lowres touches
    for a box prompt with one mask (mask token 0), in the order of csrc/host_sam_image.cpp lmx_sam_linears().  up1 / up2 are the two
    ConvTranspose2d re-laid as per-pixel GEMMs."""
    out = {}
    t = "mask_decoder.transformer."
    for i in range(2):
        p = f"{t}layers.{i}."
        for a in ("sa", "t2i"):
            for k, v in _SAM_PROJ.items():
                out[f"L{i}.{a}.{k}"] = f"{p}{_SAM_ATTN[a]}.{v}"
        out[f"L{i}.lin1"], out[f"L{i}.lin2"] = p + "mlp.lin1", p + "mlp.lin2"
        for k, v in _SAM_PROJ.items():
            out[f"L{i}.i2t.{k}"] = f"{p}{_SAM_ATTN['i2t']}.{v}"
    for k, v in _SAM_PROJ.items():
        out[f"fin.{k}"] = f"{t}final_attn_token_to_image.{v}"
    out["up1"], out["up2"] = "mask_decoder.upscale_conv1", "mask_decoder.upscale_conv2"
    for k, v in _SAM_FFN.items():
        out[f"hyp0.{k}"] = f"mask_decoder.output_hypernetworks_mlps.0.{v}"
    for k, v in _SAM_FFN.items():
        out[f"iou.{k}"] = f"mask_decoder.iou_prediction_head.{v}"
    return out


def _sam_plans(plans, who):
    plans = tuple(plans)
    if not plans or any(p not in PLANS for p in plans):
        raise LmxError(f"{who}: plans {plans!r}: a non-empty subset of {tuple(PLANS)}")
    return plans


def sam_config_block(encoder, plans=("f16", "exact")):
    """12 int32 (LmxSamCfg, csrc/sam_image.h), eps as float64, then the global-attention layer indices as int32, zero-padded to 8 bytes."""
    cfg = encoder.cfg
    gidx = sorted(int(i) for i in cfg.global_idx)
    mask = sum(1 << PLANS[p] for p in set(_sam_plans(plans, "sam_config_block")))
    ints = (SAM_ENC_VIT, cfg.hidden, cfg.heads, cfg.layers, cfg.mlp, cfg.window, cfg.patch, cfg.image, cfg.out_ch, mask, len(gidx), 0)
    tail = struct.pack(f"<{len(gidx)}i", *gidx)
    return struct.pack("<12id", *ints, float(cfg.eps)) + tail + b"\0" * (-len(tail) % 8)


def _sam_decoder_tensors(d, plans):
    """The prompt encoder's and the mask decoder's entries of a SAM image, the same behind either encoder."""
    out = {}
    out.update({"dec.gauss": host(d.gauss), "dec.corner": host(d.corner), "dec.key_pe": host(d.key_pe), "dec.no_mask": host(d.no_mask),
                "dec.out_tokens": host(d.out_tokens), "dec.point_embed": host(d.point_embed), "dec.not_a_point": host(d.not_a_point)})
    if d.mask_params is not None:
        out["dec.mask_params"] = host(d.mask_params)
    for i, L in enumerate(d.layers):
        for j in range(1, 5):
            out[f"dec.L{i}.ln{j}.g"], out[f"dec.L{i}.ln{j}.b"] = host(L[f"ln{j}"][0]), host(L[f"ln{j}"][1])
    out["dec.ln_final.g"], out["dec.ln_final.b"] = host(d.ln_final[0]), host(d.ln_final[1])
    out["dec.up_ln.g"], out["dec.up_ln.b"] = host(d.up_ln[0]), host(d.up_ln[1])
    for short, prefix in sam_decoder_linears().items():
        if "f16" in plans:
            out[f"dec.f16.{short}.w"], out[f"dec.f16.{short}.b"] = (host(t) for t in d._w16[prefix])
        if "exact" in plans:
            out[f"dec.x3.{short}.w"], out[f"dec.x3.{short}.b"], out[f"dec.x3.{short}.s"] = (host(t) for t in d._x3(prefix))
    return out


def _is_hiera(encoder):
    from .sam import HieraEncoder

    return isinstance(encoder, HieraEncoder)


def _hiera_exportable(encoder, who):
    """The C side plans and runs the default encoder only: the packed operands depend on these choices."""
    from . import kernels as K

    if not encoder.fused_mlp:
        raise ValueError(f"{who}: the encoder was built with fused_mlp false (or LMX_NO_FUSED_MLP): its blocks hold no packed MLP images and its "
                         "attn8 operands are packed for another kernel form; the C plan is the default encoder's")
    if not encoder.proj_ln:
        raise ValueError(f"{who}: the encoder has proj_ln false; the C plan is the default encoder's, whose stage-3 projections write layer_norm2")
    if tuple(K.FUSED_MLP_WIDTHS) != (112, 224):
        raise ValueError(f"{who}: FUSED_MLP_WIDTHS is {tuple(K.FUSED_MLP_WIDTHS)} (LMX_MLP448 is set); the C plan is the default encoder's, (112, 224)")


def sam_hiera_config_block(encoder, plans=("f16", "exact")):
    """The config block of a SAM image whose encoder is Hiera (csrc/sam_image.h): 12 int32, eps as float64, then blocks / dims / heads /
    windows per stage, the global blocks (ascending) and fpn_top_down as int32, zero-padded to 8 bytes — all of HieraConfig."""
    cfg = encoder.cfg
    mask = sum(1 << PLANS[p] for p in set(_sam_plans(plans, "sam_hiera_config_block")))
    ns = len(cfg.blocks)
    if not len(cfg.dims) == len(cfg.heads) == len(cfg.windows) == ns or len(cfg.pos_bkg) != 2:
        raise LmxError(f"sam_hiera_config_block: blocks, dims, heads and windows of {cfg!r} are not one entry per stage")
    gb = sorted(int(i) for i in cfg.global_blocks)
    ints = (SAM_ENC_HIERA, cfg.hidden, ns, sum(cfg.blocks), len(gb), len(cfg.fpn_top_down), cfg.q_pool_stages, cfg.image, cfg.fpn_dim, mask, *cfg.pos_bkg)
    tail = (*cfg.blocks, *cfg.dims, *cfg.heads, *cfg.windows, *gb, *cfg.fpn_top_down)
    raw = struct.pack(f"<{len(tail)}i", *(int(v) for v in tail))
    return struct.pack("<12id", *(int(v) for v in ints), float(cfg.eps)) + raw + b"\0" * (-len(raw) % 8)


HIERA_BLOCK_TENSORS = ("g1", "b1", "wqkv", "bqkv", "padkv", "wo", "bo", "g2", "b2", "w1", "bb1", "w2", "bb2")


def sam_hiera_tensors(encoder, decoder, plans=("f16", "exact")):
    """Ordered {name: numpy array}: what a HieraEncoder holds on the device, as it holds it — the packed attention and MLP images
    included, so that no packing is restated in C++ — with the neck levels outputs="embedding" reads, then the decoder's entries for
    `plans` (the trunk has one plan)."""
    plans = _sam_plans(plans, "sam_hiera_tensors")
    e = encoder
    _hiera_exportable(e, "sam_hiera_tensors")
    out = {"enc.pe_w": host(e.pe_w), "enc.pe_b": host(e.pe_b), "enc.pos": host(e.pos), "enc.lut": host(e.lut)}
    for i, B in enumerate(e.blocks):
        p = f"enc.B{i}."
        for n in HIERA_BLOCK_TENSORS + (("wp", "bp") if "wp" in B else ()):
            out[p + n] = host(B[n])
        for key in ("attn", "mlp_img"):
            for j, t in enumerate(B.get(key, ())):
                out[f"{p}{key}.{j}"] = host(t)
    for s in range(2, len(e.neck)):
        out[f"enc.neck.{s}.w"], out[f"enc.neck.{s}.b"] = host(e.neck[s][0]), host(e.neck[s][1])
    out.update(_sam_decoder_tensors(decoder, plans))
    return out


def sam_tensors(encoder, decoder, plans=("f16", "exact")):
    """Ordered {name: numpy array}: what SamVitEncoder and MaskDecoder hold on the device, in final device form, for `plans`.  The
    tensors both build lazily under the exact plan — the encoder's [whi | wlo] weights (_split2) with the two halves of the neck's
    3 x 3, the decoder's x3 weight / shifted bias / scale triples (_lin) — are built here eagerly, for every layer of
    sam_decoder_linears()."""
    plans = _sam_plans(plans, "sam_tensors")
    e, d = encoder, decoder
    out = {"enc.pe_b": host(e.pe_b), "enc.pos": host(e.pos), "enc.lut": host(e.lut)}
    if "f16" in plans:
        out["enc.pe_w"] = host(e.pe_w)
    if "exact" in plans:
        out["enc.x2.pe"] = host(e._split2("pe"))
    for i, L in enumerate(e.layers):
        p = f"enc.L{i}."
        for n in ("g1", "b1", "bqkv", "padkv", "rh", "rw", "bo", "g2", "b2", "bb1", "bb2"):
            out[p + n] = host(L[n])
        if "f16" in plans:
            for n in ("wqkv", "wo", "w1", "w2"):
                out[p + n] = host(L[n])
        if "exact" in plans:
            for n in ("qkv", "proj", "fc1", "fc2"):
                out[f"enc.x2.L{i}.{n}"] = host(e._split2(f"{i}.{n}"))
    out["enc.n1.g"], out["enc.n1.b"] = host(e.n1_ln[0]), host(e.n1_ln[1])
    out["enc.n2.g"], out["enc.n2.b"] = host(e.n2_ln[0]), host(e.n2_ln[1])
    if "f16" in plans:
        out["enc.n1.w"], out["enc.n2.w"] = host(e.n1_w), host(e.n2_w)
    if "exact" in plans:
        out["enc.x2.n1"] = host(e._split2("n1"))
        w2 = host(e._split2("n2"))
        kc = w2.shape[1] // 2
        out["enc.x2.n2.hi"], out["enc.x2.n2.lo"] = np.ascontiguousarray(w2[:, :kc]), np.ascontiguousarray(w2[:, kc:])
    out.update(_sam_decoder_tensors(d, plans))
    return out


def write_sam_image(encoder, decoder, path, plans=("f16", "exact")):
    """Export a SamVitEncoder with its MaskDecoder (any device) as the weight image lmx_sam_open_host reads, with the tensors of
    `plans`.  Returns the file's size in bytes.
    A HieraEncoder is exported too (csrc/sam_image.h; `plans` then names the decoder plans, the trunk has one); ValueError for an
    encoder not built the default way (fused_mlp,
    proj_ln, FUSED_MLP_WIDTHS), whatever its `band` setting, which changes no bit and is not recorded."""
    plans = _sam_plans(plans, "write_sam_image")
    cfg = encoder.cfg
    if _is_hiera(encoder):
        _hiera_exportable(encoder, "write_sam_image")
        if (decoder.S, decoder.G) != (cfg.image, cfg.image // 16) or cfg.fpn_dim != 256:
            raise LmxError(f"write_sam_image: a decoder for image {decoder.S} / grid {decoder.G} does not read the {cfg.fpn_dim}-channel embedding "
                           f"of a Hiera encoder with image {cfg.image} / grid {cfg.image // 16}")
        return write_image(path, KIND_SAM, sam_hiera_config_block(encoder, plans), sam_hiera_tensors(encoder, decoder, plans))
    if (decoder.S, decoder.G) != (cfg.image, cfg.grid) or cfg.out_ch != 256:
        raise LmxError(f"write_sam_image: a decoder for image {decoder.S} / grid {decoder.G} does not read the {cfg.out_ch}-channel embedding "
                       f"of an encoder with image {cfg.image} / grid {cfg.grid}")
    return write_image(path, KIND_SAM, sam_config_block(encoder, plans), sam_tensors(encoder, decoder, plans))


def check_sam_image(path):
    """lmx_sam_image_check_host: validate an image on the host (no GPU) -> SamInfo; LmxError names the offending field or tensor."""
    return _check_image(SamInfo, "lmx_sam_image_check_host", path)


# ---- the host arithmetic of the YOLO predictor (csrc/host_letterbox.cpp) -------------------------------------------------------
def letterbox_geometry(sh, sw, imgsz=640, stride=32, auto=True):
    """lmx_h_letterbox_geometry: the C++ twin of letterbox.geometry, same return value."""
    g = LetterboxGeo()
    check(_lib.load().lmx_h_letterbox_geometry(sh, sw, imgsz, stride, 1 if auto else 0, C.byref(g)), "lmx_h_letterbox_geometry")
    return letterbox.LetterboxGeo(g.sh, g.sw, g.rh, g.rw, g.top, g.left, g.oh, g.ow, g.gain, g.pad_x, g.pad_y)


def letterbox_tables(sh, sw, rh, rw):
    """lmx_h_letterbox_tables: the C++ twin of letterbox.resize_tables, same return value."""
    xofs, ialpha = np.empty(rw, np.int32), np.empty(rw * 2, np.int16)
    yofs, ibeta = np.empty(rh, np.int32), np.empty(rh * 2, np.int16)
    check(_lib.load().lmx_h_letterbox_tables(sh, sw, rh, rw, xofs.ctypes.data, ialpha.ctypes.data, yofs.ctypes.data, ibeta.ctypes.data),
          "lmx_h_letterbox_tables")
    return xofs, ialpha, yofs, ibeta


def conv_split_k(px_per_frame, N, K, cin):
    """lmx_h_conv_split_k: the C++ twin of kernels.split_k_for."""
    r = _lib.load().lmx_h_conv_split_k(px_per_frame, N, K, cin)
    check(min(r, 0), "lmx_h_conv_split_k")
    return r


# ---- the host table functions (csrc/host_resample.cpp) ---------------------------------------------------------------------
def _tables(fn, kk_dtype, in_size, out_size, filt):
    ks = C.c_int(0)
    check(fn(in_size, out_size, FILT[filt], None, None, 0, C.byref(ks)), fn.__name__)
    bounds, kk = np.empty(out_size * 2, np.int32), np.empty(out_size * ks.value, kk_dtype)
    check(fn(in_size, out_size, FILT[filt], bounds.ctypes.data, kk.ctypes.data, kk.size, C.byref(ks)), fn.__name__)
    return bounds, kk, ks.value


def pil_tables(in_size, out_size, filt):
    """lmx_h_pil_tables: the C++ twin of resample.coeff_tables, same return value."""
    return _tables(_lib.load().lmx_h_pil_tables, np.int32, in_size, out_size, filt)


def aa_tables(in_size, out_size, filt):
    """lmx_h_aa_tables: the C++ twin of resample.aa_tables, same return value."""
    return _tables(_lib.load().lmx_h_aa_tables, np.float32, in_size, out_size, filt)


def identity_table(n):
    """lmx_h_identity_table: the table of an axis that keeps its size (lmx.dino._identity_table)."""
    bounds, kk = np.empty(n * 2, np.int32), np.empty(n, np.int32)
    check(_lib.load().lmx_h_identity_table(n, bounds.ctypes.data, kk.ctypes.data), "lmx_h_identity_table")
    return bounds, kk, 1


def segment_cols(bounds, tile=256):
    """lmx_h_segment_cols: the C++ twin of resample.segment_cols."""
    b = np.ascontiguousarray(bounds, dtype=np.int32).reshape(-1)
    r = _lib.load().lmx_h_segment_cols(b.ctypes.data, b.size // 2, tile)
    check(min(r, 0), "lmx_h_segment_cols")
    return r


# ---- the model handles ----------------------------------------------------------------------------------------------------
class _NativeHandle:
    """What NativeDino and NativeYolo do alike: lmx_<model>_open_host(path, max_batch) on `device` (default: torch's current
    device), lmx_<model>_info, lmx_<model>_close, and the checks of a batch of frames.  A subclass names its entry points' prefix
    and its info struct."""
    _PREFIX = None  # "lmx_dino_"
    _INFO = None    # DinoInfo

    def __init__(self, path, max_batch, device=None):
        self._lib = _lib.load()
        self._h = None
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise LmxError(f"{type(self).__name__}: {self.device} is not a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p(0)
        with torch.cuda.device(self.device):
            check(self._fn("open_host")(str(path).encode(), *self._open_args(max_batch), C.byref(h)), self._PREFIX + "open_host")
        self._h = h
        self.info = self._INFO()
        check(self._fn("info")(self._h, C.byref(self.info)), self._PREFIX + "info")

    def _fn(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def _open_args(self, max_batch):
        """what lmx_<model>_open_host takes between the path and the handle"""
        return (int(max_batch),)

    def _handle(self):
        if self._h is None:
            raise LmxError(f"{type(self).__name__}: the handle is closed")
        return self._h

    def _device_frames(self, frames, what):
        """(n, h, w) of a contiguous u8 [n,h,w,3] tensor on the handle's device"""
        if not (frames.is_cuda and frames.device == self.device and frames.dtype == torch.uint8 and frames.dim() == 4
                and frames.shape[3] == 3 and frames.is_contiguous()):
            raise LmxError(f"{type(self).__name__}.{what}: frames must be a contiguous uint8 [n,h,w,3] tensor on {self.device}")
        return frames.shape[:3]

    def _host_frames(self, frames, what):
        """(the frames as a contiguous u8 [n,h,w,3] numpy array, n, h, w)"""
        a = np.ascontiguousarray(frames)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise LmxError(f"{type(self).__name__}.{what}: frames must be a uint8 [n,h,w,3] array")
        return (a,) + a.shape[:3]

    def close(self):
        if self._h is not None:
            self._fn("close")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeDino(_NativeHandle):
    """lmx_dino_open_host(path, max_batch) on `device` (default: torch's current device)."""
    _PREFIX, _INFO = "lmx_dino_", DinoInfo

    def prepare(self, h, w):
        """lmx_dino_prepare: tables and workspace of one frame size (synchronous); embed() of that size then only enqueues."""
        with torch.cuda.device(self.device):
            check(self._lib.lmx_dino_prepare(self._handle(), int(h), int(w)), "lmx_dino_prepare")

    def embed(self, frames, rgb=False):
        """u8 [n,h,w,3] device tensor (BGR; rgb=True: RGB) -> f32 [n, hidden] on torch's current stream of that device."""
        n, h, w = self._device_frames(frames, "embed")
        emb = torch.empty((n, self.info.hidden), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_dino_embed(self._handle(), C.c_void_p(frames.data_ptr()), n, h, w, 1 if rgb else 0,
                                           C.c_void_p(emb.data_ptr()), st), "lmx_dino_embed")
        return emb

    def embed_host(self, frames, rgb=False):
        """u8 [n,h,w,3] numpy array -> f32 [n, hidden] numpy array (lmx_dino_embed_host: uploads, embeds, downloads, synchronises)."""
        a, n, h, w = self._host_frames(frames, "embed_host")
        emb = np.empty((n, self.info.hidden), np.float32)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_dino_embed_host(self._handle(), a.ctypes.data, n, h, w, 1 if rgb else 0, emb.ctypes.data),
                  "lmx_dino_embed_host")
        return emb

class NativeYolo(_NativeHandle):
    """lmx_yolo_open_host(path, max_batch) on `device` (default: torch's current device).  `precision`: "f16" or "exact"."""
    _PREFIX, _INFO = "lmx_yolo_", YoloInfo

    @property
    def pose(self):
        return self.info.kpt_k > 0

    def class_name(self, cls):
        """lmx_yolo_class_name: the name of class `cls`, None out of range."""
        raw = self._lib.lmx_yolo_class_name(self._handle(), int(cls))
        return None if raw is None else raw.decode("utf-8")

    def prepare(self, h, w, precision):
        """lmx_yolo_prepare: geometry, tables and workspace of one (frame size, plan) (synchronous); predict() / detect() of that
        pair then only enqueue."""
        with torch.cuda.device(self.device):
            check(self._lib.lmx_yolo_prepare(self._handle(), int(h), int(w), PLANS[precision]), "lmx_yolo_prepare")

    def anchors(self, h, w):
        """lmx_yolo_anchors: (oh, ow, A) of an h x w frame."""
        oh, ow, A = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.lmx_yolo_anchors(self._handle(), int(h), int(w), C.byref(oh), C.byref(ow), C.byref(A)), "lmx_yolo_anchors")
        return oh.value, ow.value, A.value

    def predict(self, frames, precision):
        """u8 BGR [n,h,w,3] device tensor -> pred f32 [n, A, 4+nc] on torch's current stream of that device (lmx_yolo_predict)."""
        n, h, w = self._device_frames(frames, "predict")
        A = self.anchors(h, w)[2]
        pred = torch.empty((n, A, 4 + self.info.nc), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_yolo_predict(self._handle(), C.c_void_p(frames.data_ptr()), n, h, w, PLANS[precision], C.c_void_p(pred.data_ptr()), st),
                  "lmx_yolo_predict")
        return pred

    def detect(self, frames, precision, conf=0.25, iou=0.7, max_det=300):
        """u8 BGR [n,h,w,3] device tensor -> (boxes [n,max_det,4], scores, cls, src, counts), plus kpts [n,max_det,K,ndim] for a pose
        image, on torch's current stream of that device (lmx_yolo_detect; the outputs are initialised by the call)."""
        n, h, w = self._device_frames(frames, "detect")
        md = max(int(max_det), 0)
        dev = self.device
        boxes = torch.empty((n, md, 4), dtype=torch.float32, device=dev)
        scores = torch.empty((n, md), dtype=torch.float32, device=dev)
        cls, src = (torch.empty((n, md), dtype=torch.int32, device=dev) for _ in range(2))
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        kpts = torch.empty((n, md, self.info.kpt_k, self.info.kpt_ndim), dtype=torch.float32, device=dev) if self.pose else None
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            check(self._lib.lmx_yolo_detect(self._handle(), C.c_void_p(frames.data_ptr()), n, h, w, PLANS[precision], float(conf), float(iou),
                                            int(max_det), *(C.c_void_p(t.data_ptr()) for t in (boxes, scores, cls, src, counts)),
                                            C.c_void_p(kpts.data_ptr()) if kpts is not None else None, st), "lmx_yolo_detect")
        return (boxes, scores, cls, src, counts) + ((kpts,) if kpts is not None else ())

    def detect_host(self, frames, precision, conf=0.25, iou=0.7, max_det=300):
        """u8 BGR [n,h,w,3] numpy array -> the same outputs as numpy arrays (lmx_yolo_detect_host: uploads, detects, downloads,
        synchronises)."""
        a, n, h, w = self._host_frames(frames, "detect_host")
        md = max(int(max_det), 0)
        boxes, scores = np.empty((n, md, 4), np.float32), np.empty((n, md), np.float32)
        cls, src, counts = np.empty((n, md), np.int32), np.empty((n, md), np.int32), np.empty((n,), np.int32)
        kpts = np.empty((n, md, self.info.kpt_k, self.info.kpt_ndim), np.float32) if self.pose else None
        with torch.cuda.device(self.device):
            check(self._lib.lmx_yolo_detect_host(self._handle(), a.ctypes.data, n, h, w, PLANS[precision], float(conf), float(iou), int(max_det),
                                                 *(t.ctypes.data for t in (boxes, scores, cls, src, counts)),
                                                 kpts.ctypes.data if kpts is not None else None), "lmx_yolo_detect_host")
        return (boxes, scores, cls, src, counts) + ((kpts,) if kpts is not None else ())


class NativeSam(_NativeHandle):
    """lmx_sam_open_host(path, max_batch) on `device` (default: torch's current device).  `precision`: "f16" or "exact"."""
    _PREFIX, _INFO = "lmx_sam_", SamInfo
    OUTPUTS = ("mask", "mask_bits", "contour", "lowres")  # what a caller may leave out (NULL in C); stats and iou always come

    @property
    def grid(self):
        return self.info.image // self.info.patch

    def prepare(self, h, w, precision):
        """lmx_sam_prepare: tables and workspace of one (frame size, plan) (synchronous); encode() / decode() / segment() of that pair
        then only enqueue."""
        with torch.cuda.device(self.device):
            check(self._lib.lmx_sam_prepare(self._handle(), int(h), int(w), PLANS[precision]), "lmx_sam_prepare")

    def resized(self, h, w):
        """lmx_sam_resized: ResizeLongestSide.get_preprocess_shape of an h x w frame -> (nh, nw)."""
        nh, nw = C.c_int(0), C.c_int(0)
        check(self._lib.lmx_sam_resized(self._handle(), int(h), int(w), C.byref(nh), C.byref(nw)), "lmx_sam_resized")
        return nh.value, nw.value

    def _emb_dtype(self, precision):
        """(a Hiera embedding is f16 under both decoder plans: the trunk has one plan)"""
        return torch.float32 if precision == "exact" and self.info.encoder != SAM_ENC_HIERA else torch.float16

    def encode(self, frames, precision):
        """u8 [n,h,w,3] device tensor, channel order as given -> emb [n,G,G,256], f16 ("f16") / f32 ("exact"), on torch's current
        stream of that device (lmx_sam_encode)."""
        n, h, w = self._device_frames(frames, "encode")
        g = self.grid
        emb = torch.empty((n, g, g, 256), dtype=self._emb_dtype(precision), device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_sam_encode(self._handle(), C.c_void_p(frames.data_ptr()), n, h, w, PLANS[precision], C.c_void_p(emb.data_ptr()), st),
                  "lmx_sam_encode")
        return emb

    def _outputs(self, n, h, w, outputs, empty):
        """the output arrays of one call (`empty(shape, dtype name)`), None for those of OUTPUTS the caller leaves out"""
        unknown = set(outputs) - set(self.OUTPUTS)
        if unknown:
            raise LmxError(f"{type(self).__name__}: outputs {sorted(unknown)}: a subset of {self.OUTPUTS}")
        L = 4 * self.grid
        shapes = dict(mask=((n, h, w), "uint8"), mask_bits=((n, h, (w + 7) // 8), "uint8"), stats=((n, 8), "int64"), contour=((n, 8), "int64"),
                      iou=((n,), "float32"), lowres=((n, L, L), "float32"))
        return {k: (empty(*v) if k in outputs or k in ("stats", "iou") else None) for k, v in shapes.items()}

    def _device_boxes(self, boxes, n, what):
        if not (boxes.is_cuda and boxes.device == self.device and boxes.dtype == torch.float32 and tuple(boxes.shape) == (n, 4) and boxes.is_contiguous()):
            raise LmxError(f"{type(self).__name__}.{what}: boxes must be a contiguous float32 [{n},4] tensor on {self.device}")
        return C.c_void_p(boxes.data_ptr())

    def _device_call(self, fn, name, src, n, h, w, boxes, precision, outputs):
        dev = self.device
        out = self._outputs(n, h, w, outputs, lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=dev))
        ptr = {k: (C.c_void_p(t.data_ptr()) if t is not None else None) for k, t in out.items()}
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            check(fn(self._handle(), C.c_void_p(src.data_ptr()), n, h, w, self._device_boxes(boxes, n, name), PLANS[precision], ptr["mask"],
                     ptr["mask_bits"], ptr["stats"], ptr["contour"], ptr["iou"], ptr["lowres"], st), "lmx_sam_" + name)
        return {k: t for k, t in out.items() if t is not None}

    def decode(self, emb, boxes, frame_hw, precision, outputs=OUTPUTS):
        """emb [n,G,G,256] of encode() under the same precision, boxes f32 [n,4] xyxy in frame pixels -> dict(stats int64 [n,8], iou
        f32 [n], and of `outputs`: mask u8 [n,h,w], mask_bits u8 [n,h,ceil(w/8)], contour int64 [n,8], lowres f32 [n,4G,4G])
        (lmx_sam_decode)."""
        g = self.grid
        if not (emb.is_cuda and emb.device == self.device and emb.dtype == self._emb_dtype(precision) and emb.dim() == 4
                and tuple(emb.shape[1:]) == (g, g, 256) and emb.is_contiguous()):
            raise LmxError(f"NativeSam.decode: emb must be a contiguous {self._emb_dtype(precision)} [n,{g},{g},256] tensor on {self.device}")
        h, w = frame_hw
        return self._device_call(self._lib.lmx_sam_decode, "decode", emb, emb.shape[0], int(h), int(w), boxes, precision, outputs)

    def segment(self, frames, boxes, precision, outputs=OUTPUTS):
        """u8 [n,h,w,3] device tensor and boxes f32 [n,4] -> the dict of decode() (lmx_sam_segment: encode into the handle's workspace,
        then decode)."""
        n, h, w = self._device_frames(frames, "segment")
        return self._device_call(self._lib.lmx_sam_segment, "segment", frames, n, h, w, boxes, precision, outputs)

    def segment_host(self, frames, boxes, precision, outputs=OUTPUTS):
        """u8 [n,h,w,3] and f32 [n,4] numpy arrays -> the same dict of numpy arrays (lmx_sam_segment_host: uploads, segments, downloads,
        synchronises)."""
        a, n, h, w = self._host_frames(frames, "segment_host")
        b = np.ascontiguousarray(boxes, dtype=np.float32)
        if b.shape != (n, 4):
            raise LmxError(f"NativeSam.segment_host: boxes must be a float32 [{n},4] array")
        out = self._outputs(n, h, w, outputs, lambda shape, dt: np.empty(shape, getattr(np, dt)))
        ptr = {k: (t.ctypes.data if t is not None else None) for k, t in out.items()}
        with torch.cuda.device(self.device):
            check(self._lib.lmx_sam_segment_host(self._handle(), a.ctypes.data, n, h, w, b.ctypes.data, PLANS[precision], ptr["mask"], ptr["mask_bits"],
                                                 ptr["stats"], ptr["contour"], ptr["iou"], ptr["lowres"]), "lmx_sam_segment_host")
        return {k: t for k, t in out.items() if t is not None}



class NativeFused(_NativeHandle):
    """lmx_fused_open_host: the fused per-frame path (lmx.pipeline.FusedExtractor.step + lmx.dist.pack_records) behind one handle over
    a YOLO, a SAM and a DINO weight image, on `device` (default: torch's current device).  Steps of up to max_frames frames; SAM runs
    in passes of sam_chunk frames, sam_lanes of them in flight.  `precision`: "f16" or "exact".  Every step gives (records uint8
    [rows, stride], layout) with the layout in the form lmx.dist.unpack_records takes.  ONE step in flight per handle: synchronise the
    stream of a step before the next step, schedule() or prepare()."""
    _PREFIX, _INFO = "lmx_fused_", FusedInfo

    def __init__(self, yolo_path, sam_path, dino_path, max_frames, sam_chunk, sam_lanes=2, max_streams=7, device=None):
        self._lib = _lib.load()
        self._h = None
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise LmxError(f"NativeFused: {self.device} is not a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p(0)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_fused_open_host(str(yolo_path).encode(), str(sam_path).encode(), str(dino_path).encode(), int(max_frames), int(sam_chunk),
                                                int(sam_lanes), int(max_streams), C.byref(h)), "lmx_fused_open_host")
        self._h = h
        self.info = FusedInfo()
        check(self._lib.lmx_fused_info(self._h, C.byref(self.info)), "lmx_fused_info")
        self.scheduled = False

    def layout(self, h, w, scheduled=None):
        """lmx_fused_layout -> (layout, stride): the record of an h x w frame (scheduled: None = as the handle's schedule stands)."""
        from . import kernels as K

        lay = RecordLayout()
        sch = self.scheduled if scheduled is None else bool(scheduled)
        check(self._lib.lmx_fused_layout(self._handle(), int(h), int(w), int(sch), C.byref(lay)), "lmx_fused_layout")
        return K.layout_of(lay)

    def prepare(self, h, w, precision):
        """lmx_fused_prepare: the three models' tables and workspaces, every SAM lane and the step's buffers for one (frame size, plan)
        (synchronous); step() of that pair then only enqueues."""
        with torch.cuda.device(self.device):
            check(self._lib.lmx_fused_prepare(self._handle(), int(h), int(w), PLANS[precision]), "lmx_fused_prepare")

    def schedule(self, n, det_idx=None, emb_idx=None):
        """lmx_fused_schedule: the reference schedule for later steps of n frames (FusedExtractor.step's det_idx / emb_idx; None: every
        frame); both None clears it (dense steps).  Synchronous."""
        def arr(idx):
            if idx is None:
                return None, -1
            idx = [int(i) for i in idx]
            return (C.c_int32 * max(1, len(idx)))(*idx), len(idx)

        (d, nd), (e, ne) = arr(det_idx), arr(emb_idx)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_fused_schedule(self._handle(), int(n), d, nd, e, ne), "lmx_fused_schedule")
        self.scheduled = not (det_idx is None and emb_idx is None)

    def step(self, frames, precision, conf=0.5, n_rows=None):
        """u8 BGR [n,h,w,3] device tensor -> (records uint8 [n_rows, stride] on the device, layout), enqueued on torch's current stream
        of that device (lmx_fused_step); n_rows (default n) >= n, the rows from n on are padding."""
        n, h, w = self._device_frames(frames, "step")
        n_rows = n if n_rows is None else int(n_rows)
        layout, stride = self.layout(h, w)
        records = torch.empty((max(n_rows, 0), stride), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_fused_step(self._handle(), C.c_void_p(frames.data_ptr()), n, h, w, PLANS[precision], float(conf),
                                           C.c_void_p(records.data_ptr()), n_rows, st), "lmx_fused_step")
        return records, layout

    def step_host(self, frames, precision, conf=0.5, n_rows=None):
        """u8 BGR [n,h,w,3] numpy array -> (records uint8 [n_rows, stride] numpy array, layout) (lmx_fused_step_host: uploads, steps,
        downloads the records in one copy, synchronises)."""
        a, n, h, w = self._host_frames(frames, "step_host")
        n_rows = n if n_rows is None else int(n_rows)
        layout, stride = self.layout(h, w)
        records = np.empty((max(n_rows, 0), stride), np.uint8)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_fused_step_host(self._handle(), a.ctypes.data, n, h, w, PLANS[precision], float(conf), records.ctypes.data, n_rows),
                  "lmx_fused_step_host")
        return records, layout

    def step_yuv(self, y, c, h, w, precision, layout="nv12", matrix="bt601", v=None, conf=0.5, n_rows=None):
        """NV12 / I420 frames as a decoder leaves them on the device (lmx.kernels.yuv_frames' tensors: pitches and frame strides come
        from the tensors' strides) -> (records, layout) as step(): lmx_fused_step_yuv converts into a BGR buffer the handle owns, then
        steps on it.  The records are those of step(lmx.kernels.yuv420_to_bgr(...)), byte for byte."""
        from . import kernels as K

        f, n, dev = K.yuv_frames(y, c, int(h), int(w), layout, matrix, v)
        if dev != self.device:
            raise LmxError(f"NativeFused.step_yuv: the planes are on {dev}, the handle on {self.device}")
        n_rows = n if n_rows is None else int(n_rows)
        rec_layout, stride = self.layout(h, w)
        records = torch.empty((max(n_rows, 0), stride), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_fused_step_yuv(self._handle(), C.byref(f), n, int(h), int(w), PLANS[precision], float(conf),
                                               C.c_void_p(records.data_ptr()), n_rows, st), "lmx_fused_step_yuv")
        return records, rec_layout

    def step_yuv_roi(self, y, c, h, w, roi, precision, layout="nv12", matrix="bt601", v=None, conf=0.5, n_rows=None):
        """step_yuv on the window roi = (x, y, w, h) of the frames (lmx_fused_step_yuv_roi): the window is converted into the handle's
        BGR buffer and the step runs at the window's size — the records (and their layout) are those of
        step(lmx.kernels.yuv420_to_bgr_roi(...)), byte for byte; prepare(roi h, roi w, precision) is what prepares it."""
        from . import kernels as K

        f, n, dev = K.yuv_frames(y, c, int(h), int(w), layout, matrix, v)
        if dev != self.device:
            raise LmxError(f"NativeFused.step_yuv_roi: the planes are on {dev}, the handle on {self.device}")
        rect = _lib.Rect(*(int(t) for t in roi))
        if rect.w < 1 or rect.h < 1:
            raise LmxError(f"NativeFused.step_yuv_roi: roi is empty: w = {rect.w}, h = {rect.h}")
        n_rows = n if n_rows is None else int(n_rows)
        rec_layout, stride = self.layout(rect.h, rect.w)
        records = torch.empty((max(n_rows, 0), stride), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self._lib.lmx_fused_step_yuv_roi(self._handle(), C.byref(f), n, int(h), int(w), C.byref(rect), PLANS[precision], float(conf),
                                                   C.c_void_p(records.data_ptr()), n_rows, st), "lmx_fused_step_yuv_roi")
        return records, rec_layout

    def step_yuv_host(self, yuv, precision, layout="nv12", matrix="bt601", conf=0.5, n_rows=None):
        """rawvideo frames in host memory, uint8 numpy [n, h * 3 / 2, w] tightly packed (`nv12`, or `yuv420p` as layout "i420") ->
        (records uint8 [n_rows, stride] numpy array, layout) (lmx_fused_step_yuv_host: uploads 1.5 bytes per pixel in one copy,
        converts, steps, downloads the records in one copy, synchronises)."""
        from . import kernels as K

        a = np.ascontiguousarray(yuv)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[1] % 3 != 0:
            raise LmxError("NativeFused.step_yuv_host: yuv must be a uint8 [n, h * 3 / 2, w] array")
        if layout not in K.YUV_LAYOUTS or matrix not in K.YUV_MATRICES:
            raise LmxError(f"NativeFused.step_yuv_host: layout {layout!r} / matrix {matrix!r}: one of {tuple(K.YUV_LAYOUTS)} and one of {tuple(K.YUV_MATRICES)}")
        n, h, w = a.shape[0], a.shape[1] // 3 * 2, a.shape[2]
        n_rows = n if n_rows is None else int(n_rows)
        rec_layout, stride = self.layout(h, w)
        records = np.empty((max(n_rows, 0), stride), np.uint8)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_fused_step_yuv_host(self._handle(), a.ctypes.data, K.YUV_LAYOUTS[layout], K.YUV_MATRICES[matrix], n, h, w,
                                                    PLANS[precision], float(conf), records.ctypes.data, n_rows), "lmx_fused_step_yuv_host")
        return records, rec_layout


def _vp(a):
    """void* of a tensor, of a numpy array or of nothing"""
    return C.c_void_p(0 if a is None else a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def _seeds(who, seeds, n, S, items):
    """one 64-bit seed per clip or graph (`items`) as a uint64 numpy array; None in eval mode"""
    from . import kernels as K

    if S == 0:
        return None
    sd = K.pack_seeds(seeds)
    if sd.shape != (n,):
        raise LmxError(f"{who}: {n} {items} need {n} seeds, got {sd.shape}")
    return sd


class _NativeGait(_NativeHandle):
    """What NativeTcn and NativeXfm do alike: lmx_<model>_open_host(path, max_clips, max_samples), the checks of a series (and of a
    mask) on the device and on the host, one seed per clip, and the outputs of a call."""

    def __init__(self, path, max_clips, max_samples=10, device=None):
        self._max_samples = int(max_samples)
        super().__init__(path, max_clips, device)

    def _open_args(self, max_batch):
        return (int(max_batch), self._max_samples)

    def _seeds(self, seeds, n, S, what):
        return _seeds(f"{type(self).__name__}.{what}", seeds, n, S, "clips")

    def _args(self, what, x, mask, seeds, n_samples, saliency):
        """(x, mask, n, T, S, seeds, pred, stats, saliency or None) of one call: tensors on the handle's device for "score", numpy
        arrays for "score_host"."""
        name, dev, F, host = type(self).__name__, self.device, self.info.input_dim, what == "score_host"
        if host:
            x = np.ascontiguousarray(x, np.float32)
            if x.ndim != 3 or x.shape[2] != F:
                raise LmxError(f"{name}.score_host: x must be a float32 [n, T, {F}] array")
        elif not (x.is_cuda and x.device == dev and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == F and x.is_contiguous()):
            raise LmxError(f"{name}.score: x must be a contiguous float32 [n, T, {F}] tensor on {dev}")
        n, T, S = int(x.shape[0]), int(x.shape[1]), int(n_samples)
        if host and mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (n, T):
                raise LmxError(f"{name}.score_host: mask must be a uint8 [{n}, {T}] array")
        elif mask is not None and not (mask.device == dev and mask.dtype == torch.uint8 and tuple(mask.shape) == (n, T) and mask.is_contiguous()):
            raise LmxError(f"{name}.score: mask must be a contiguous uint8 [{n}, {T}] tensor on {dev}")
        sd = self._seeds(seeds, n, S, what)
        empty = (lambda *shape: np.empty(shape, np.float32)) if host else (lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev))
        return x, mask, n, T, S, sd, empty(n, max(S, 1)), empty(n, 2), empty(n, T) if saliency else None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class NativeTcn(_NativeGait):
    """lmx_tcn_open_host(path, max_clips, max_samples) on `device` (default: torch's current device): the TCN gait model from its
    weight image.  score / score_host give the bits of lmx.tcn.TcnScorer.score (tests/test_gpu_tcn.py)."""
    _PREFIX, _INFO = "lmx_tcn_", TcnInfo

    def score(self, x, seeds, n_samples=10):
        """f32 [n, T, input_dim] device tensor, n host seeds -> (mean [n], std [n], pred [n, max(S, 1)]) on torch's current stream."""
        x, _, n, T, S, sd, pred, stats, _ = self._args("score", x, None, seeds, n_samples, False)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_tcn_score(self._handle(), _vp(x), _vp(sd), n, T, S, _vp(pred), _vp(stats), self._stream()), "lmx_tcn_score")
        return stats[:, 0], stats[:, 1], pred

    def score_host(self, x, seeds, n_samples=10):
        """f32 [n, T, input_dim] numpy array -> numpy (mean, std, pred) (lmx_tcn_score_host: uploads, scores, downloads, synchronises)."""
        x, _, n, T, S, sd, pred, stats, _ = self._args("score_host", x, None, seeds, n_samples, False)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_tcn_score_host(self._handle(), _vp(x), _vp(sd), n, T, S, _vp(pred), _vp(stats)), "lmx_tcn_score_host")
        return stats[:, 0], stats[:, 1], pred


class NativeXfm(_NativeGait):
    """lmx_xfm_open_host(path, max_clips, max_samples) on `device` (default: torch's current device): the gait transformer from its
    weight image.  score / score_host give the bits of lmx.xfm.XfmScorer (tests/test_gpu_xfm.py)."""
    _PREFIX, _INFO = "lmx_xfm_", XfmInfo

    def score(self, x, mask=None, seeds=None, n_samples=10, saliency=False):
        """f32 [n, T, input_dim] and uint8 [n, T] (or None) device tensors, n host seeds -> (mean [n], std [n], pred [n, max(S, 1)],
        saliency [n, T] or None) on torch's current stream."""
        x, mask, n, T, S, sd, pred, stats, sal = self._args("score", x, mask, seeds, n_samples, saliency)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_xfm_score(self._handle(), _vp(x), _vp(mask), _vp(sd), n, T, S, _vp(pred), _vp(stats), _vp(sal), self._stream()),
                  "lmx_xfm_score")
        return stats[:, 0], stats[:, 1], pred, sal

    def score_host(self, x, mask=None, seeds=None, n_samples=10, saliency=False):
        """numpy f32 [n, T, input_dim] and uint8 [n, T] (or None) -> numpy (mean, std, pred, saliency or None) (lmx_xfm_score_host:
        uploads, scores, downloads, synchronises)."""
        x, mask, n, T, S, sd, pred, stats, sal = self._args("score_host", x, mask, seeds, n_samples, saliency)
        with torch.cuda.device(self.device):
            check(self._lib.lmx_xfm_score_host(self._handle(), _vp(x), _vp(mask), _vp(sd), n, T, S, _vp(pred), _vp(stats), _vp(sal)),
                  "lmx_xfm_score_host")
        return stats[:, 0], stats[:, 1], pred, sal


class _NativeGraph(_NativeHandle):
    """What NativeGfm and NativeGnn do alike: lmx_<model>_open_host(path, max_graphs, <the model's limits>), the graphs as the
    model's batch where the call wants them, one seed per graph, and the call with the outputs in the order of the C signature."""

    def __init__(self, path, max_graphs, limits, device=None):
        self._extra = tuple(int(v) for v in limits)
        super().__init__(path, max_graphs, device)

    def _open_args(self, max_batch):
        return (int(max_batch),) + self._extra

    def _batch(self, what, graphs, *extra):
        """the graphs as a batch on the CPU (score_host) or on the handle's device (score)"""
        from . import kernels as K

        cls, where = getattr(K, self._BATCH), torch.device("cpu") if what == "score_host" else self.device
        b = graphs if isinstance(graphs, cls) else cls(graphs, where, *extra)
        if b.device != where:
            raise LmxError(f"{type(self).__name__}.{what}: the graphs are on {b.device}")
        return b

    def _run(self, what, b, seeds, S, outs):
        sd = _seeds(f"{type(self).__name__}.{what}", seeds, b.n, S, "graphs")
        g, name = b.struct(), self._PREFIX + what
        args = [self._handle(), C.byref(g), _vp(sd), S] + [_vp(t) for t in outs]
        if what == "score":
            args.append(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        with torch.cuda.device(self.device):
            check(getattr(self._lib, name)(*args), name)


class NativeGfm(_NativeGraph):
    """lmx_gfm_open_host(path, max_graphs, max_nodes_total, max_samples) on `device` (default: torch's current device): the graph
    transformer from its weight image.  score / score_host give the bits of lmx.gfm.GfmScorer (tests/test_gpu_gfm.py)."""
    _PREFIX, _INFO, _BATCH = "lmx_gfm_", GfmInfo, "GfmBatch"

    def __init__(self, path, max_graphs, max_nodes_total, max_samples=10, device=None):
        super().__init__(path, max_graphs, (max_nodes_total, max_samples), device)

    def _call(self, what, graphs, seeds, n_samples, targets, node):
        b, S = self._batch(what, graphs, targets), int(n_samples)
        empty = lambda *shape: torch.empty(shape, dtype=torch.float32, device=b.device)  # noqa: E731
        pred, stats = empty(b.n, max(S, 1)), empty(b.n, 2)
        npred = empty(b.nodes) if node else None
        attn = empty(b.nodes) if (b.target is not None and S == 0) else None
        self._run(what, b, seeds, S, (pred, stats, npred, attn))
        return stats[:, 0], stats[:, 1], pred, npred, attn

    def score(self, graphs, seeds=None, n_samples=10, targets=None, node=False):
        """graphs: lmx.gfm.build_graph's dicts (or a GfmBatch on the handle's device), n host seeds -> (mean [n], std [n], pred
        [n, max(S, 1)], node_pred [sum N] or None, attn_to_target [sum N] or None: with targets, S = 0) on torch's current stream."""
        return self._call("score", graphs, seeds, n_samples, targets, node)

    def score_host(self, graphs, seeds=None, n_samples=10, targets=None, node=False):
        """The same from and to HOST memory (CPU tensors): lmx_gfm_score_host uploads, scores, downloads, synchronises."""
        return self._call("score_host", graphs, seeds, n_samples, targets, node)


class NativeGnn(_NativeGraph):
    """lmx_gnn_open_host(path, max_graphs, max_nodes_total, max_edges_total, max_samples) on `device` (default: torch's current device):
    GraphGPS from its weight image.  score / score_host give the bits of lmx.gnn.GnnScorer (tests/test_gpu_gnn.py)."""
    _PREFIX, _INFO, _BATCH = "lmx_gnn_", GnnInfo, "GnnBatch"

    def __init__(self, path, max_graphs, max_nodes_total, max_edges_total, max_samples=10, device=None):
        super().__init__(path, max_graphs, (max_nodes_total, max_edges_total, max_samples), device)

    def _call(self, what, graphs, seeds, n_samples):
        b, S = self._batch(what, graphs), int(n_samples)
        empty = lambda *shape: torch.empty(shape, dtype=torch.float32, device=b.device)  # noqa: E731
        mc, stats = (empty(b.nodes, S), empty(b.nodes, 2)) if S else (None, None)
        gp, npred, attw = (None, None, None) if S else (empty(b.n), empty(b.nodes), empty(b.nodes))
        self._run(what, b, seeds, S, (mc, stats, gp, npred, attw))
        return mc, stats, gp, npred, attw

    def score(self, graphs, seeds=None, n_samples=10):
        """graphs: lmx.gnn.build_graph's dicts (or a GnnBatch on the handle's device), n host seeds -> (node_mc [sum N, S], stats
        [sum N, 2], graph_pred [n], node_pred [sum N], attn_weights [sum N]) as lmx.gnn.GnnScorer.forward, on torch's current stream."""
        return self._call("score", graphs, seeds, n_samples)

    def score_host(self, graphs, seeds=None, n_samples=10):
        """The same from and to HOST memory (CPU tensors): lmx_gnn_score_host uploads, scores, downloads, synchronises."""
        return self._call("score_host", graphs, seeds, n_samples)
