"""SAM image encoder on liblmx — the ``predictor.set_image(image)`` half of services/sam3-pipeline/app/main.py:80.

BASELINE cfg#3 names the SAM2 Hiera-B+ trunk + FPN neck; this module runs it as a launch
sequence over the C-ABI kernels:
  pre   : PIL-bilinear ResizeLongestSide(1024) on u8 (lmx_k_pil_resize_*), SamPredictor's (x-mean)/std applied
          to the frame AS GIVEN (the service hands over BGR: SURVEY Appendix C-2) and the zero pad to 1024^2 are
          folded into the patch-embed im2col (lmx_k_im2col_u8);
  trunk : patch-embed GEMM with the windowed position table added in the epilogue (residual broadcast), then 24
          multi-scale blocks: LN -> qkv GEMM -> [2x2 max Q-pool] -> window / global flash attention addressed IN PLACE
          on the token grid (no window_partition copies; padded keys take the qkv bias) -> proj GEMM (+residual, or
          + pooled `proj` shortcut at stage changes) -> LN -> MLP GEMMs (GELU, +residual).  f32 residual stream.
  neck  : 1x1 lateral GEMMs to 256 channels, nearest-x2 top-down add on levels 2/3 (GEMM residual epilogue).
"""
import itertools
import math
import os
import threading
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import kernels as K
from . import resample

SAM_PIXEL_MEAN = (123.675, 116.28, 103.53)
SAM_PIXEL_STD = (58.395, 57.12, 57.375)


@dataclass
class HieraConfig:
    hidden: int = 112
    blocks: tuple = (2, 3, 16, 3)
    dims: tuple = (112, 224, 448, 896)
    heads: tuple = (2, 4, 8, 16)
    windows: tuple = (8, 4, 14, 7)
    global_blocks: tuple = (12, 16, 20)
    pos_bkg: tuple = (14, 14)
    q_pool_stages: int = 3
    fpn_dim: int = 256
    fpn_top_down: tuple = (2, 3)
    eps: float = 1e-6
    image: int = 1024

    def block_plan(self):
        """[(dim_in, dim_out, heads, window, q_stride)] per block (TF sam2 :466-486)."""
        plan, t = [], 0
        for s, nb in enumerate(self.blocks):
            for b in range(nb):
                first = s > 0 and b == 0
                dim = self.dims[s - 1] if first else self.dims[s]
                win = self.windows[s - 1] if first else self.windows[s]
                if t in self.global_blocks:
                    win = 0
                qs = 2 if (0 < s <= self.q_pool_stages and b == 0) else 0
                plan.append((dim, self.dims[s], self.heads[s], win, qs))
                t += 1
        return plan


def hiera_b_plus():
    return HieraConfig()


def param_spec(cfg):
    """Ordered {transformers Sam2VisionModel parameter name: (shape, init kind)}."""
    s = {}
    s["backbone.pos_embed"] = ((1, cfg.hidden) + tuple(cfg.pos_bkg), "tok")
    s["backbone.pos_embed_window"] = ((1, cfg.hidden, cfg.windows[0], cfg.windows[0]), "tok")
    s["backbone.patch_embed.projection.weight"] = ((cfg.hidden, 3, 7, 7), "w")
    s["backbone.patch_embed.projection.bias"] = ((cfg.hidden,), "b")
    for i, (dim, dim_out, heads, win, qs) in enumerate(cfg.block_plan()):
        p = f"backbone.blocks.{i}."
        s[p + "layer_norm1.weight"] = ((dim,), "g")
        s[p + "layer_norm1.bias"] = ((dim,), "b")
        s[p + "attn.qkv.weight"] = ((3 * dim_out, dim), "w")
        s[p + "attn.qkv.bias"] = ((3 * dim_out,), "b")
        s[p + "attn.proj.weight"] = ((dim_out, dim_out), "w")
        s[p + "attn.proj.bias"] = ((dim_out,), "b")
        s[p + "layer_norm2.weight"] = ((dim_out,), "g")
        s[p + "layer_norm2.bias"] = ((dim_out,), "b")
        s[p + "mlp.proj_in.weight"] = ((4 * dim_out, dim_out), "w")
        s[p + "mlp.proj_in.bias"] = ((4 * dim_out,), "b")
        s[p + "mlp.proj_out.weight"] = ((dim_out, 4 * dim_out), "w")
        s[p + "mlp.proj_out.bias"] = ((dim_out,), "b")
        if dim != dim_out:
            s[p + "proj.weight"] = ((dim_out, dim), "w")
            s[p + "proj.bias"] = ((dim_out,), "b")
    for j, c in enumerate(reversed(cfg.dims)):
        s[f"neck.convs.{j}.weight"] = ((cfg.fpn_dim, c, 1, 1), "w")
        s[f"neck.convs.{j}.bias"] = ((cfg.fpn_dim,), "b")
    return s


def resize_longest_side(h, w, target=1024):
    """segment_anything ResizeLongestSide.get_preprocess_shape: int(x*scale + 0.5)."""
    scale = target * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def sam_norm_lut():
    """lut[c][u] = (f32(u) - mean[c]) / std[c] — Sam.preprocess' `(x - pixel_mean) / pixel_std` on the f32 image."""
    u = np.arange(256, dtype=np.float32)
    m = np.array(SAM_PIXEL_MEAN, np.float32)
    s = np.array(SAM_PIXEL_STD, np.float32)
    return ((u[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


# MFMA k-slot order (csrc/hiera.hip), the order in which an accumulator tile is an operand: position 32 s + 8 g + 4 h + i holds
# feature KSLOT[position] = 16 (2 s + h) + 4 g + i.  Every prefix of a multiple of 32 positions is a permutation of its own range.
KSLOT = np.array([16 * (2 * s + h) + 4 * g + i for s in range(8) for g in range(4) for h in range(2) for i in range(4)])


def _swz_wide(r):  # rows of 256 / 512 bytes: the 16-byte chunk c of row r is stored at chunk c ^ (r & 15)
    return r & 15


def _swz_128(r):  # rows of 128 bytes: ... at chunk c ^ ((r >> 1) & 7)
    return (r >> 1) & 7


def _kslot_cols(w, n):
    """w [rows, <= n] -> [rows, n] (n % 32 == 0): column p holds w's column KSLOT[p], zeros where w has no such column."""
    out = np.zeros((w.shape[0], n), w.dtype)
    ok = KSLOT[:n] < w.shape[1]
    out[:, ok] = w[:, KSLOT[:n][ok]]
    return out


def _head_rows(wqkv, bqkv, heads, hh, sec):
    """The rows of head hh in section sec (q | k | v) of the qkv projection, padded to 64: (w [64, Din], b [64]).  v's row 63 is zero
    with bias 1: the softmax sum then rides the PV product."""
    D = wqkv.shape[0] // 3
    hd = D // heads
    w, b = np.zeros((64, wqkv.shape[1]), np.float32), np.zeros((64,), np.float32)
    w[:hd], b[:hd] = wqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd], bqkv[sec * D + hh * hd: sec * D + (hh + 1) * hd]
    if sec == 2:
        b[63] = 1.0
    return w, b


def _head_proj(wo, heads, hh):
    """The output projection's columns of head hh, [Dout, 64] in k-slot order, zeros past the head dim."""
    hd = wo.shape[1] // heads
    return _kslot_cols(wo[:, hh * hd: (hh + 1) * hd], 64)


def _lds_image(m, key, rows=None, cols=None):
    """Matrix m, zero-padded to [rows, cols] (its own shape by default; cols * 2 bytes = 128, 256 or 512 per row), as f16 -> its LDS
    image: the 16-byte chunk c of row r stored at chunk c ^ key(r); zero-padded to 32 KB."""
    rows, cols = rows or m.shape[0], cols or m.shape[1]
    ch = np.zeros((rows, cols), np.float16)
    ch[:m.shape[0], :m.shape[1]] = m
    ch = ch.reshape(rows, cols // 8, 8)
    out = np.zeros_like(ch)
    for r in range(rows):
        out[r, np.arange(cols // 8) ^ key(r)] = ch[r]
    img = np.zeros((16384,), np.float16)
    img[:rows * cols] = out.reshape(-1)
    return img


def pack_hiera_attn(wqkv, bqkv, wo, bo, heads, ln_inside=False):
    """Operands of lmx_k_hiera_attn8 (csrc/hiera.hip) from the block's torch-layout parameters: wqkv [3D, D], bqkv [3D], wo [D, D],
    bo [D] (numpy, f32).  Returns (wqkv_p f16 [3*heads*64, 128], bqkv_p f32 [3*heads*64], wo_p f16 [D, heads*64], bo f32 [D]):
    q | k | v sections with each head padded from D/heads to 64 rows (_head_rows); the 64 columns of a head in wo_p — and, with
    ln_inside (the kernel normalises the f32 rows itself and holds them in accumulator layout), the 128 input columns of wqkv_p — are
    in MFMA k-slot order (KSLOT)."""
    D = wo.shape[0]
    if D // heads > 63 or D > 128:
        raise ValueError("pack_hiera_attn: head dim <= 63 and D <= 128")
    wq = np.zeros((3 * heads * 64, 128), np.float32)
    bq = np.zeros((3 * heads * 64,), np.float32)
    for sec in range(3):
        for hh in range(heads):
            r0 = sec * heads * 64 + hh * 64
            w, bq[r0:r0 + 64] = _head_rows(wqkv, bqkv, heads, hh, sec)
            wq[r0:r0 + 64, :128 if ln_inside else D] = _kslot_cols(w, 128) if ln_inside else w
    wop = np.concatenate([_head_proj(wo, heads, hh) for hh in range(heads)], 1)
    return wq.astype(np.float16), bq, wop.astype(np.float16), np.ascontiguousarray(bo, dtype=np.float32)


def pack_hiera_attn4(wqkv, bqkv, wo, bo, heads):
    """Operands of lmx_k_hiera_attn4 (csrc/hiera.hip): the LDS images of the 4 * heads matrices the kernel streams, and its biases.
    wqkv [3D, D], bqkv [3D], wo [D, D], bo [D] (numpy, f32; D = 224, heads = 4).  Image 4 h + s, s in q | k | v: the head's 64 rows
    (_head_rows) of 512 bytes; image 4 h + 3: the projection's columns of head h (_head_proj) as 256 rows (224 outputs, then zeros)
    of 128 bytes.  bias: [head][q | k | v][64] then bo."""
    imgs, bias = [], []
    for hh in range(heads):
        for sec in range(3):
            w, b = _head_rows(wqkv, bqkv, heads, hh, sec)
            imgs.append(_lds_image(w, _swz_wide, 64, 256))
            bias.append(b)
        imgs.append(_lds_image(_head_proj(wo, heads, hh), _swz_128, 256, 64))
    return np.stack(imgs), np.concatenate(bias + [bo]).astype(np.float32)


def pack_hiera_attn_pool(wsc, bsc, wqkv, bqkv, wo, bo, heads):
    """Operands of lmx_k_hiera_attn_pool (csrc/hiera.hip) for a block that opens a stage: wsc [Dout, Din] / bsc: the shortcut's
    projection; wqkv [3 Dout, Din], bqkv; wo [Dout, Dout], bo (numpy, f32).  LDS images of 32 KB, in the order the kernel streams them.
    Din 112 -> Dout 224 (4 heads): 14 images — shortcut rows 0..127, shortcut rows 128.., then per head [q | k] (64 + 64 rows of 256
    bytes, _head_rows), [v], and the projection's columns of the head (_head_proj, rows of 128 bytes).
    Din 224 -> Dout 448 (8 heads): 47 images — shortcut in 7 images of 64 rows (512-byte rows), then per head q, k, v (64 rows each) and
    the projection's columns of the head in two images (output rows 0..223, 224..447).
    bias: shortcut + projection [Dout], [head][q | k | v][64][, Dout zeros]."""
    Dout, Din = wsc.shape
    wide = Din > 128  # 512-byte rows
    step, cols = (64, 256) if wide else (128, 128)
    imgs = [_lds_image(wsc[j:j + step], _swz_wide, step, cols) for j in range(0, Dout, step)]
    bias = [bsc + bo]  # the shortcut's and the output projection's biases: one vector, added once
    for hh in range(heads):
        (q, bq), (k, bk), (v, bv) = (_head_rows(wqkv, bqkv, heads, hh, sec) for sec in range(3))
        bias += [bq, bk, bv]
        sections = (q, k, v) if wide else (np.concatenate([q, k]), v)
        imgs += [_lds_image(w, _swz_wide, len(w), cols) for w in sections]
        proj = _head_proj(wo, heads, hh)
        imgs += [_lds_image(half, _swz_128, 256, 64) for half in ((proj[:Dout // 2], proj[Dout // 2:]) if wide else (proj,))]
    if not wide:
        bias.append(np.zeros((Dout,), np.float32))
    return np.stack(imgs), np.concatenate(bias).astype(np.float32)


def pack_ln_mlp(w1, b1, w2, b2, g2, e2, gn=None, en=None):
    """Operands of lmx_k_ln_mlp_img (csrc/hiera.hip): w1 [4D, D], b1 [4D], w2 [D, 4D], b2 [D] (torch Linear layouts), layer_norm2's
    g2 / e2 and — for the kernel's h_next output — the next block's layer_norm1's gn / en (numpy, f32; D = 112 or 224).  Per step of
    64 hidden units: the 64 rows of w1 with their D input columns in k-slot order (rows of 256 bytes at D = 112, 512 at 224) and the
    D rows x 64 columns of w2, columns in k-slot order (rows of 128 bytes); at D = 112 both halves share an image (w2's at byte
    16384), at D = 224 they alternate.  bias: [b1 | b2 | g2 | e2 | gn | en], zeros for gn / en where no next block is given."""
    D = w2.shape[0]
    imgs = []
    for c in range(0, 4 * D, 64):
        i1 = _lds_image(_kslot_cols(w1[c:c + 64], 128 if D <= 128 else 256), _swz_wide)
        i2 = _lds_image(_kslot_cols(w2[:, c:c + 64], 64), _swz_128)
        if D <= 128:
            i1[8192:8192 + D * 64] = i2[:D * 64]
            imgs.append(i1)
        else:
            imgs += [i1, i2]
    z = np.zeros((D,), np.float32)
    bias = np.concatenate([b1, b2, g2, e2, gn if gn is not None else z, en if en is not None else z]).astype(np.float32)
    return np.stack(imgs), bias


# shape class (dim, dim_out, heads, window, q_stride) -> the kernel of csrc/hiera.hip that runs such a block's attention half in one
# launch.  The encoder packs operands for every block of such a class, whatever the switches say; hiera_plan() decides per call
FUSED_ATTN = {(112, 112, 2, 8, 0): "attn8",       # Hiera-B+ stage 1
              (224, 224, 4, 4, 0): "attn4",       # stage 2 after its first block: the same, weights streamed
              (112, 224, 4, 8, 2): "attn_pool",   # the blocks that open stages 2 and 3: pooled queries and shortcut
              (224, 448, 8, 4, 2): "attn_pool"}


def attn8_ln_inside(i, fused_mlp):
    """Block i of the attn8 class normalises its rows in the kernel (operands packed with ln_inside): the first block, and every one
    when no fused MLP in front writes its layer_norm1 rows (the class has D = 112, a width every fused MLP is built for)."""
    return i == 0 or not fused_mlp


class BlockPlan(NamedTuple):
    """What one Hiera block runs: a record of hiera_plan(), executed by HieraEncoder.trunk()."""
    H: int             # the token grid going in: rows (the band's while it lasts; behind a join the rows joined to), columns,
    W: int
    Hf: int            # and the whole grid's rows at this resolution
    Ho: int            # the same going out (halved where the block pools its queries)
    Wo: int
    Hfo: int
    join: int          # > 0: the band grows or ends in front of this block; its `join` rows are joined with the table's to H rows
    attn: str          # the attention half: "attn8_ln" (layer_norm1 inside) | "attn8" | "attn_pool" | "attn4" | "launches"
    ln1: str           # layer_norm1's rows come from: "kernel" (attn8_ln) | "prev" (the previous block's MLP kernel) | "launch"
    shortcut: str      # launches only: None | "gemm" | "gemm+maxpool" | "pooled_gemm"
    query: str         # launches only: "qkv" | "qkv+maxpool" | "pooled_q+kv"
    window: int        # 0: global attention
    ln_out: bool       # launches only: the projection's tile holds whole rows and writes layer_norm2's with them (K.gemm ln_out)
    mlp: str           # "img" (csrc/hiera.hip, streamed images) | "fused" (csrc/mlp.hip) | "launches" (LayerNorm + two GEMMs)
    emit_ln1: bool     # the MLP kernel also writes the next block's layer_norm1 rows, while it still holds them
    stage_end: bool
    keep: bool         # stage end: the output is returned (else None: below `lowest`)
    x16: bool          # ... and the MLP kernel writes the f16 copy the FPN's lateral convolution reads
    join_out: bool     # ... as a tensor of its own: the band's rows, then the table's
    clone: bool        # ... and the stream goes on in a copy: a same-width next block would update the kept output in place

    def choices(self):
        """The kernel choices alone: what the band's constant rows depend on besides the weights."""
        return (self.attn, self.ln1, self.shortcut, self.query, self.ln_out, self.mlp, self.emit_ln1)


def hiera_plan(cfg, n, rows, fused_mlp=True, lowest=0, proj_ln=True):
    """[BlockPlan per block] for n frames whose blocks in front of the first global one run on `rows` stage-1 token rows (a band, or
    cfg.image // 4: the whole grid).  rows may also be a sequence with one entry per block: the token rows, of the grid that block
    reads, it runs on (K.hiera_bands) — where a block needs more than the block before it left, a join sits in front of it and the
    band goes on behind it with the rows it needs.  The one place that chooses kernels, computed per call: the K.*_ok functions read
    their environment switches every time.  lowest: stage outputs below this index are not kept.  proj_ln=False: no ln_out
    projections."""
    g = cfg.image // 4
    blocks = cfg.block_plan()
    first_global = next((i for i, b in enumerate(blocks) if b[3] == 0), None)
    stage_ends = [e - 1 for e in itertools.accumulate(cfg.blocks)]
    per = None if isinstance(rows, int) else tuple(rows)
    if per is not None and len(per) != len(blocks):
        raise ValueError(f"hiera_plan: {len(per)} row counts for {len(blocks)} blocks")
    H, W, Hf = rows if per is None else per[0], g, g
    band = H < g
    plan, prev = [], None  # prev: the block before, which learns from this one's attention half whether to emit layer_norm1
    for i, (dim, D, heads, win, qs) in enumerate(blocks):
        # one number: the band ends in front of the first global block, where every token sees every other
        need = per[i] if per is not None else Hf if band and i == first_global else H
        if per is not None and not H <= need <= Hf:
            raise ValueError(f"hiera_plan: block {i} on {need} rows, the block before left {H} of {Hf}")
        join = H if need > H else 0
        if join:
            H, band = need, need < Hf
        fused = FUSED_ATTN.get((dim, D, heads, win, qs))
        shortcut = query = None
        if fused == "attn8" and K.hiera_attn8_ok(D, heads, win, H, W, qs):
            attn = "attn8_ln" if attn8_ln_inside(i, fused_mlp) else "attn8"
        elif fused == "attn_pool" and K.hiera_attn_pool_ok(dim, D, heads, win, H, W, qs):
            attn = "attn_pool"
        elif fused == "attn4" and K.hiera_attn4_ok(D, heads, win, H, W, qs):
            attn = "attn4"
        else:
            # pooled: the GEMM writes the 2 x 2 max-pool of its product (the shortcut's; the q third's, k and v from a second launch)
            pooled = qs and K.pooled_gemm_ok(n * H * W, D)
            attn = "launches"
            shortcut = None if dim == D else "pooled_gemm" if pooled else "gemm+maxpool" if qs else "gemm"
            query = "pooled_q+kv" if pooled else "qkv+maxpool" if qs else "qkv"
        ln1 = "kernel" if attn == "attn8_ln" else "launch"
        if prev is not None:
            if prev.mlp != "launches" and attn != "attn8_ln":
                prev = prev._replace(emit_ln1=True)
                if not join:  # (behind a join those rows are the band's alone: dropped)
                    ln1 = "prev"
            plan.append(prev)
        Ho, Wo, Hfo = (H // 2, W // 2, Hf // 2) if qs else (H, W, Hf)
        mlp = "launches" if not (fused_mlp and D in K.FUSED_MLP_WIDTHS) else "img" if K.ln_mlp_img_ok(D, n * Ho * Wo) else "fused"
        # stage 3 of Hiera-B+ after its opening block: the layer's choice, whatever the batch
        ln_out = attn == mlp == "launches" and proj_ln and dim == D == 448 and not qs
        end = i in stage_ends
        keep = end and stage_ends.index(i) >= lowest
        prev = BlockPlan(H, W, Hf, Ho, Wo, Hfo, join, attn, ln1, shortcut, query, win, ln_out, mlp, False, end, keep,
                         x16=keep and mlp != "launches", join_out=keep and band,
                         clone=keep and not band and i + 1 < len(blocks) and blocks[i + 1][0] == blocks[i + 1][1])
        H, W, Hf = Ho, Wo, Hfo
    return plan + [prev]


# lmx_hiera_block_t's enums (include/lmx.h) -> BlockPlan's strings
_ATTN = ("attn8_ln", "attn8", "attn_pool", "attn4", "launches")
_LN1 = ("kernel", "prev", "launch")
_SHORTCUT = (None, "gemm", "gemm+maxpool", "pooled_gemm")
_QUERY = (None, "qkv", "qkv+maxpool", "pooled_q+kv")
_MLP = ("img", "fused", "launches")


def _block_plan_of(rec):
    H, W, Hf, Ho, Wo, Hfo, join, attn, ln1, shortcut, query, window, ln_out, mlp, emit_ln1, stage_end, keep, x16, join_out, clone = rec
    return BlockPlan(H, W, Hf, Ho, Wo, Hfo, join, _ATTN[attn], _LN1[ln1], _SHORTCUT[shortcut], _QUERY[query], window, bool(ln_out), _MLP[mlp],
                     bool(emit_ln1), bool(stage_end), bool(keep), bool(x16), bool(join_out), bool(clone))


def native_plan(cfg, n, nh, nw, lowest=0):
    """(rows per block, [BlockPlan per block]) for n frames resized to nh x nw as the C side computes them (lmx_h_hiera_plan): what
    HieraEncoder(band="blocks")._settle and hiera_plan give for an encoder built the default way with no LMX_* switch set — the plan
    a caller without Python runs (tests/test_hiera_plan_c_host.py holds the two equal)."""
    rows, recs = K.hiera_plan_host(cfg, n, nh, nw, lowest)
    return rows, [_block_plan_of(r) for r in recs]


def native_plan_rows(cfg, n, rows, lowest=0):
    """[BlockPlan per block] = hiera_plan(cfg, n, rows, lowest=lowest) as the C side computes it (lmx_h_hiera_plan_rows)."""
    return [_block_plan_of(r) for r in K.hiera_plan_rows_host(cfg, n, rows, lowest)]


class HieraEncoder:
    """Device-resident Hiera trunk + FPN.  ``encode(frames)`` -> dict(fpn=[3 NHWC f16 levels, high->low res],
    stages=[4 f32 stage outputs]).  Token grids are [n, H, W, C] row-major throughout (no partition copies).

    Every call computes its block plan on the host (hiera_plan: which kernels each block runs, where its layer_norm1 rows come from,
    what happens at a stage end) and trunk() executes it record by record.

    band (default on): a landscape frame fills only the top rows of the square canvas, and until the first global-attention block
    tokens mix only inside windows and 2 x 2 pools — a token row whose windows never reach a pixel holds the same values for every
    frame.  The blocks in front of the first global one then run on the top rows alone (K.hiera_band: 168 of 256 stage-1 rows for a
    16:9 frame); the other rows come from a table built once per frame geometry (_band_table) and are joined in front of the first
    global block (K.band_join).  Every kernel computes a row from its window alone, whatever the grid's height, so the result is
    bit for bit that of band=False (tests/test_gpu_hiera_band.py).

    band="blocks": the band is sized block by block (block_rows: 152 / 76 stage-1 / stage-2 rows for that frame, and 42 of stage 3
    only where the 14 x 14 windows begin); where a block needs more rows than the one before it left, a join in front of it adds the
    constant rows between the two and the band goes on behind it (tests/test_gpu_hiera_block_bands.py)."""

    def __init__(self, cfg, state_dict, device="cuda", fused_mlp=True, band=True):
        if band not in (True, False, "blocks"):
            raise ValueError(f"band {band!r}: expected True, False or 'blocks'")
        self.cfg = cfg
        self.band = band
        self.device = torch.device(device)
        # False: LN / GEMM / GEMM launches for every width (A/B comparisons and tests; LMX_NO_FUSED_MLP=1 forces it)
        self.fused_mlp = fused_mlp and not os.environ.get("LMX_NO_FUSED_MLP")
        self.proj_ln = True  # False: no projection writes layer_norm2 (hiera_plan's ln_out; tests compare the two)
        dev = self.device
        sd = state_dict

        def t32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def t16(a):
            return t32(a).to(torch.float16).contiguous()

        # patch embed: conv [D,3,7,7] -> GEMM [D, (ky,kx,c)] padded to K%8==0
        w = np.transpose(sd["backbone.patch_embed.projection.weight"], (0, 2, 3, 1)).reshape(cfg.hidden, 147)
        self.k_pad = 152
        self.pe_w = t16(np.concatenate([w, np.zeros((cfg.hidden, self.k_pad - 147), np.float32)], 1))
        self.pe_b = t32(sd["backbone.patch_embed.projection.bias"])
        # windowed position table for the (fixed) input grid, computed once on the host like _get_pos_embed (:640-646)
        g = cfg.image // 4
        pe = torch.nn.functional.interpolate(torch.from_numpy(sd["backbone.pos_embed"]), size=(g, g), mode="bicubic")
        win = torch.from_numpy(sd["backbone.pos_embed_window"])
        pe = pe + win.tile([x // y for x, y in zip(pe.shape, win.shape)])
        self.pos = pe.permute(0, 2, 3, 1).reshape(g * g, cfg.hidden).contiguous().to(dev)
        self.grid0 = g
        self.blocks = []
        for i, (dim, dim_out, heads, win_, qs) in enumerate(cfg.block_plan()):
            p = f"backbone.blocks.{i}."
            qkv_b = sd[p + "attn.qkv.bias"]
            blk = dict(dim=dim, dim_out=dim_out, heads=heads, win=win_, qs=qs,
                       g1=t32(sd[p + "layer_norm1.weight"]), b1=t32(sd[p + "layer_norm1.bias"]),
                       wqkv=t16(sd[p + "attn.qkv.weight"]), bqkv=t32(qkv_b),
                       # what Linear(0) yields for a zero-padded token, rounded like the GEMM output
                       padkv=t16(qkv_b),
                       wo=t16(sd[p + "attn.proj.weight"]), bo=t32(sd[p + "attn.proj.bias"]),
                       g2=t32(sd[p + "layer_norm2.weight"]), b2=t32(sd[p + "layer_norm2.bias"]),
                       w1=t16(sd[p + "mlp.proj_in.weight"]), bb1=t32(sd[p + "mlp.proj_in.bias"]),
                       w2=t16(sd[p + "mlp.proj_out.weight"]), bb2=t32(sd[p + "mlp.proj_out.bias"]))
            if dim != dim_out:
                blk["wp"], blk["bp"] = t16(sd[p + "proj.weight"]), t32(sd[p + "proj.bias"])
            kind = FUSED_ATTN.get((dim, dim_out, heads, win_, qs))
            if kind:
                f32 = lambda k: np.asarray(sd[p + k], np.float32)  # noqa: E731
                attn = (f32("attn.qkv.weight"), f32("attn.qkv.bias"), f32("attn.proj.weight"), f32("attn.proj.bias"), heads)
                packed = (pack_hiera_attn(*attn, ln_inside=attn8_ln_inside(i, self.fused_mlp)) if kind == "attn8" else
                          pack_hiera_attn4(*attn) if kind == "attn4" else pack_hiera_attn_pool(f32("proj.weight"), f32("proj.bias"), *attn))
                blk["attn"] = tuple(torch.from_numpy(a).to(dev) for a in packed)
            self.blocks.append(blk)
        for i, blk in enumerate(self.blocks):  # the fused MLP's operands as LDS images, with the NEXT block's layer_norm1 vectors
            nxt = self.blocks[i + 1] if i + 1 < len(self.blocks) else None
            blk["next_ln1"] = (nxt["g1"], nxt["b1"]) if nxt else None  # (csrc/mlp.hip's kernel takes them as tensors)
            if blk["dim_out"] in (112, 224) and self.fused_mlp:
                p = f"backbone.blocks.{i}."
                nx = f"backbone.blocks.{i + 1}." if nxt else None
                f32 = lambda k: np.asarray(sd[k], np.float32)  # noqa: E731
                blk["mlp_img"] = tuple(torch.from_numpy(a).to(dev) for a in pack_ln_mlp(
                    f32(p + "mlp.proj_in.weight"), f32(p + "mlp.proj_in.bias"), f32(p + "mlp.proj_out.weight"), f32(p + "mlp.proj_out.bias"),
                    f32(p + "layer_norm2.weight"), f32(p + "layer_norm2.bias"),
                    f32(nx + "layer_norm1.weight") if nx else None, f32(nx + "layer_norm1.bias") if nx else None))
        n = len(cfg.dims) - 1
        self.neck = [(t16(sd[f"neck.convs.{n - i}.weight"][:, :, 0, 0]), t32(sd[f"neck.convs.{n - i}.bias"])) for i in range(n + 1)]
        self.lut = t32(sam_norm_lut())
        self._tabs = {}
        self.first_global = next((i for i, B in enumerate(self.blocks) if B["win"] == 0), None)
        self._bands, self._block_bands, self._band_tabs, self._band_lock = {}, {}, {}, threading.Lock()

    # ---- preprocessing ------------------------------------------------------------------------------------
    def _tables(self, h, w):
        key = (h, w)
        if key not in self._tabs:
            nh, nw = resize_longest_side(h, w, self.cfg.image)
            dev = self.device

            def up(tab):
                b, k, ks = tab
                return (torch.from_numpy(b).to(dev), torch.from_numpy(k).to(dev), ks)

            th = up(resample.coeff_tables(w, nw, resample.BILINEAR)) if nw != w else None
            tv = up(resample.coeff_tables(h, nh, resample.BILINEAR)) if nh != h else None
            self._tabs[key] = (nh, nw, th, tv)
        return self._tabs[key]

    def preprocess(self, frames, band=0):
        """u8 [n,h,w,3] (channel order as handed over) -> (PIL-resized u8 [n,nh,nw,3], patch matrix f16 [n*g*g, 152]); band > 0: the
        patches of the top `band` token rows only, [n*band*g, 152] (a canvas of 4 * band pixel rows)."""
        n, h, w, _ = frames.shape
        nh, nw, th, tv = self._tables(h, w)
        img = K.pil_resize(frames, nw, nh, th, tv, swap_rb=False)
        S = self.cfg.image
        return img, K.im2col_u8(img, self.lut, 4 * band if band else S, S, 7, 7, 4, 3, self.k_pad)

    # ---- the band of rows that depends on the frame ---------------------------------------------------------
    def band_rows(self, nh, nw):
        """Stage-1 token rows the blocks in front of the first global one compute for a frame resized to nh x nw; 0: the whole grid."""
        if (nh, nw) not in self._bands:
            plan = self.cfg.block_plan()
            self._bands[(nh, nw)] = K.hiera_band([p[3] for p in plan], [p[4] for p in plan], self.grid0, nh, nw)
        return self._bands[(nh, nw)]

    def block_rows(self, nh, nw, n=1):
        """band="blocks": the token rows each block runs on for n frames resized to nh x nw, one entry per block at the resolution
        that block reads (K.hiera_bands); the whole grid from the first global block on, and everywhere where there is no band.
        The constant rows come from the whole-grid plan's kernels (_band_table), so a block in the band must run the kernel that
        plan chose: one whose shape check fails on the rule's rows runs on the next count of whole windows that passes — up to
        the whole grid, where it needs no constant rows — and is never moved to another kernel, whose rounding the table lacks."""
        return self._settle(nh, nw, n)[0]

    def _settle(self, nh, nw, n, lowest=0):
        """-> (block_rows(nh, nw, n), the band's plan on them, the whole-grid plan of one frame that builds the table); the plans are
        None where there is no band."""
        if (nh, nw) not in self._block_bands:
            plan = self.cfg.block_plan()
            self._block_bands[(nh, nw)] = K.hiera_bands([p[3] for p in plan], [p[4] for p in plan], self.grid0, nh, nw)
        rows = self._block_bands[(nh, nw)]
        if rows[0] == self.grid0:
            return rows, None, None
        whole, blocks = self.plan(1, self.grid0), self.cfg.block_plan()
        while True:  # (every round adds rows to a block: it ends at the whole grid at the latest)
            plan = self.plan(n, rows, lowest)
            bad = next((i for i in range(self.first_global) if plan[i].H < plan[i].Hf and plan[i].choices() != whole[i].choices()), None)
            if bad is None:
                return rows, plan, whole
            rows, d = list(rows), 0
            for i in range(bad, self.first_global):
                piece = math.lcm(blocks[i][3], 2 if blocks[i][4] else 1)
                d = max(d, rows[i] + piece if i == bad else rows[i])
                rows[i] = d = min(-(-d // piece) * piece, plan[i].Hf)
                if blocks[i][4]:
                    d //= 2
            rows = tuple(rows)

    def plan(self, n, rows, lowest=0):
        """hiera_plan() of this encoder for n frames on `rows` stage-1 token rows in front of the first global block, or on the rows
        per block of block_rows()."""
        return hiera_plan(self.cfg, n, rows, self.fused_mlp, lowest, self.proj_ln)

    def _table_key(self, nh, nw, band, whole=None):
        """The band table's key: the geometry, the band (one number, or the rows per block) and the kernel choices of the pass that
        builds it — one frame, the whole grid (`whole`: that plan, where the caller has it), the blocks in front of the first global
        one — so it never depends on a caller's batch size (K.pooled_gemm_ok does)."""
        return (nh, nw, band, tuple(p.choices() for p in (whole or self.plan(1, self.grid0))[:self.first_global]))

    def _band_table(self, frames, nh, nw, band, whole=None):
        """The rows below the band, the same for every frame of this geometry: dict(x = {block with a join in front: rows [have, need)
        of the f32 stream entering it}, stages / stages16 = the rows below the band of the stage outputs inside it), each
        [rows * W_s, D].  Built once per _table_key by the full-grid path on one frame, outside any running launch trace (a trace
        describes the steady step), and finished with a synchronisation of the building stream: passes on other streams read the
        table without an event."""
        key = self._table_key(nh, nw, band, whole)
        tab = self._band_tabs.get(key)
        if tab is not None:
            return tab
        if torch.cuda.is_current_stream_capturing():
            raise K.LmxError("HieraEncoder: the constant rows below the band are not built for this frame geometry, and a stream capture "
                             "cannot build them (it needs a synchronisation): call encode() once before capturing")
        with self._band_lock:
            if key in self._band_tabs:
                return self._band_tabs[key]
            trace, K.LAUNCH_TRACE = K.LAUNCH_TRACE, None
            try:
                plan = self.plan(1, band)  # the band's own plan: where its joins sit and how many rows its stage outputs have
                taps = {i: (P.join, P.H) for i, P in enumerate(plan) if P.join}
                ends = [P.Ho for P in plan if P.stage_end and P.join_out]
                stages, stages16 = self.trunk(self.preprocess(frames[:1])[1], 1, taps=taps)

                def below(t, Hb):  # rows >= Hb of a [1, Hs, Ws, D] grid, as a table of its own
                    return t.reshape(-1, t.shape[-2], t.shape[-1])[Hb:].reshape(-1, t.shape[-1]).clone()

                tab = dict(x=taps, stages=[below(s, Hb) for s, Hb in zip(stages, ends)],
                           stages16=[below(s16.view(s.shape), Hb) if s16 is not None else None for s, s16, Hb in zip(stages, stages16, ends)])
            finally:
                K.LAUNCH_TRACE = trace
            torch.cuda.current_stream(self.device).synchronize()
            self._band_tabs[key] = tab  # (tables of earlier selections stay: a pass on another stream may still read one)
        return tab

    # ---- network ------------------------------------------------------------------------------------------
    def trunk(self, patches, n, band=0, table=None, lowest=0, taps=None, plan=None):
        """patches -> (stages, stages16): executes self.plan(n, band or the whole grid, lowest) block by block.  band > 0, or the rows
        per block of block_rows(): `patches` hold the band's stage-1 token rows of each frame; the blocks in front of the first
        global one run on those rows, and `table` (_band_table) supplies the others in front of every block that needs more and
        in the stage outputs inside the band.  lowest: stage outputs below this index are not kept (None).  taps (one frame, the
        whole grid) = {block: (have, need)}: each entry is replaced by a copy of rows [have, need) of the stream entering that
        block, and the trunk stops in front of the last of them.  plan: that plan, where the caller has computed it."""
        cfg = self.cfg
        g = self.grid0
        rows = band or g
        H = rows if isinstance(rows, int) else rows[0]
        x = K.gemm(patches, self.pe_w, bias=self.pe_b, res=self.pos[:H * g], res_rows=H * g, out_dtype=torch.float32)
        stages, stages16 = [], []
        dev = x.device
        h_next = None
        for i, (P, B) in enumerate(zip(plan or self.plan(n, rows, lowest), self.blocks)):
            if taps and i in taps:
                have, need = taps[i]
                taps[i] = x.view(P.H, P.W, -1)[have:need].reshape((need - have) * P.W, -1).clone()
                if i == max(taps):
                    return stages, stages16
            if P.join:
                x = K.band_join(x.view(n, P.join, P.W, -1), table["x"][i], P.H).view(n * P.H * P.W, -1)
            D, heads = B["dim_out"], B["heads"]
            h = None if P.ln1 == "kernel" else h_next if P.ln1 == "prev" else K.layernorm(x, B["g1"], B["b1"], cfg.eps)
            h2 = None
            # the attention half, [layer_norm1 ->] qkv -> window attention -> proj + residual, in one launch (csrc/hiera.hip) ...
            if P.attn == "attn8_ln":
                K.hiera_attn8(x, B["attn"], n, P.H, P.W, heads, ln=(B["g1"], B["b1"], cfg.eps))
            elif P.attn == "attn8":
                K.hiera_attn8(x, B["attn"], n, P.H, P.W, heads, h=h)
            elif P.attn == "attn_pool":  # the stage-opening block: pooled q + shortcut
                x = K.hiera_attn_pool(h, B["attn"], n, P.H, P.W, heads, D)
            elif P.attn == "attn4":
                K.hiera_attn4(h, x, B["attn"], n, P.H, P.W, heads)
            else:  # ... or as separate launches
                x, h2 = self._attention_half(P, B, h, x, n)
            rows = n * P.Ho * P.Wo
            # the FPN's lateral convolution reads a stage output as f16: written by the MLP kernel, not cast later
            x16 = torch.empty((rows, D), dtype=torch.float16, device=dev) if P.x16 else None
            h_next = torch.empty((rows, D), dtype=torch.float16, device=dev) if P.emit_ln1 else None
            if P.mlp == "img":  # (the next block's LayerNorm vectors are packed in)
                K.ln_mlp_img(x, B["mlp_img"], cfg.eps, x16=x16, h_next=h_next)
            elif P.mlp == "fused":  # one pass over x (csrc/mlp.hip)
                K.ln_mlp(x, B["g2"], B["b2"], B["w1"], B["bb1"], B["w2"], B["bb2"], cfg.eps, x16=x16,
                         next_ln=B["next_ln1"] + (h_next,) if P.emit_ln1 else None)
            else:
                if h2 is None:  # (else: written by the attention projection, ln_out)
                    h2 = K.layernorm(x, B["g2"], B["b2"], cfg.eps)
                u = K.gemm(h2, B["w1"], bias=B["bb1"], act=K.ACT_GELU)
                K.gemm(u, B["w2"], bias=B["bb2"], res=x, out=x)
            if not P.stage_end:
                continue
            k = len(stages)
            if not P.keep:
                stages.append(None)
                stages16.append(None)
            elif P.join_out:  # the band's rows, then the constant ones
                stages.append(K.band_join(x.view(n, P.Ho, P.Wo, D), table["stages"][k], P.Hfo))
                stages16.append(K.band_join(x16.view(n, P.Ho, P.Wo, D), table["stages16"][k], P.Hfo).view(-1, D) if x16 is not None else None)
            else:
                stages.append(x.view(n, P.Ho, P.Wo, D))
                stages16.append(x16)
                if P.clone:
                    x = x.clone()
        return stages, stages16  # stages16: f16 copies of the stage outputs where the stage's last kernel wrote one (else None)

    def _attention_half(self, P, B, h, x, n):
        """[shortcut GEMM ->] qkv GEMM -> [Q-pool] -> attention -> proj GEMM + residual as separate launches, in the forms P names;
        returns x after the block's pooling and layer_norm2(x) where the projection wrote it (P.ln_out), else None."""
        D, heads, win, qs = B["dim_out"], B["heads"], P.window, B["qs"]
        hd = D // heads
        H, W, Hq, Wq = P.H, P.W, P.Ho, P.Wo
        dev = h.device
        if P.shortcut is None:
            res = x
        elif P.shortcut == "pooled_gemm":  # the shortcut's projection and its 2 x 2 max-pool in one launch
            res = K.gemm(h, B["wp"], bias=B["bp"], out_dtype=torch.float32, pool_hw=(H, W))
        else:
            res = K.gemm(h, B["wp"], bias=B["bp"], out_dtype=torch.float32)
            if P.shortcut == "gemm+maxpool":
                pooled = torch.empty((n, Hq, Wq, D), dtype=torch.float32, device=dev)
                K.maxpool2(res.view(n, H, W, D), pooled)
                res = pooled.view(-1, D)
        if P.query == "pooled_q+kv":
            # pooled queries: the q third of the projection writes its 2 x 2 max-pool directly (a_mode 2), k and v come from
            # a second launch on the same rows — the full-resolution q is neither written nor read back by a pooling pass
            q = K.gemm(h, B["wqkv"][:D], bias=B["bqkv"][:D], pool_hw=(H, W))
            kv = K.gemm(h, B["wqkv"][D:], bias=B["bqkv"][D:])
            k, v = kv[:, :D], kv[:, D:]
        else:
            qkv = K.gemm(h, B["wqkv"], bias=B["bqkv"])
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            if P.query == "qkv+maxpool":
                qp = torch.empty((n, Hq, Wq, D), dtype=torch.float16, device=dev)
                K.maxpool2(qkv.view(n, H, W, 3 * D)[..., :D], qp)
                q = qp.view(-1, D)
        a = torch.empty((n * Hq * Wq, D), dtype=torch.float16, device=dev)
        if win > 0:
            nW = -(-H // win) * -(-W // win)
            wq = win // 2 if qs else win
            K.attention(q, k, v, a, n * nW, heads, wq * wq, win * win, hd, hd ** -0.5,
                        window=dict(Gh=H, Gw=W, ws=win, q_stride=2 if qs else 1),
                        pad_k=B["padkv"][D:2 * D], pad_v=B["padkv"][2 * D:])
        else:
            K.attention(q, k, v, a, n, heads, Hq * Wq, H * W, hd, hd ** -0.5)
        xo = torch.empty((n * Hq * Wq, D), dtype=torch.float32, device=dev) if res is not x else x
        h2 = torch.empty((n * Hq * Wq, D), dtype=torch.float16, device=dev) if P.ln_out else None
        K.gemm(a, B["wo"], bias=B["bo"], res=res, out=xo, ln_out=(h2, B["g2"], B["b2"], self.cfg.eps) if P.ln_out else None)
        return xo, h2

    def fpn(self, stages, stages16=None, lowest=0):
        """-> the three highest-resolution levels; lowest: levels below it are not computed (None)."""
        cfg = self.cfg
        nlev = len(stages) - 1
        feats, prev = [None] * (nlev + 1), None
        for i in range(nlev, lowest - 1, -1):
            s = stages[i]
            n, H, W, C = s.shape
            a = stages16[i] if stages16 and stages16[i] is not None else K.cast_f16(s.view(-1, C))
            w, b = self.neck[i]
            out = torch.empty((n, H, W, cfg.fpn_dim), dtype=torch.float16, device=s.device)
            if i not in cfg.fpn_top_down or i == nlev:
                K.gemm(a, w, bias=b, out=out.view(-1, cfg.fpn_dim))
            else:
                up = torch.empty((n, H, W, cfg.fpn_dim), dtype=torch.float16, device=s.device)
                K.upsample2(prev, up)
                K.gemm(a, w, bias=b, res=up.view(-1, cfg.fpn_dim), out=out.view(-1, cfg.fpn_dim))
            prev = out
            feats[i] = out
        return feats[:3]

    def encode_patches(self, patches, n):
        stages, stages16 = self.trunk(patches, n)
        return dict(fpn=self.fpn(stages, stages16), stages=stages)

    def encode(self, frames, precision=None, outputs="all"):
        """outputs="all": every FPN level and stage output.  "embedding": what the mask decoder reads — fpn[2], stages[2:] and
        `resized`; fpn[0], fpn[1] and the first two stage outputs are None: neither their lateral convolutions nor their f16 copies
        (nor, with a band, their joins) run.
        (precision is accepted for interface parity with SamVitEncoder and ignored: the Hiera trunk has one plan, f16
        operands, which meets north_star's mask bar with margin — 0.9996 raw-frame IoU with the exact decoder.)"""
        if outputs not in ("all", "embedding"):
            raise ValueError(f"outputs {outputs!r}: expected 'all' or 'embedding'")
        lowest = 2 if outputs == "embedding" else 0
        n, h, w, _ = frames.shape
        nh, nw = self._tables(h, w)[:2]
        plan = whole = None
        if self.band == "blocks":
            band, plan, whole = self._settle(nh, nw, n, lowest)
            band, top = (band, band[0]) if plan else (0, 0)
        else:
            band = top = self.band_rows(nh, nw) if self.band else 0
        table = self._band_table(frames, nh, nw, band, whole) if band else None
        img, patches = self.preprocess(frames, top)
        stages, stages16 = self.trunk(patches, n, band, table, lowest, plan=plan)
        return dict(fpn=self.fpn(stages, stages16, lowest), stages=stages, resized=img)


# ======================================================================================================================
# SAM v1 ImageEncoderViT — what `sam_model_registry["vit_b"|"vit_l"]` builds in services/sam3-pipeline/app/main.py:58-65
# (SURVEY.md Appendix A.2).  vit_h has head dim 80: the attention kernel's 96-wide head-dim class (csrc/attn.hip HDW).
# ======================================================================================================================
@dataclass
class SamVitConfig:
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    global_idx: tuple = (2, 5, 8, 11)
    window: int = 14
    patch: int = 16
    image: int = 1024
    out_ch: int = 256
    eps: float = 1e-6

    @property
    def grid(self):
        return self.image // self.patch


def sam_vit_b():
    return SamVitConfig()


def sam_vit_l():
    return SamVitConfig(hidden=1024, layers=24, heads=16, mlp=4096, global_idx=(5, 11, 17, 23))


def sam_vit_h():
    return SamVitConfig(hidden=1280, layers=32, heads=16, mlp=5120, global_idx=(7, 15, 23, 31))


def vit_param_spec(cfg):
    """Ordered {transformers SamModel `vision_encoder.*` parameter name: (shape, init kind)}."""
    D, hd, g = cfg.hidden, cfg.hidden // cfg.heads, cfg.grid
    s = {"vision_encoder.pos_embed": ((1, g, g, D), "tok"),
         "vision_encoder.patch_embed.projection.weight": ((D, 3, cfg.patch, cfg.patch), "w"),
         "vision_encoder.patch_embed.projection.bias": ((D,), "b")}
    for i in range(cfg.layers):
        p = f"vision_encoder.layers.{i}."
        S = g if i in cfg.global_idx else cfg.window
        s[p + "layer_norm1.weight"] = ((D,), "g")
        s[p + "layer_norm1.bias"] = ((D,), "b")
        s[p + "attn.rel_pos_h"] = ((2 * S - 1, hd), "b")
        s[p + "attn.rel_pos_w"] = ((2 * S - 1, hd), "b")
        s[p + "attn.qkv.weight"] = ((3 * D, D), "w")
        s[p + "attn.qkv.bias"] = ((3 * D,), "b")
        s[p + "attn.proj.weight"] = ((D, D), "w")
        s[p + "attn.proj.bias"] = ((D,), "b")
        s[p + "layer_norm2.weight"] = ((D,), "g")
        s[p + "layer_norm2.bias"] = ((D,), "b")
        s[p + "mlp.lin1.weight"] = ((cfg.mlp, D), "w")
        s[p + "mlp.lin1.bias"] = ((cfg.mlp,), "b")
        s[p + "mlp.lin2.weight"] = ((D, cfg.mlp), "w")
        s[p + "mlp.lin2.bias"] = ((D,), "b")
    s["vision_encoder.neck.conv1.weight"] = ((cfg.out_ch, D, 1, 1), "w")
    s["vision_encoder.neck.layer_norm1.weight"] = ((cfg.out_ch,), "g")
    s["vision_encoder.neck.layer_norm1.bias"] = ((cfg.out_ch,), "b")
    s["vision_encoder.neck.conv2.weight"] = ((cfg.out_ch, cfg.out_ch, 3, 3), "w")
    s["vision_encoder.neck.layer_norm2.weight"] = ((cfg.out_ch,), "g")
    s["vision_encoder.neck.layer_norm2.bias"] = ((cfg.out_ch,), "b")
    return s


class SamVitEncoder:
    """Device-resident SAM v1 image encoder: patch-embed GEMM (+abs pos), windowed (14x14, zero-padded 64->70) and global
    attention with decomposed relative-position bias, MLP, neck (1x1 -> LN2d -> 3x3 -> LN2d).  ``encode(frames)`` ->
    dict(fpn=[None, None, embedding f16 [n,64,64,256]], resized=...) — same shape contract as HieraEncoder for the decoder."""

    def __init__(self, cfg, state_dict, device="cuda", precision="exact"):
        """precision: the default plan of encode() — "exact" (services, adapters: every weight as the two-term f16 split
        [whi | wlo], one launch per Linear with lmx_k_gemm's a_rep = 2; f16 weights alone carry 3.9e-4 of the path's 9e-4
        relative logit error, profiles/r03_sam_vit_precision_probe.txt) or "f16" (throughput: 2x less MFMA work)."""
        if precision not in ("exact", "f16"):
            raise ValueError(f"precision {precision!r}: expected 'exact' or 'f16'")
        self.precision = precision
        self.cfg = cfg
        self.device = torch.device(device)
        dev = self.device
        sd = state_dict
        D, P = cfg.hidden, cfg.patch
        self._w32, self._w2 = {}, {}  # f32 [N, K] weights by key, and their [whi | wlo] f16 [N, 2K] form (built on first exact use)

        def t32(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def t16(a, key=None):
            if key is not None:
                self._w32[key] = np.ascontiguousarray(a, dtype=np.float32)
            return t32(a).to(torch.float16).contiguous()

        w = np.transpose(sd["vision_encoder.patch_embed.projection.weight"], (0, 2, 3, 1)).reshape(D, P * P * 3)
        self._w32["pe"] = np.ascontiguousarray(w, dtype=np.float32)
        self.k_pad = P * P * 3  # 768: already a multiple of 8
        self.pe_w, self.pe_b = t16(w), t32(sd["vision_encoder.patch_embed.projection.bias"])
        self.pos = t32(sd["vision_encoder.pos_embed"].reshape(cfg.grid * cfg.grid, D))
        self.layers = []
        for i in range(cfg.layers):
            p = f"vision_encoder.layers.{i}."
            qb = sd[p + "attn.qkv.bias"]
            self.layers.append(dict(
                glob=i in cfg.global_idx,
                g1=t32(sd[p + "layer_norm1.weight"]), b1=t32(sd[p + "layer_norm1.bias"]),
                wqkv=t16(sd[p + "attn.qkv.weight"], f"{i}.qkv"), bqkv=t32(qb), padkv=t16(qb),
                rh=t32(sd[p + "attn.rel_pos_h"]), rw=t32(sd[p + "attn.rel_pos_w"]),
                wo=t16(sd[p + "attn.proj.weight"], f"{i}.proj"), bo=t32(sd[p + "attn.proj.bias"]),
                g2=t32(sd[p + "layer_norm2.weight"]), b2=t32(sd[p + "layer_norm2.bias"]),
                w1=t16(sd[p + "mlp.lin1.weight"], f"{i}.fc1"), bb1=t32(sd[p + "mlp.lin1.bias"]),
                w2=t16(sd[p + "mlp.lin2.weight"], f"{i}.fc2"), bb2=t32(sd[p + "mlp.lin2.bias"])))
        self.n1_w = t16(sd["vision_encoder.neck.conv1.weight"][:, :, 0, 0], "n1")
        self.n1_ln = (t32(sd["vision_encoder.neck.layer_norm1.weight"]), t32(sd["vision_encoder.neck.layer_norm1.bias"]))
        c2 = sd["vision_encoder.neck.conv2.weight"]
        self.n2_w = t16(np.transpose(c2, (0, 2, 3, 1)).reshape(c2.shape[0], -1), "n2")
        self.n2_ln = (t32(sd["vision_encoder.neck.layer_norm2.weight"]), t32(sd["vision_encoder.neck.layer_norm2.bias"]))
        self.lut = t32(sam_norm_lut())
        self._tabs = {}

    _tables = HieraEncoder._tables

    def preprocess(self, frames):
        n, h, w, _ = frames.shape
        nh, nw, th, tv = self._tables(h, w)
        img = K.pil_resize(frames, nw, nh, th, tv, swap_rb=False)
        S, P = self.cfg.image, self.cfg.patch
        return img, K.im2col_u8(img, self.lut, S, S, P, P, P, 0, self.k_pad)

    def _split2(self, key):
        """[whi | wlo] f16 [N, 2K] of the f32 weight `key`: whi = f16(w), wlo = f16(w - whi) (often subnormal: the f16 MFMA honours
        subnormal operands on gfx950, tools/mfma_denorm_probe.py) — w to 2^-22 relative, or 3e-8 absolute for tiny weights."""
        if key not in self._w2:
            w = self._w32[key]
            hi = w.astype(np.float16)
            lo = (w - hi.astype(np.float32)).astype(np.float16)
            self._w2[key] = torch.from_numpy(np.ascontiguousarray(np.concatenate([hi, lo], 1))).to(self.device)
        return self._w2[key]

    def embed(self, patches, n, precision=None):
        cfg = self.cfg
        precision = precision or self.precision
        if precision not in ("exact", "f16"):
            raise ValueError(f"precision {precision!r}: expected 'exact' or 'f16'")
        exact = precision == "exact"
        g, D, H = cfg.grid, cfg.hidden, cfg.heads
        hd = D // H
        rows = n * g * g

        def lin(a, w16, key, **kw):  # one launch either way: f16 weights, or a_rep = 2 over [whi | wlo]
            if exact:
                w2 = self._split2(key)
                if a.shape[1] % 64 == 0 and a.shape[0] >= 512 and w2.shape[0] >= 96 and w2.shape[0] % 8 == 0:
                    return K.gemm(a, w2, a_rep=2, **kw)
                # shapes outside the LDS-DMA kernel (toy configurations; ViT-B / L / H never get here): the same sum over an
                # explicit [a | a] copy
                return K.gemm(torch.cat([a, a], 1), w2, **kw)
            return K.gemm(a, w16, **kw)

        x = lin(patches, self.pe_w, "pe", bias=self.pe_b, res=self.pos, res_rows=g * g, out_dtype=torch.float32)
        for i, L in enumerate(self.layers):
            h = K.layernorm(x, L["g1"], L["b1"], cfg.eps)
            qkv = lin(h, L["wqkv"], f"{i}.qkv", bias=L["bqkv"])
            q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
            a = torch.empty((rows, D), dtype=torch.float16, device=x.device)
            if L["glob"]:
                K.attention(q, k, v, a, n, H, g * g, g * g, hd, hd ** -0.5, rel_pos=(L["rh"], L["rw"]))
            else:
                ws = cfg.window
                nW = (-(-g // ws)) ** 2
                K.attention(q, k, v, a, n * nW, H, ws * ws, ws * ws, hd, hd ** -0.5, window=dict(Gh=g, Gw=g, ws=ws, q_stride=1),
                            pad_k=L["padkv"][D:2 * D], pad_v=L["padkv"][2 * D:], rel_pos=(L["rh"], L["rw"]))
            lin(a, L["wo"], f"{i}.proj", bias=L["bo"], res=x, out=x)
            h2 = K.layernorm(x, L["g2"], L["b2"], cfg.eps)
            u = lin(h2, L["w1"], f"{i}.fc1", bias=L["bb1"], act=K.ACT_GELU)
            lin(u, L["w2"], f"{i}.fc2", bias=L["bb2"], res=x, out=x)
        # neck: 1x1 (no bias) -> LayerNorm2d -> 3x3 (no bias) -> LayerNorm2d
        y = lin(K.cast_f16(x), self.n1_w, "n1", out_dtype=torch.float32)
        y = K.layernorm(y, *self.n1_ln, 1e-6)
        y4 = y.view(n, g, g, cfg.out_ch)
        if exact:  # the 3x3 as two accumulating launches of the implicit GEMM (whi, then + wlo), f32 output, f32 embedding
            if "n2.hi" not in self._w2:
                w2 = self._split2("n2")
                Kc = w2.shape[1] // 2
                self._w2["n2.hi"], self._w2["n2.lo"] = w2[:, :Kc].contiguous(), w2[:, Kc:].contiguous()
            acc = K.conv3x3(y4, self._w2["n2.hi"], bias=None, act=K.ACT_NONE, out_dtype=torch.float32)
            acc = K.conv3x3(y4, self._w2["n2.lo"], bias=None, act=K.ACT_NONE, res=acc, out=acc)
            y = K.layernorm(acc.view(rows, cfg.out_ch), *self.n2_ln, 1e-6, out_dtype=torch.float32)
        else:
            y = K.conv3x3(y4, self.n2_w, bias=None, act=K.ACT_NONE)
            y = K.layernorm(y.view(rows, cfg.out_ch), *self.n2_ln, 1e-6)
        return y.view(n, g, g, cfg.out_ch)

    def encode(self, frames, precision=None, outputs="all"):
        """(outputs is accepted for interface parity with HieraEncoder: the embedding is all this encoder returns.)"""
        img, patches = self.preprocess(frames)
        return dict(fpn=[None, None, self.embed(patches, frames.shape[0], precision)], resized=img)
