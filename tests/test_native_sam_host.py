"""The host half of the model-level C API for SAM (include/lmx.h "MODEL level: SAM"), without a GPU:
  * the weight image lmx.native.write_sam_image writes from CPU-built SamVitEncoder / MaskDecoder objects, read back by
    lmx_sam_image_check_host (csrc/host_sam_image.cpp): the configuration, and every tensor bit for bit what the plans upload — the
    lazily built exact-plan tensors (SamVitEncoder._split2, MaskDecoder._x3) recomputed here from the float32 parameters;
  * corrupted images: each is LMX_EINVAL with the offending field or tensor named, and the process survives;
  * a DINO image and a YOLO image fed to the SAM reader.
lmx_sam_resized takes a handle, and a handle needs a device: its five sizes are held to ResizeLongestSide.get_preprocess_shape in
tests/test_gpu_native_sam.py, and the arithmetic behind it (lmx_sam_resized_hw) on the host in tests/test_sam_image_reader_sanitized.py.
Reduced encoders (image / patch / window 1024 / 16 / 14): S64 = hidden 192, 3 heads, windowed + global; S80 = hidden 320, 4 heads
(head dim 80), global + windowed."""
import dataclasses
import struct

import numpy as np
import pytest

from imagepatch import entry_offset as _entry_offset
from imagepatch import patch as _patch
from lmx import dino, native, sam, sam_decoder, weights, yolo
from lmx.exact import split_rows_x3

C = native.C
CONFIGS = {
    "S64": lambda: sam.SamVitConfig(hidden=192, heads=3, layers=2, mlp=384, global_idx=(1,)),
    "S80": lambda: sam.SamVitConfig(hidden=320, heads=4, layers=2, mlp=640, global_idx=(0,)),
}
PLANS = {"S64": ("f16", "exact"), "S80": ("f16",)}
RESIZED_SIZES = [(1080, 1920), (1920, 1080), (64, 64), (1, 1024), (683, 1024)]
CFG_AT = {n: 48 + 4 * i for i, n in enumerate(("encoder", "hidden", "heads", "layers", "mlp", "window", "patch", "image", "out_ch", "plans", "n_global",
                                                "reserved"))}
GLOBAL_IDX_AT = 48 + 48 + 8


def build(name):
    """(encoder, decoder) on the CPU; the constructors launch no kernel"""
    cfg = CONFIGS[name]()
    enc = sam.SamVitEncoder(cfg, weights.synth_state_dict(sam.vit_param_spec(cfg), 5), "cpu")
    return enc, sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), "cpu")


@pytest.fixture(scope="module")
def models():
    return {name: build(name) for name in CONFIGS}


@pytest.fixture(scope="module")
def images(models, tmp_path_factory):
    """{name: (path, bytes)}: S64 with both plans, S80 with the f16 plan only"""
    tmp = tmp_path_factory.mktemp("sam_images")
    out = {}
    for name, (enc, dec) in models.items():
        path = tmp / f"{name}.lmx"
        size = native.write_sam_image(enc, dec, path, PLANS[name])
        raw = path.read_bytes()
        assert size == len(raw)
        out[name] = (path, raw)
    return out


def _expected_tensors(enc, dec, plans):
    """{name: (dtype, shape, bytes or None)} from the two objects alone.  The f16 plan's tensors are the attributes __init__ uploaded;
    the exact plan's are recomputed from the float32 parameters the way _split2 and _lin build them."""
    host = lambda t: np.ascontiguousarray(t.numpy())
    want = {}
    put = lambda k, a: want.__setitem__(k, np.ascontiguousarray(a))

    def split2(key):
        w = enc._w32[key]
        hi = w.astype(np.float16)
        return np.concatenate([hi, (w - hi.astype(np.float32)).astype(np.float16)], 1)

    put("enc.pe_b", host(enc.pe_b)), put("enc.pos", host(enc.pos)), put("enc.lut", host(enc.lut))
    if "f16" in plans:
        put("enc.pe_w", host(enc.pe_w)), put("enc.n1.w", host(enc.n1_w)), put("enc.n2.w", host(enc.n2_w))
    if "exact" in plans:
        put("enc.x2.pe", split2("pe")), put("enc.x2.n1", split2("n1"))
        n2 = split2("n2")
        put("enc.x2.n2.hi", n2[:, :n2.shape[1] // 2]), put("enc.x2.n2.lo", n2[:, n2.shape[1] // 2:])
    for i, L in enumerate(enc.layers):
        for n in ("g1", "b1", "bqkv", "padkv", "rh", "rw", "bo", "g2", "b2", "bb1", "bb2") + (("wqkv", "wo", "w1", "w2") if "f16" in plans else ()):
            put(f"enc.L{i}.{n}", host(L[n]))
        if "exact" in plans:
            for n in ("qkv", "proj", "fc1", "fc2"):
                put(f"enc.x2.L{i}.{n}", split2(f"{i}.{n}"))
    for k, t in (("n1.g", enc.n1_ln[0]), ("n1.b", enc.n1_ln[1]), ("n2.g", enc.n2_ln[0]), ("n2.b", enc.n2_ln[1])):
        put("enc." + k, host(t))
    for k in ("gauss", "corner", "key_pe", "no_mask", "out_tokens", "point_embed", "not_a_point"):
        put("dec." + k, host(getattr(dec, k)))
    for i, L in enumerate(dec.layers):
        for j in range(1, 5):
            put(f"dec.L{i}.ln{j}.g", host(L[f"ln{j}"][0])), put(f"dec.L{i}.ln{j}.b", host(L[f"ln{j}"][1]))
    put("dec.ln_final.g", host(dec.ln_final[0])), put("dec.ln_final.b", host(dec.ln_final[1]))
    put("dec.up_ln.g", host(dec.up_ln[0])), put("dec.up_ln.b", host(dec.up_ln[1]))
    t = "mask_decoder.transformer."
    proj = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "out_proj"}
    lin = {}  # short name -> ((f16 w, f32 b) as uploaded, parameter prefix)
    for i, L in enumerate(dec.layers):
        for a, key, full in (("sa", "sa", "self_attn"), ("t2i", "t2i", "cross_attn_token_to_image"), ("i2t", "i2t", "cross_attn_image_to_token")):
            for s, p in proj.items():
                lin[f"L{i}.{a}.{s}"] = (L[key][p], f"{t}layers.{i}.{full}.{p}")
        lin[f"L{i}.lin1"], lin[f"L{i}.lin2"] = (L["w1"], f"{t}layers.{i}.mlp.lin1"), (L["w2"], f"{t}layers.{i}.mlp.lin2")
    for s, p in proj.items():
        lin[f"fin.{s}"] = (dec.final[p], f"{t}final_attn_token_to_image.{p}")
    lin["up1"], lin["up2"] = (dec.up1, "mask_decoder.upscale_conv1"), (dec.up2, "mask_decoder.upscale_conv2")
    for j, (s, p) in enumerate((("in", "proj_in"), ("mid", "layers.0"), ("out", "proj_out"))):
        lin[f"hyp0.{s}"] = (dec.hypers[0][j], f"mask_decoder.output_hypernetworks_mlps.0.{p}")
        lin[f"iou.{s}"] = (dec.iou_head[j], f"mask_decoder.iou_prediction_head.{p}")
    assert len(lin) == 2 * 14 + 4 + 2 + 6
    for short, ((w16, b32), prefix) in lin.items():
        if "f16" in plans:
            put(f"dec.f16.{short}.w", host(w16)), put(f"dec.f16.{short}.b", host(b32))
        if "exact" in plans:
            w, b = dec._sd[prefix + ".weight"], dec._sd[prefix + ".bias"]
            if short in ("up1", "up2"):
                w, b = np.transpose(w, (2, 3, 1, 0)).reshape(4 * w.shape[1], w.shape[0]), np.tile(b, 4)
            x3, sc, e = split_rows_x3(w, [w.shape[1]])
            put(f"dec.x3.{short}.w", x3), put(f"dec.x3.{short}.b", np.ldexp(b.astype(np.float32), e).astype(np.float32)), put(f"dec.x3.{short}.s", sc)
    return want


def _directory(raw):
    """{name: (dtype code, shape, offset, nbytes)} of an image"""
    n, dir_off = struct.unpack_from("<I", raw, 20)[0], struct.unpack_from("<Q", raw, 24)[0]
    out = {}
    for i in range(n):
        raw_name, dt, rank, *rest = struct.unpack_from("<48sII4iQQ", raw, dir_off + i * native.ENTRY_BYTES)
        out[raw_name.rstrip(b"\0").decode()] = (dt, tuple(rest[:rank]), rest[4], rest[5])
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_image_round_trip(models, images, name):
    enc, dec = models[name]
    cfg = enc.cfg
    path, raw = images[name]
    info = native.check_sam_image(path)
    mask = 3 if len(PLANS[name]) == 2 else 1
    assert (info.encoder, info.hidden, info.heads, info.layers, info.mlp, info.window, info.patch, info.image, info.plans, info.max_batch) == \
        (0, cfg.hidden, cfg.heads, cfg.layers, cfg.mlp, 14, 16, 1024, mask, 0)
    magic, version, kind, cfg_bytes, n, dir_off, data_off, file_bytes = struct.unpack_from("<8sIIIIQQQ", raw, 0)
    assert (magic, version, kind, file_bytes, dir_off) == (b"LMXIMAGE", 1, native.KIND_SAM, len(raw), 48 + cfg_bytes) and data_off % 64 == 0
    ints = struct.unpack_from("<12i", raw, 48)
    assert ints == (0, cfg.hidden, cfg.heads, cfg.layers, cfg.mlp, 14, 16, 1024, 256, mask, len(cfg.global_idx), 0)
    assert struct.unpack_from("<d", raw, 96)[0] == cfg.eps and struct.unpack_from("<i", raw, GLOBAL_IDX_AT)[0] == cfg.global_idx[0]
    assert cfg_bytes == 56 + 8 and raw[GLOBAL_IDX_AT + 4:48 + cfg_bytes] == b"\0" * 4
    # every tensor the plans upload sits in the file bit for bit, with its dtype and shape, at a 64-byte aligned offset
    want = _expected_tensors(enc, dec, PLANS[name])
    got = _directory(raw)
    assert set(got) == set(want), set(got) ^ set(want)
    for tname, a in want.items():
        dt, shape, off, nbytes = got[tname]
        assert dt == native._DTYPE[a.dtype] and shape == a.shape, (tname, dt, shape, a.dtype, a.shape)
        assert off % 64 == 0 and off >= data_off and nbytes == a.nbytes and raw[off:off + nbytes] == a.tobytes(), tname
    assert (got["enc.L0.rh"][1], got["enc.L1.rh"][1]) == (((27, 64), (127, 64)) if name == "S64" else ((127, 80), (27, 80)))


def test_the_exporter_builds_what_the_plans_build_lazily(models, tmp_path):
    """an encoder and a decoder whose lazy caches are already filled (as after an exact-plan run) export the same bytes as fresh ones"""
    enc, dec = build("S64")
    fresh, used = tmp_path / "fresh.lmx", tmp_path / "used.lmx"
    native.write_sam_image(enc, dec, fresh)
    from lmx.exact import split_rows_x3 as split

    name = "mask_decoder.transformer.layers.0.self_attn.q_proj"  # what MaskDecoder._x3 caches on its first use
    import torch

    w, b = dec._sd[name + ".weight"], dec._sd[name + ".bias"]
    x3, sc, e = split(w, [w.shape[1]])
    dec._wx[name] = (torch.from_numpy(x3), torch.from_numpy(np.ldexp(b.astype(np.float32), e).astype(np.float32)), torch.from_numpy(sc))
    native.write_sam_image(enc, dec, used)
    assert fresh.read_bytes() == used.read_bytes()
    with pytest.raises(native.LmxError, match="plans"):
        native.write_sam_image(enc, dec, tmp_path / "none.lmx", ())
    with pytest.raises(native.LmxError, match="plans"):
        native.write_sam_image(enc, dec, tmp_path / "bf16.lmx", ("bf16",))


def _corruptions(raw):
    """(id, bytes, the words lmx_last_error must contain) for the S64 image, which holds both plans"""
    data_off = struct.unpack_from("<Q", raw, 32)[0]
    w, s = _entry_offset(raw, "enc.L1.wqkv"), _entry_offset(raw, "dec.x3.iou.out.s")
    off_w = struct.unpack_from("<Q", raw, w + 72)[0]
    cfg = lambda field, value, base=raw: _patch(base, CFG_AT[field], "<i", value)
    return [
        ("magic", b"LMXIMAGF" + raw[8:], "magic"),
        ("version", _patch(raw, 8, "<I", native.VERSION + 1), "version"),
        ("kind", _patch(raw, 12, "<I", native.KIND_YOLO), "kind 2 is not SAM"),
        ("cut_header", raw[:40], "header"),
        ("cut_data", raw[:data_off + (len(raw) - data_off) // 2], "file_bytes"),
        ("file_bytes_plus_one", _patch(raw, 40, "<Q", len(raw) + 1), "file_bytes"),
        ("dir_offset_past_end", _patch(raw, 24, "<Q", len(raw) - 8), "directory"),
        ("offset_past_end", _patch(raw, w + 72, "<Q", (len(raw) + 63) // 64 * 64), "tensor 'enc.L1.wqkv' has offset"),
        ("offset_unaligned", _patch(raw, w + 72, "<Q", off_w + 8), "not a multiple of 64"),
        ("nbytes", _patch(raw, w + 80, "<Q", struct.unpack_from("<Q", raw, w + 80)[0] + 2), "nbytes"),
        ("tensor_renamed", _patch(raw, w, "<2s", b"xx"), "missing tensor 'enc.L1.wqkv'"),
        ("wrong_dtype", _patch(raw, w + 48, "<I", 1), "tensor 'enc.L1.wqkv' has dtype 1, expected f16"),
        ("wrong_dtype_scale", _patch(raw, s + 48, "<I", 2), "tensor 'dec.x3.iou.out.s' has dtype 2, expected f32"),
        ("wrong_shape", _patch(raw, w + 56, "<i", struct.unpack_from("<i", raw, w + 56)[0] + 8), "tensor 'enc.L1.wqkv' has rank 2 shape"),
        ("shape_against_config", cfg("mlp", 448), "tensor 'enc.L0.bb1' has rank 1 shape [384], the config block (mlp) says rank 1 [448]"),
        ("relpos_against_global_idx", _patch(raw, GLOBAL_IDX_AT, "<i", 0), "tensor 'enc.L0.rh' has rank 2 shape [27, 64]"),
        ("head_dim_100", cfg("heads", 4, cfg("hidden", 400)), "head dim 100"),
        ("hidden_not_heads", cfg("heads", 5), "hidden 192 is not a multiple of heads 5"),
        ("global_idx_beyond_layers", _patch(raw, GLOBAL_IDX_AT, "<i", 2), "global_idx[0] = 2 is not a layer"),
        ("n_global", cfg("n_global", 3), "n_global 3"),
        ("encoder_kind", cfg("encoder", 1), "encoder 1 is not the SAM v1 ViT"),
        ("plan_mask_0", cfg("plans", 0), "plans mask 0"),
        ("out_ch", cfg("out_ch", 128), "out_ch 128"),
        ("exact_hidden_160", cfg("heads", 2, cfg("hidden", 160)), "the exact plan needs hidden 160"),
        ("exact_mlp", cfg("mlp", 392), "the exact plan needs mlp 392"),
        ("eps", _patch(raw, 96, "<d", float("nan")), "eps"),
    ]


def test_corrupted_images_are_refused(images, tmp_path):
    lib = native._lib.load()
    path, raw = images["S64"]
    p80, raw80 = images["S80"]
    cases = _corruptions(raw)
    # an f16-only image whose mask claims the exact plan; the same image without one tensor of the decoder's f16 plan
    cases.append(("mask_claims_exact", _patch(raw80, CFG_AT["plans"], "<i", 3), "missing tensor 'enc.x2.pe'"))
    cases.append(("mask_claims_only_exact", _patch(raw80, CFG_AT["plans"], "<i", 2), "missing tensor 'enc.x2.pe'"))
    cases.append(("decoder_linear_missing", _patch(raw80, _entry_offset(raw80, "dec.f16.L1.i2t.o.w"), "<2s", b"xx"), "missing tensor 'dec.f16.L1.i2t.o.w'"))
    for name, data, word in cases:
        bad = tmp_path / f"{name}.lmx"
        bad.write_bytes(data)
        info = native.SamInfo()
        rc = lib.lmx_sam_image_check_host(str(bad).encode(), C.byref(info))
        msg = lib.lmx_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert word in msg, (name, msg)
        bad.unlink()
    # the process is alive and the intact images still read
    assert native.check_sam_image(path).plans == 3 and native.check_sam_image(p80).hidden == 320
    assert lib.lmx_sam_image_check_host(str(path).encode(), None) == 0
    with pytest.raises(native.LmxError, match="cannot open"):
        native.check_sam_image(tmp_path / "absent.lmx")


def test_the_sam_reader_refuses_the_other_kinds(images, tmp_path):
    cfg = dataclasses.replace(dino.dinov2_base(), layers=1)
    emb = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 31), "cpu")
    ycfg = yolo.YoloConfig("n", nc=80, imgsz=320)
    det = yolo.YoloDetector(ycfg, yolo.synthetic_state_dict(ycfg, 7, yolo.bn_stats_path("n")), "cpu")
    d, y = tmp_path / "dino.lmx", tmp_path / "yolo.lmx"
    native.write_dino_image(emb, d)
    native.write_yolo_image(det, y, ("f16",))
    with pytest.raises(native.LmxError, match=r"sam image: kind 1 is not SAM"):
        native.check_sam_image(d)
    with pytest.raises(native.LmxError, match=r"sam image: kind 2 is not SAM"):
        native.check_sam_image(y)
    with pytest.raises(native.LmxError, match=r"yolo image: kind 3 is not YOLO"):
        native.check_yolo_image(images["S80"][0])
    with pytest.raises(native.LmxError, match=r"dino image: kind 3 is not DINO"):
        native.check_dino_image(images["S80"][0])


def test_a_decoder_for_another_grid_is_not_exported(models, tmp_path):
    enc, _ = models["S64"]
    dec32 = sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), "cpu", image_size=512, grid=32)
    with pytest.raises(native.LmxError, match="decoder for image 512 / grid 32"):
        native.write_sam_image(enc, dec32, tmp_path / "x.lmx")
