"""The SAM weight image of a Hiera encoder (lmx.native.write_sam_image on a HieraEncoder, csrc/sam_image.h) without a GPU:
  * an image written from CPU-built HieraEncoder / MaskDecoder objects passes lmx_sam_image_check_host, holds every tensor the encoder
    holds bit for bit — the packed attention and MLP images included — and is the same file whatever the encoder's `band` setting;
  * corrupted images: each is LMX_EINVAL with the offending field or tensor named, and the process survives;
  * the exporter refuses an encoder not built the default way, naming the attribute;
  * a ViT image written by this tree is byte for byte the one the exporter wrote before it knew Hiera.
R8 is Hiera-B+ cut to eight blocks (tests/test_hiera_plan_c_host.py): image 1024, as the decoder's grid demands, and the B+ widths."""
import hashlib
import struct

import numpy as np
import pytest

import test_native_sam_host as TS
from imagepatch import entry_offset, patch
from lmx import kernels as K
from lmx import native, sam, sam_decoder, weights

C = native.C
R8 = sam.HieraConfig(blocks=(2, 2, 3, 1), global_blocks=(6,))
INTS = ("encoder", "hidden", "n_stages", "n_blocks", "n_global", "n_top_down", "q_pool_stages", "image", "fpn_dim", "plans", "pos_bkg0", "pos_bkg1")
CFG_AT = {n: 48 + 4 * i for i, n in enumerate(INTS)}
EPS_AT = 48 + 48
TAIL_AT = EPS_AT + 8  # blocks[4] dims[4] heads[4] windows[4] global_blocks[1] fpn_top_down[2], then 4 bytes of padding
ARR_AT = {n: TAIL_AT + 16 * i for i, n in enumerate(("blocks", "dims", "heads", "windows"))}
GLOBAL_AT, TOP_DOWN_AT, PAD_AT, CFG_BYTES = TAIL_AT + 64, TAIL_AT + 68, TAIL_AT + 76, 56 + 80
# sha256 of the ViT images of tests/test_native_sam_host.py (S64 with both plans, S80 with the f16 plan) as the exporter wrote them
# before it took a HieraEncoder: computed with the parent commit's lmx/native.py
VIT_SHA256 = {"S64": (44870336, "eedbe8756fd02c8d0944dda6808c947e03c69daf0244cf7f3daff72917218b58"),
              "S80": (22021312, "08493c4b84415306e306930ce0e5aba7515044db59476a48d372c653b6ae3c27")}


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for v in ("LMX_HIERA_ATTN8", "LMX_HIERA_ATTN4", "LMX_HIERA_ATTN_POOL", "LMX_HIERA_ATTN_POOL3", "LMX_MLP_IMG", "LMX_NO_FUSED_MLP"):
        monkeypatch.delenv(v, raising=False)


def state_dict():
    return weights.synth_state_dict(sam.param_spec(R8), 5)


def build(band="blocks", **kw):
    """(encoder, decoder) on the CPU; the constructors launch no kernel"""
    return sam.HieraEncoder(R8, state_dict(), "cpu", band=band, **kw), sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), "cpu")


@pytest.fixture(scope="module")
def model():
    return build()


@pytest.fixture(scope="module")
def image(model, tmp_path_factory):
    """(path, bytes) of the R8 image with both decoder plans"""
    path = tmp_path_factory.mktemp("sam_hiera_images") / "r8.lmx"
    size = native.write_sam_image(*model, path, ("f16", "exact"))
    raw = path.read_bytes()
    assert size == len(raw)
    return path, raw


def expected_encoder_tensors(enc):
    """{name: array} from the encoder's attributes alone"""
    host = lambda t: np.ascontiguousarray(t.numpy())
    want = {"enc.pe_w": host(enc.pe_w), "enc.pe_b": host(enc.pe_b), "enc.pos": host(enc.pos), "enc.lut": host(enc.lut)}
    for i, B in enumerate(enc.blocks):
        for n, t in B.items():
            if n in ("attn", "mlp_img"):
                for j, a in enumerate(t):
                    want[f"enc.B{i}.{n}.{j}"] = host(a)
            elif n not in ("dim", "dim_out", "heads", "win", "qs", "next_ln1"):
                want[f"enc.B{i}.{n}"] = host(t)
    for s in (2, 3):  # the levels outputs="embedding" reads
        want[f"enc.neck.{s}.w"], want[f"enc.neck.{s}.b"] = host(enc.neck[s][0]), host(enc.neck[s][1])
    return want


def test_image_round_trip(model, image):
    enc, dec = model
    path, raw = image
    info = native.check_sam_image(path)
    assert (info.encoder, info.hidden, info.heads, info.layers, info.mlp, info.window, info.patch, info.image, info.plans, info.max_batch) == \
        (2, 112, 2, 8, 0, 8, 16, 1024, 3, 0)
    assert info.image // info.patch == 64
    magic, version, kind, cfg_bytes, n, dir_off, data_off, file_bytes = struct.unpack_from("<8sIIIIQQQ", raw, 0)
    assert (magic, version, kind, file_bytes, dir_off, cfg_bytes) == (b"LMXIMAGE", 1, native.KIND_SAM, len(raw), 48 + CFG_BYTES, CFG_BYTES)
    assert native.VERSION == 1
    assert struct.unpack_from("<12i", raw, 48) == (2, 112, 4, 8, 1, 2, 3, 1024, 256, 3, 14, 14)
    assert struct.unpack_from("<d", raw, EPS_AT)[0] == R8.eps
    assert struct.unpack_from("<19i", raw, TAIL_AT) == (*R8.blocks, *R8.dims, *R8.heads, *R8.windows, 6, 2, 3) and raw[PAD_AT:48 + CFG_BYTES] == b"\0" * 4
    # every tensor the encoder holds sits in the file bit for bit; the decoder's entries are the ViT image's
    want = expected_encoder_tensors(enc)
    assert sum(k.startswith("enc.B") and ".attn." in k for k in want) == 4 + 4 + 2 + 2 + 2 and sum(".mlp_img." in k for k in want) == 2 * 4
    want.update({k: v for k, v in TS._expected_tensors(TS.build("S64")[0], dec, ("f16", "exact")).items() if k.startswith("dec.")})
    got = TS._directory(raw)
    assert set(got) == set(want), set(got) ^ set(want)
    for name, a in want.items():
        dt, shape, off, nbytes = got[name]
        assert dt == native._DTYPE[a.dtype] and shape == a.shape, (name, dt, shape, a.dtype, a.shape)
        assert off % 64 == 0 and off >= data_off and nbytes == a.nbytes, name
        assert np.array_equal(np.frombuffer(raw, a.dtype, a.size, off).reshape(a.shape).view(np.uint8), a.view(np.uint8)), name
    assert got["enc.B0.attn.0"][1] == (384, 128) and got["enc.B3.attn.0"][1] == (16, 16384) and got["enc.B2.attn.0"][1] == (14, 16384)
    assert got["enc.B4.attn.0"][1] == (47, 16384) and got["enc.B1.mlp_img.0"][1] == (7, 16384) and got["enc.B3.mlp_img.0"][1] == (28, 16384)


def test_writing_twice_and_every_band_setting_give_the_same_bytes(model, image, tmp_path):
    digest = hashlib.sha256(image[1]).digest()
    again = tmp_path / "again.lmx"
    native.write_sam_image(*model, again, ("f16", "exact"))
    assert hashlib.sha256(again.read_bytes()).digest() == digest
    for band in (True, False):  # the band changes no bit of the result and is not recorded
        native.write_sam_image(*build(band), again, ("f16", "exact"))
        assert hashlib.sha256(again.read_bytes()).digest() == digest, band


def test_a_vit_image_is_byte_for_byte_the_parents(tmp_path):
    for name, (size, sha) in VIT_SHA256.items():
        path = tmp_path / f"{name}.lmx"
        assert native.write_sam_image(*TS.build(name), path, TS.PLANS[name]) == size
        assert hashlib.sha256(path.read_bytes()).hexdigest() == sha, name
        assert native.check_sam_image(path).encoder == 0
        path.unlink()


def corruptions(raw, raw16):
    """(id, bytes, the words lmx_last_error must contain) for the R8 image with both plans; raw16: the same with the f16 plan only"""
    data_off = struct.unpack_from("<Q", raw, 32)[0]
    cfg = lambda field, value, base=raw: patch(base, CFG_AT[field], "<i", value)
    arr = lambda name, s, value, base=raw: patch(base, ARR_AT[name] + 4 * s, "<i", value)
    e = lambda name: entry_offset(raw, name)
    return [
        ("cut_data", raw[:data_off + (len(raw) - data_off) // 2], "file_bytes"),
        ("cut_config", raw[:100], "file"),
        ("encoder_kind_1", cfg("encoder", 1), "encoder 1 is not the SAM v1 ViT"),
        ("encoder_kind_3", cfg("encoder", 3), "encoder 3 is not the SAM v1 ViT"),
        # each config field against a number it must agree with, or against a tensor's shape
        ("hidden", cfg("hidden", 120), "hidden 120 is not dims[0] = 112"),
        ("hidden_and_dims0", arr("dims", 0, 120, cfg("hidden", 120)), "tensor 'enc.pe_w' has rank 2 shape [112, 152], the config block (hidden, 152) says rank 2 [120, 152]"),
        ("n_stages", cfg("n_stages", 5), "n_stages 5, n_global 1, n_top_down 2 call for 23 integers"),
        ("n_stages_2", cfg("n_stages", 2), "n_stages 2"),
        ("n_blocks", cfg("n_blocks", 9), "n_blocks 9 is not the sum of blocks[], 8"),
        ("blocks", cfg("n_blocks", 9, arr("blocks", 0, 3)), "tensor 'enc.B2.wqkv' has rank 2 shape [672, 112]"),
        ("blocks_0", arr("blocks", 3, 0), "blocks[3] = 0"),
        ("n_global", cfg("n_global", 3), "n_stages 4, n_global 3, n_top_down 2 call for 21 integers"),
        ("n_global_into_the_padding", cfg("n_global", 2), "global_blocks[1] = 2 does not ascend"),  # (the same 80 bytes: read on)
        ("n_top_down", cfg("n_top_down", 9), "n_top_down 9"),
        ("q_pool_stages", cfg("q_pool_stages", 1), "q_pool_stages 1"),
        ("image_512", cfg("image", 512), "image 512: the mask decoder reads an embedding of 64 x 64, image / 16 is 32"),
        ("image_1022", cfg("image", 1022), "image 1022"),
        ("fpn_dim_128", cfg("fpn_dim", 128), "fpn_dim 128 is not the mask decoder's width 256"),
        ("plan_mask_0", cfg("plans", 0), "plans mask 0"),
        ("mask_claims_exact", cfg("plans", 3, raw16), "missing tensor 'dec.x3.L0.sa.q.w'"),
        ("pos_bkg", cfg("pos_bkg1", 0), "pos_bkg 14 x 0"),
        ("eps", patch(raw, EPS_AT, "<d", float("nan")), "eps"),
        ("dims_2", arr("dims", 2, 512), "tensor 'enc.B4.wqkv' has rank 2 shape [1344, 224], the config block (3 * dims, dims (output, input width of the block)) says rank 2 [1536, 224]"),
        ("dims_3", arr("dims", 3, 1024), "tensor 'enc.B7.wqkv' has rank 2 shape [2688, 448]"),
        ("dims_not_heads", arr("heads", 3, 24), "dim 896 is not a multiple of heads 24"),
        # the head-dimension rule of the attention kernels: neither a fused kernel nor the launch path serves the block
        ("head_dim_112", arr("heads", 2, 4), "block 4: head dim 112 (dims 448 / heads 4) is not supported"),
        ("head_dim_28", arr("heads", 3, 32), "block 7: head dim 28"),
        ("windows_0", arr("windows", 2, 0), "stage 2: dims 448 heads 8 windows 0"),
        ("global_past_the_last_block", patch(raw, GLOBAL_AT, "<i", 8), "global_blocks[0] = 8 is not a block of 0 .. 7"),
        ("top_down", patch(raw, TOP_DOWN_AT, "<i", 7), "fpn_top_down[0] = 7 is not a stage of 0 .. 3"),
        ("padding", patch(raw, PAD_AT, "<i", 1), "padding behind the hiera config arrays"),
        # tensors
        ("packed_attention_missing", patch(raw, e("enc.B0.attn.0"), "<2s", b"xx"), "missing tensor 'enc.B0.attn.0'"),
        ("packed_pool_bias_missing", patch(raw, e("enc.B4.attn.1"), "<2s", b"xx"), "missing tensor 'enc.B4.attn.1'"),
        ("packed_attention_size", patch(patch(raw, e("enc.B3.attn.0") + 56, "<i", 32), e("enc.B3.attn.0") + 60, "<i", 8192),
         "tensor 'enc.B3.attn.0' has rank 2 shape [32, 8192], the config block (pack_hiera_attn4: 4 * heads images of 16384) says rank 2 [16, 16384]"),
        ("packed_mlp_missing", patch(raw, e("enc.B1.mlp_img.1"), "<2s", b"xx"), "missing tensor 'enc.B1.mlp_img.1'"),
        ("packed_mlp_nbytes", patch(raw, e("enc.B3.mlp_img.0") + 80, "<Q", 28 * 32768 - 2), "nbytes"),
        ("shortcut_missing", patch(raw, e("enc.B7.wp"), "<2s", b"xx"), "missing tensor 'enc.B7.wp'"),
        ("shortcut_dtype", patch(raw, e("enc.B2.wp") + 48, "<I", 1), "tensor 'enc.B2.wp' has dtype 1, expected f16"),
        ("neck_missing", patch(raw, e("enc.neck.2.w"), "<2s", b"xx"), "missing tensor 'enc.neck.2.w'"),
        ("position_table", patch(raw, e("enc.pos") + 56, "<i", 65528), "tensor 'enc.pos' has rank 2 shape"),
        ("decoder_norm_missing", patch(raw, e("dec.up_ln.g"), "<2s", b"xx"), "missing tensor 'dec.up_ln.g'"),
        ("offset_unaligned", patch(raw, e("enc.B5.w1") + 72, "<Q", struct.unpack_from("<Q", raw, e("enc.B5.w1") + 72)[0] + 8), "not a multiple of 64"),
    ]


@pytest.fixture(scope="module")
def image16(model, tmp_path_factory):
    path = tmp_path_factory.mktemp("sam_hiera_images16") / "r8_f16.lmx"
    native.write_sam_image(*model, path, ("f16",))
    return path, path.read_bytes()


def test_corrupted_images_are_refused(image, image16, tmp_path):
    lib = native._lib.load()
    path, raw = image
    cases = corruptions(raw, image16[1])
    assert len(cases) >= 35
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
    assert native.check_sam_image(path).plans == 3 and native.check_sam_image(image16[0]).plans == 1
    assert lib.lmx_sam_image_check_host(str(path).encode(), None) == 0


def test_the_exporter_refuses_an_encoder_not_built_the_default_way(model, tmp_path, monkeypatch):
    enc, dec = model
    out = tmp_path / "x.lmx"
    with pytest.raises(ValueError, match="fused_mlp"):
        native.write_sam_image(sam.HieraEncoder(R8, state_dict(), "cpu", fused_mlp=False), dec, out)
    with monkeypatch.context() as m:
        m.setenv("LMX_NO_FUSED_MLP", "1")
        switched = sam.HieraEncoder(R8, state_dict(), "cpu")
    with pytest.raises(ValueError, match="fused_mlp"):
        native.write_sam_image(switched, dec, out)
    no_ln = sam.HieraEncoder(R8, state_dict(), "cpu")
    no_ln.proj_ln = False
    with pytest.raises(ValueError, match="proj_ln"):
        native.write_sam_image(no_ln, dec, out)
    with monkeypatch.context() as m:
        m.setattr(K, "FUSED_MLP_WIDTHS", (112, 224, 448))  # what LMX_MLP448 does at import
        with pytest.raises(ValueError, match="FUSED_MLP_WIDTHS"):
            native.write_sam_image(enc, dec, out)
    with pytest.raises(native.LmxError, match="decoder for image 512 / grid 32"):
        native.write_sam_image(enc, sam_decoder.MaskDecoder(sam_decoder.synthetic_state_dict(6), "cpu", image_size=512, grid=32), out)
    with pytest.raises(native.LmxError, match="plans"):
        native.write_sam_image(enc, dec, out, ())
    assert not out.exists()
