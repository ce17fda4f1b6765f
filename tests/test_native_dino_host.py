"""The host half of the model-level C API (include/lmx.h "MODEL level"), without a GPU:
  * lmx_h_pil_tables / lmx_h_aa_tables / lmx_h_identity_table / lmx_h_segment_cols (csrc/host_resample.cpp) against their Python
    restatements in lmx/resample.py, which the other tests pin against Pillow and torch: np.array_equal, no tolerance;
  * the weight image lmx.native.write_dino_image writes, read back by lmx_dino_image_check_host (csrc/host_dino_image.cpp);
  * corrupted images: each is LMX_EINVAL with the offending field named, and the process survives."""
import dataclasses
import struct

import numpy as np
import pytest

from imagepatch import entry_offset as _entry_offset
from imagepatch import patch as _patch
from lmx import dino, native, weights
from lmx import resample as R

# in -> out per axis: the service's 1080p frames to both recipes' sizes, odd sizes, an upscale, an unchanged axis, tiny axes, primes
PAIRS = [(1920, 455), (1080, 256), (1920, 224), (1080, 224), (481, 114), (270, 64), (100, 256), (256, 256), (7, 3), (3, 7), (1, 1), (997, 251)]
FILTERS = [R.BILINEAR, R.BICUBIC]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_pil_tables_equal_python(pair, filt):
    b, k, ks = native.pil_tables(*pair, filt)
    rb, rk, rks = R.coeff_tables(*pair, filt)
    assert ks == rks and b.dtype == rb.dtype and k.dtype == rk.dtype
    assert np.array_equal(b, rb) and np.array_equal(k, rk)
    assert native.segment_cols(b) == R.segment_cols(rb)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_aa_tables_equal_python(pair, filt):
    b, k, ks = native.aa_tables(*pair, filt)
    rb, rk, rks = R.aa_tables(*pair, filt)
    assert ks == rks and b.dtype == rb.dtype and k.dtype == rk.dtype == np.float32
    assert np.array_equal(b, rb)
    assert np.array_equal(k.view(np.uint32), rk.view(np.uint32)), "float32 weights differ in their bits"
    assert native.segment_cols(b) == R.segment_cols(rb)
    # the slice a centre crop keeps (what the model handle uploads), and a tile other than 256
    if pair[1] >= 224:
        o = int((pair[1] - 224) / 2.0)
        cut = rb.reshape(-1, 2)[o:o + 224].reshape(-1)
        assert native.segment_cols(cut) == R.segment_cols(cut)
    assert native.segment_cols(b, 7) == R.segment_cols(rb, 7)


@pytest.mark.parametrize("n", [1, 5, 1920])
def test_identity_table_equals_python(n):
    b, k, ks = native.identity_table(n)
    rb, rk, rks = dino._identity_table(n)
    assert ks == rks == 1 and np.array_equal(b, rb) and np.array_equal(k, rk) and b.dtype == rb.dtype and k.dtype == rk.dtype


def test_table_calls_refuse_bad_arguments():
    lib = native._lib.load()
    ks = native.C.c_int(0)
    assert lib.lmx_h_pil_tables(0, 4, 3, None, None, 0, native.C.byref(ks)) == -1 and b"in_size" in lib.lmx_last_error()
    assert lib.lmx_h_aa_tables(8, 4, 1, None, None, 0, native.C.byref(ks)) == -1 and b"filt" in lib.lmx_last_error()
    b, k = np.empty(8, np.int32), np.empty(3, np.int32)  # 4 outputs need 4 * ksize entries
    assert lib.lmx_h_pil_tables(8, 4, 3, b.ctypes.data, k.ctypes.data, k.size, native.C.byref(ks)) == -1
    assert b"kk_host" in lib.lmx_last_error() and ks.value == R.coeff_tables(8, 4, R.BICUBIC)[2]


# ---- the weight image ------------------------------------------------------------------------------------------------------
FLOAT_RECIPE = dino.DinoPreprocess(kind="float", filt=R.BILINEAR, shortest_edge=None, size_hw=(224, 224), crop=None)
CONFIGS = {
    "dinov2": lambda: dataclasses.replace(dino.dinov2_base(), layers=2),
    "dinov3": lambda: dataclasses.replace(dino.dinov3_vitl16(), layers=2, preproc=FLOAT_RECIPE),
}


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """{arch: (cfg, embedder on the CPU, path of its image, the image's bytes)}; the constructor launches no kernel."""
    out = {}
    for arch, make in CONFIGS.items():
        cfg = make()
        emb = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 31), "cpu")
        path = tmp_path_factory.mktemp("img") / f"{arch}.lmx"
        size = native.write_dino_image(emb, path)
        raw = path.read_bytes()
        assert size == len(raw)
        out[arch] = (cfg, emb, path, raw)
    return out


@pytest.mark.parametrize("arch", list(CONFIGS))
def test_image_round_trip(images, arch):
    cfg, emb, path, raw = images[arch]
    info = native.check_dino_image(path)
    assert (info.arch, info.hidden, info.heads, info.layers, info.tokens, info.image, info.patch, info.gated, info.recipe_kind, info.max_batch) == \
        (native.ARCH[cfg.arch], cfg.hidden, cfg.heads, 2, cfg.tokens, cfg.image, cfg.patch, int(cfg.gated), native.RECIPE[emb.recipe.kind], 0)
    # every tensor sits in the file bit for bit, at the 64-byte aligned offset its directory entry names
    tensors = native.dino_tensors(emb)
    magic, version, kind, cfg_bytes, n, dir_off, data_off, file_bytes = struct.unpack_from("<8sIIIIQQQ", raw, 0)
    assert (magic, version, kind, n, file_bytes) == (b"LMXIMAGE", 1, native.KIND_DINO, len(tensors), len(raw)) and data_off % 64 == 0
    assert n == 3 + (1 if cfg.arch == "dinov2" else 2) + 14 * 2 + 3
    for i, (name, a) in enumerate(tensors.items()):
        raw_name, dt, rank, *rest = struct.unpack_from("<48sII4iQQ", raw, dir_off + i * native.ENTRY_BYTES)
        off, nbytes = rest[4:]
        assert raw_name.rstrip(b"\0").decode() == name and rank == a.ndim and tuple(rest[:rank]) == a.shape
        assert off % 64 == 0 and off >= data_off and raw[off:off + nbytes] == a.tobytes()


def _corruptions(cfg, raw):
    """(id, bytes, the word lmx_last_error must contain)"""
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    gf = _entry_offset(raw, "gf")
    return [
        ("magic", b"LMXIMAGF" + raw[8:], "magic"),
        ("version", _patch(raw, 8, "<I", native.VERSION + 1), "version"),
        ("kind", _patch(raw, 12, "<I", native.KIND_SAM), "kind"),
        ("cut_header", raw[:40], "header"),
        ("cut_config", raw[:100], "header"),
        ("cut_directory", raw[:dir_off + 5 * native.ENTRY_BYTES + 17], "directory"),
        ("cut_data", raw[:data_off + (len(raw) - data_off) // 2], "file_bytes"),
        ("cut_last_byte", raw[:-1], "file_bytes"),
        ("offset_past_end", _patch(raw, gf + 72, "<Q", len(raw) + 64), "offset"),
        ("offset_wraps", _patch(raw, gf + 72, "<Q", 2 ** 64 - 64), "offset"),
        ("offset_in_directory", _patch(raw, gf + 72, "<Q", 0), "offset"),
        ("tensor_removed", _patch(raw, gf, "<2s", b"xx"), "missing tensor 'gf'"),
        ("hidden_changed", _patch(raw, 48 + 4, "<i", cfg.hidden + 8 * cfg.heads), "config block (hidden"),
        ("head_dim_128", _patch(raw, 48 + 8, "<i", cfg.hidden // 128), "head dim"),
        ("tokens_changed", _patch(raw, 48 + 40, "<i", cfg.tokens + 1), "tokens"),
        ("n_tensors_huge", _patch(raw, 20, "<I", 2 ** 20), "directory"),
    ]


@pytest.mark.parametrize("arch", list(CONFIGS))
def test_corrupted_images_are_refused(images, arch, tmp_path):
    cfg, emb, path, raw = images[arch]
    lib = native._lib.load()
    for name, data, word in _corruptions(cfg, raw):
        bad = tmp_path / f"{name}.lmx"
        bad.write_bytes(data)
        info = native.DinoInfo()
        rc = lib.lmx_dino_image_check_host(str(bad).encode(), native.C.byref(info))
        msg = lib.lmx_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert word in msg, (name, msg)
        with pytest.raises(native.LmxError, match="rc=-1"):
            native.check_dino_image(bad)
    # the process is alive and the intact image still reads
    assert native.check_dino_image(path).hidden == cfg.hidden
    with pytest.raises(native.LmxError, match="cannot open"):
        native.check_dino_image(tmp_path / "absent.lmx")
