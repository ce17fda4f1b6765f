"""The host half of the model-level C API for YOLO (include/lmx.h "MODEL level: YOLOv8"), without a GPU:
  * lmx_h_letterbox_geometry / lmx_h_letterbox_tables / lmx_h_conv_split_k (csrc/host_letterbox.cpp) against lmx/letterbox.py and
    lmx.kernels.split_k_for: equal field by field / np.array_equal, no tolerance;
  * the weight image lmx.native.write_yolo_image writes, read back by lmx_yolo_image_check_host (csrc/host_yolo_image.cpp), which derives
    the layer table from (scale, nc, keypoint shape) itself;
  * corrupted images: each is LMX_EINVAL with the offending field or tensor named, and the process survives."""
import dataclasses
import itertools
import random
import struct

import numpy as np
import pytest

from imagepatch import entry_offset as _entry_offset
from imagepatch import patch as _patch
from lmx import dino, native, weights, yolo
from lmx import kernels as K
from lmx import letterbox as LB

C = native.C
SIDES = [37, 53, 180, 270, 320, 360, 481, 640, 720, 1080, 1280, 1920]
GRID = list(itertools.product(SIDES, SIDES, [160, 320, 640], [True, False]))


def _same_geo(a, b):
    """field by field; the doubles by == (a dataclass compares its fields with ==, but say so explicitly)"""
    return all(getattr(a, f.name) == getattr(b, f.name) and type(getattr(a, f.name)) is type(getattr(b, f.name)) for f in dataclasses.fields(a))


def test_geometry_equals_python_on_the_grid():
    """Equal on the whole grid — and the cases the twin can get wrong are present in GRID, not hoped for:
      * `sw * r` (or `sh * r`) lands on .5 exactly, where Python's round goes to the EVEN neighbour and a round-half-up does not;
      * dh (or dw) is a half integer, k + .5: `dh - 0.1` and `dh + 0.1` are then the two values next to the .5 tie the LetterBox
        roundings exist for, and top != bottom (k and k + 1).  (dh is a multiple of .5, so dh +- 0.1 itself never equals .5: the tie is
        on dh.)"""
    ties = down_to_even = halves = 0
    for sh, sw, imgsz, auto in GRID:
        want = LB.geometry(sh, sw, imgsz, 32, auto)
        assert _same_geo(native.letterbox_geometry(sh, sw, imgsz, 32, auto), want), (sh, sw, imgsz, auto)
        r = min(imgsz / sh, imgsz / sw)
        for x in (sw * r, sh * r):
            if x % 1 == 0.5:
                ties += 1
                down_to_even += round(x) != int(x + 0.5)  # a round-half-up twin would differ here
        halves += want.top != want.oh - want.rh - want.top or want.left != want.ow - want.rw - want.left
    assert ties and down_to_even and halves, (ties, down_to_even, halves)


def test_geometry_equals_python_on_random_sizes():
    rng = random.Random(20240)
    for _ in range(48):
        sh, sw = rng.randint(17, 4096), rng.randint(17, 4096)
        for imgsz, auto in ((640, True), (320, False)):
            assert _same_geo(native.letterbox_geometry(sh, sw, imgsz, 32, auto), LB.geometry(sh, sw, imgsz, 32, auto)), (sh, sw, imgsz, auto)


# (sh, sw) -> (rh, rw): the service's downscale, non-integer factors, upscaling, destination = source +- 1, a source of 2 pixels
TABLE_PAIRS = [((1080, 1920), (360, 640)), ((1080, 1920), (180, 320)), ((481, 270), (320, 180)), ((720, 1280), (405, 719)), ((37, 53), (223, 320)),
               ((100, 100), (101, 99)), ((100, 100), (99, 101)), ((2, 2), (7, 9)), ((2, 640), (1, 320)), ((640, 2), (320, 3)), ((333, 517), (206, 320)),
               ((53, 37), (320, 223)), ((1, 1), (4, 4)), ((997, 251), (640, 161))]


@pytest.mark.parametrize("pair", TABLE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}to{p[1][0]}x{p[1][1]}")
def test_tables_equal_python(pair):
    (sh, sw), (rh, rw) = pair
    got, want = native.letterbox_tables(sh, sw, rh, rw), LB.resize_tables(sh, sw, rh, rw)
    for g, w, name in zip(got, want, ("xofs", "ialpha", "yofs", "ibeta")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def test_split_k_equals_python():
    seen, want_set = set(), set()
    for px, N, cin in itertools.product([25, 100, 400, 960, 3840, 15360, 61440], [16, 32, 64, 80, 128, 256, 512, 516], [16, 32, 48, 64, 256, 512]):
        want = K.split_k_for(px, N, 27 * cin, cin)
        got = native.conv_split_k(px, N, 27 * cin, cin)
        assert got == want, (px, N, cin)
        seen.add(got)
        want_set.add(want)
    # the grid reaches no split, the smallest split and the cap, and the twin returns every value Python returns on it
    assert seen == want_set and {1, 2, 8} <= seen, (seen, want_set)


def test_host_calls_refuse_bad_arguments():
    lib = native._lib.load()
    g = native.LetterboxGeo()
    err = lambda: lib.lmx_last_error().decode()
    assert lib.lmx_h_letterbox_geometry(0, 640, 640, 32, 1, C.byref(g)) == -1 and "frame size" in err()
    assert lib.lmx_h_letterbox_geometry(480, -3, 640, 32, 1, C.byref(g)) == -1 and "frame size" in err()
    assert lib.lmx_h_letterbox_geometry(480, 640, 640, 32, 1, None) == -1 and "out_host" in err()
    assert lib.lmx_h_letterbox_geometry(480, 640, 16, 32, 1, C.byref(g)) == -1 and "imgsz" in err()
    assert lib.lmx_h_letterbox_geometry(480, 640, 640, 0, 1, C.byref(g)) == -1 and "stride" in err()
    x, a = np.empty(8, np.int32), np.empty(16, np.int16)
    assert lib.lmx_h_letterbox_tables(0, 4, 8, 8, x.ctypes.data, a.ctypes.data, x.ctypes.data, a.ctypes.data) == -1 and "source size" in err()
    assert lib.lmx_h_letterbox_tables(4, 4, 8, 0, x.ctypes.data, a.ctypes.data, x.ctypes.data, a.ctypes.data) == -1 and "destination size" in err()
    assert lib.lmx_h_letterbox_tables(4, 4, 8, 8, x.ctypes.data, None, x.ctypes.data, a.ctypes.data) == -1 and "null output" in err()
    assert lib.lmx_h_conv_split_k(0, 64, 1728, 64) == -1 and "px_per_frame" in err()
    assert lib.lmx_h_conv_split_k(100, 64, 1728, -32) == -1 and "cin" in err()
    with pytest.raises(native.LmxError, match="imgsz"):
        native.letterbox_geometry(480, 640, 8)


# ---- the weight image ------------------------------------------------------------------------------------------------------
POSE_SHAPE = (17, 3)
CONFIGS = {
    "n": lambda: (yolo.YoloConfig("n", nc=80, imgsz=320), yolo.bn_stats_path("n")),
    "l": lambda: (yolo.YoloConfig("l", nc=80, imgsz=320), yolo.bn_stats_path("l")),
    "pose": lambda: (yolo.YoloConfig("n", nc=1, imgsz=320, kpt_shape=POSE_SHAPE), yolo.bn_stats_path("n", pose=True)),  # tests/test_gpu_yolo.py's
}


@pytest.fixture(scope="module")
def detectors():
    """{name: detector on the CPU}; the constructor launches no kernel."""
    out = {}
    for name, make in CONFIGS.items():
        cfg, bn = make()
        out[name] = yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7, bn), "cpu")
    return out


def _expected_tensors(det, plans):
    """What the image must hold, from the detector alone: det.w for the f16 plan; for the exact plan _PlanExact._w with the groups of
    its call site in forward_letterboxed — 9 x [ci] for 3 x 3 (its own rule), [c] * (2 + n) for C2f cv2, [c_] * 4 for SPPF cv2, the
    two concat halves for the C2f cv1 that reads a concat, one group otherwise."""
    T = det.table
    co = [m.get("c2", 0) for m in T]
    groups = {"model.12.cv1": [co[9], co[6]], "model.15.cv1": [co[12], co[4]], "model.18.cv1": [co[16], co[12]], "model.21.cv1": [co[19], co[9]],
              "model.9.cv2": [T[9]["c1"] // 2] * 4}
    for i, m in enumerate(T):
        if m["kind"] == "c2f":
            groups[f"model.{i}.cv2"] = [m["c2"] // 2] * (2 + m["n"])
    host = lambda t: np.ascontiguousarray(t.numpy())
    want = {"stem.w": host(det.w["model.0"][0]), "stem.b": host(det.w["model.0"][1])}
    exact = yolo._PlanExact(det)  # a plan of the test's own: nothing cached by the exporter
    for name, (w, b) in det.w.items():
        if name == "model.0":
            continue
        if "f16" in plans:
            want[f"f16.{name}.w"], want[f"f16.{name}.b"] = host(w), host(b)
        if "exact" in plans:
            x3, xb, sc = exact._w(name, groups.get(name))
            want[f"x3.{name}.w"], want[f"x3.{name}.b"], want[f"x3.{name}.s"] = host(x3), host(xb), host(sc)
    return want


@pytest.mark.parametrize("plans", [("f16", "exact"), ("f16",)], ids=["both", "f16only"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_image_round_trip(detectors, name, plans, tmp_path):
    det = detectors[name]
    cfg = det.cfg
    path = tmp_path / f"{name}.lmx"
    size = native.write_yolo_image(det, path, plans)
    raw = path.read_bytes()
    assert size == len(raw)
    info = native.check_yolo_image(path)
    k, ndim = cfg.kpt_shape or (0, 0)
    assert (chr(info.scale), info.nc, info.imgsz, info.kpt_k, info.kpt_ndim, info.plans, info.max_batch) == \
        (cfg.scale, cfg.nc, 320, k, ndim, 3 if len(plans) == 2 else 1, 0)
    magic, version, kind, cfg_bytes, n, dir_off, data_off, file_bytes = struct.unpack_from("<8sIIIIQQQ", raw, 0)
    assert (magic, version, kind, file_bytes, dir_off) == (b"LMXIMAGE", 1, native.KIND_YOLO, len(raw), 48 + cfg_bytes) and data_off % 64 == 0
    # the config block: ten integers, then the names blob
    ints = struct.unpack_from("<10i", raw, 48)
    nk_pad = (k * ndim + 3) // 4 * 4
    assert ints[:8] == (ord(cfg.scale), cfg.nc, (cfg.nc + 3) // 4 * 4, 320, k, ndim, nk_pad, info.plans) and ints[8] == cfg.nc
    blob = raw[88:88 + ints[9]]
    assert cfg_bytes == 40 + (ints[9] + 7) // 8 * 8 and raw[88 + ints[9]:48 + cfg_bytes] == b"\0" * (-ints[9] % 8)
    assert blob.endswith(b"\0") and [s.decode("utf-8") for s in blob[:-1].split(b"\0")] == [det.names[i] for i in range(cfg.nc)]
    # every tensor sits in the file bit for bit, at the 64-byte aligned offset its directory entry names
    want = _expected_tensors(det, plans)
    assert n == len(want)
    for i, (tname, a) in enumerate(want.items()):
        raw_name, dt, rank, *rest = struct.unpack_from("<48sII4iQQ", raw, dir_off + i * native.ENTRY_BYTES)
        off, nbytes = rest[4:]
        assert raw_name.rstrip(b"\0").decode() == tname and dt == native._DTYPE[a.dtype] and rank == a.ndim and tuple(rest[:rank]) == a.shape, tname
        assert off % 64 == 0 and off >= data_off and nbytes == a.nbytes and raw[off:off + nbytes] == a.tobytes(), tname


@pytest.mark.parametrize("scale", ["s", "m", "x"])
def test_layer_table_twin_on_the_other_scales(scale, tmp_path):
    """n and l have width / depth 0.25 / 0.33 and 1 / 1; s, m and x put 0.5, 0.75 and 1.25 through ceil(. / 8), 0.67 through the
    half-to-even round and 768 through max_ch.  The reader accepts the image only if its own layer table gives every tensor the shape
    Python's gave it; nc = 3 pads Detect's class rows.  No BatchNorm statistics: nothing is computed."""
    cfg = yolo.YoloConfig(scale, nc=3, imgsz=640)
    det = yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7), "cpu")
    path = tmp_path / f"{scale}.lmx"
    native.write_yolo_image(det, path, ("f16",))
    info = native.check_yolo_image(path)
    assert (chr(info.scale), info.nc, info.imgsz, info.plans) == (scale, 3, 640, 1)
    raw = path.read_bytes()
    n = struct.unpack_from("<I", raw, 20)[0]
    assert n == 2 + 2 * (len(det.w) - 1)  # the reader asked for every one of them: none is missing, none has another shape


def _corruptions(raw):
    """(id, bytes, the words lmx_last_error must contain) for a detection image that holds both plans"""
    data_off = struct.unpack_from("<Q", raw, 32)[0]
    names_bytes = struct.unpack_from("<i", raw, 48 + 36)[0]
    w, b = _entry_offset(raw, "f16.model.4.cv2.w"), _entry_offset(raw, "x3.model.22.cv3.1.2.s")
    off_w = struct.unpack_from("<Q", raw, w + 72)[0]
    return [
        ("magic", b"LMXIMAGF" + raw[8:], "magic"),
        ("version", _patch(raw, 8, "<I", native.VERSION + 1), "version"),
        ("kind", _patch(raw, 12, "<I", native.KIND_SAM), "kind"),
        ("cut_header", raw[:40], "header"),
        ("cut_data", raw[:data_off + (len(raw) - data_off) // 2], "file_bytes"),
        ("file_bytes_plus_one", _patch(raw, 40, "<Q", len(raw) + 1), "file_bytes"),
        ("file_bytes_minus_one", raw[:-1], "file_bytes"),
        ("tensor_missing", _patch(raw, w, "<2s", b"xx"), "missing tensor 'f16.model.4.cv2.w'"),
        ("wrong_shape", _patch(raw, w + 56, "<i", struct.unpack_from("<i", raw, w + 56)[0] + 8), "tensor 'f16.model.4.cv2.w' has rank 2 shape"),
        ("wrong_dtype", _patch(raw, w + 48, "<I", 1), "tensor 'f16.model.4.cv2.w' has dtype 1, expected f16"),
        ("wrong_dtype_scale", _patch(raw, b + 48, "<I", 2), "tensor 'x3.model.22.cv3.1.2.s' has dtype 2, expected f32"),
        ("offset_unaligned", _patch(raw, w + 72, "<Q", off_w + 8), "not a multiple of 64"),
        ("offset_before_data", _patch(raw, w + 72, "<Q", 0), "outside the data"),
        ("offset_past_end", _patch(raw, w + 72, "<Q", (len(raw) + 63) // 64 * 64), "outside the data"),
        ("nbytes", _patch(raw, w + 80, "<Q", struct.unpack_from("<Q", raw, w + 80)[0] + 2), "nbytes"),
        ("names_terminator", _patch(raw, 88 + names_bytes - 1, "<1s", b"x"), "names blob: the last name has no NUL"),
        ("names_count", _patch(raw, 48 + 32, "<i", 81), "n_names 81 is not nc 80"),
        ("names_fewer", _patch(raw, 88 + 6, "<1s", b"_"), "names blob holds 79"),  # "person\0" loses its terminator: 79 strings for 80 classes
        ("plan_mask_0", _patch(raw, 48 + 28, "<i", 0), "plans mask 0"),
        ("scale", _patch(raw, 48, "<i", ord("q")), "scale"),
    ]


def test_corrupted_images_are_refused(detectors, tmp_path):
    lib = native._lib.load()
    path = tmp_path / "n.lmx"
    native.write_yolo_image(detectors["n"], path)
    raw = path.read_bytes()
    cases = _corruptions(raw)
    # a pose image without (one tensor of) cv4; an f16-only image whose mask claims the exact plan
    pose = tmp_path / "pose.lmx"
    native.write_yolo_image(detectors["pose"], pose, ("f16",))
    praw = pose.read_bytes()
    cases.append(("pose_without_cv4", _patch(praw, _entry_offset(praw, "f16.model.22.cv4.1.0.w"), "<2s", b"xx"), "missing tensor 'f16.model.22.cv4.1.0.w'"))
    cases.append(("mask_claims_exact", _patch(praw, 48 + 28, "<i", 3), "missing tensor 'x3.model.1.w'"))
    assert len(cases) >= 14
    for name, data, word in cases:
        bad = tmp_path / f"{name}.lmx"
        bad.write_bytes(data)
        info = native.YoloInfo()
        rc = lib.lmx_yolo_image_check_host(str(bad).encode(), C.byref(info))
        msg = lib.lmx_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert word in msg, (name, msg)
        bad.unlink()
    # the process is alive and the intact images still read
    assert native.check_yolo_image(path).nc == 80 and native.check_yolo_image(pose).kpt_k == 17
    with pytest.raises(native.LmxError, match="cannot open"):
        native.check_yolo_image(tmp_path / "absent.lmx")


def test_each_reader_refuses_the_other_kind(detectors, tmp_path):
    cfg = dataclasses.replace(dino.dinov2_base(), layers=1)
    emb = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 31), "cpu")
    d, y = tmp_path / "dino.lmx", tmp_path / "yolo.lmx"
    native.write_dino_image(emb, d)
    native.write_yolo_image(detectors["n"], y, ("f16",))
    with pytest.raises(native.LmxError, match=r"yolo image: kind 1 is not YOLO"):
        native.check_yolo_image(d)
    with pytest.raises(native.LmxError, match=r"dino image: kind 2 is not DINO"):
        native.check_dino_image(y)
    assert native.check_dino_image(d).layers == 1 and native.check_yolo_image(y).plans == 1
