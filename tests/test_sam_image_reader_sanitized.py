"""The SAM weight-image reader (csrc/host_image.cpp, host_sam_image.cpp) parses untrusted bytes, so it is run once under
AddressSanitizer and UndefinedBehaviorSanitizer — as a stand-alone program (tests/sam_image_check_main.cpp), on the CPU, in a child
process: nothing is loaded into this interpreter.  The program reads the intact images, every corrupted file of
tests/test_native_sam_host.py, a DINO and a YOLO image and an absent path; it must exit 0 with an empty stderr (no sanitizer report)
and give, file by file, the return code and the message liblmx.so gives.  The same program answers the arithmetic behind
lmx_sam_resized (which itself takes a handle, and so a device) for the sizes the service sees."""
import dataclasses
import os
import subprocess

import test_native_sam_host as TS
from imagepatch import entry_offset, patch
from lmx import dino, native, sam, weights, yolo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "sam_image_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_image.cpp", "host_sam_image.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _library(path):
    """(return code, message) of the ctypes call into liblmx.so"""
    lib = native._lib.load()
    rc = lib.lmx_sam_image_check_host(str(path).encode(), None)
    return rc, lib.lmx_last_error().decode() if rc else ""


def test_reader_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "sam_image_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)
    files = []

    def add(name, data):
        p = tmp_path / f"{name}.lmx"
        p.write_bytes(data)
        files.append(p)

    raws = {}
    for name in TS.CONFIGS:
        enc, dec = TS.build(name)
        path = tmp_path / f"{name}_src.lmx"
        native.write_sam_image(enc, dec, path, TS.PLANS[name])
        raws[name] = path.read_bytes()
        path.unlink()
        add(f"{name}_intact", raws[name])
    cases = TS._corruptions(raws["S64"])
    for name, data, _ in cases:
        add(name, data)
    r80 = raws["S80"]
    add("mask_claims_exact", patch(r80, TS.CFG_AT["plans"], "<i", 3))
    add("mask_claims_only_exact", patch(r80, TS.CFG_AT["plans"], "<i", 2))
    add("decoder_linear_missing", patch(r80, entry_offset(r80, "dec.f16.L1.i2t.o.w"), "<2s", b"xx"))
    # the other kinds' images, and a path that does not exist
    cfg = dataclasses.replace(dino.dinov2_base(), layers=1)
    native.write_dino_image(dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 31), "cpu"), tmp_path / "a_dino_image.lmx")
    ycfg = yolo.YoloConfig("n", nc=80, imgsz=320)
    native.write_yolo_image(yolo.YoloDetector(ycfg, yolo.synthetic_state_dict(ycfg, 7, yolo.bn_stats_path("n")), "cpu"), tmp_path / "a_yolo_image.lmx", ("f16",))
    files += [tmp_path / "a_dino_image.lmx", tmp_path / "a_yolo_image.lmx", tmp_path / "absent.lmx"]
    assert len(files) == 2 + len(cases) + 3 + 3 and len(cases) >= 20

    try:
        run = subprocess.run([str(exe), "check", *map(str, files)], capture_output=True, text=True)
        assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
        assert run.stderr == "", run.stderr[-2000:]
        lines = run.stdout.splitlines()
        assert len(lines) == len(files)
        outcomes = []
        for line, path in zip(lines, files):
            rc, shown, msg = line.split("\t", 2)
            want = _library(path)
            assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
            outcomes.append(int(rc))
        assert outcomes == [0, 0] + [-1] * (len(files) - 2), outcomes  # the intact images read, everything else is LMX_EINVAL
        # ResizeLongestSide.get_preprocess_shape, and the sizes at which int(x + 0.5) sits on a tie or next to one
        sizes = TS.RESIZED_SIZES + [(3, 2048), (1, 3000), (2047, 2048), (1365, 2048), (767, 1025)]
        args = [str(v) for hw in sizes for v in hw]
        run = subprocess.run([str(exe), "resized", "1024", *args], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
        got = [tuple(int(v) for v in line.split("\t")) for line in run.stdout.splitlines()]
        assert got == [sam.resize_longest_side(h, w, 1024) for h, w in sizes], got
        assert got[:5] == [(576, 1024), (1024, 576), (1024, 1024), (1, 1024), (683, 1024)]
    finally:
        for p in files:
            p.unlink(missing_ok=True)
