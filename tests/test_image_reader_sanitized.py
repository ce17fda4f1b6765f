"""The weight-image readers (csrc/host_image.cpp, host_dino_image.cpp, host_yolo_image.cpp) parse untrusted bytes, so they are run
once under AddressSanitizer and UndefinedBehaviorSanitizer — as a stand-alone program (tests/image_check_main.cpp), on the CPU, in a
child process: nothing is loaded into this interpreter.  The program reads the intact images, each image with the other kind's
reader, an absent path and every corrupted file of tests/test_native_dino_host.py and tests/test_native_yolo_host.py; it must exit
0 with an empty stderr (no sanitizer report) and give, file by file, the return code and the message liblmx.so gives."""
import dataclasses
import os
import subprocess

import test_native_dino_host as TD
import test_native_yolo_host as TY
from imagepatch import entry_offset, patch
from lmx import dino, native, weights, yolo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "image_check_main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                    ("host_image.cpp", "host_dino_image.cpp", "host_yolo_image.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# small networks of both architectures (learned positions / RoPE): the reader's work does not grow with the tensors' sizes
DINO_CONFIGS = {
    "dinov2": lambda: dataclasses.replace(dino.dinov2_base(), hidden=256, heads=4, mlp=1024, layers=2),
    "dinov3": lambda: dino.DinoConfig(hidden=256, heads=4, mlp=1024, layers=2),
}


def _library(check, path):
    """(return code, message) of the ctypes call into liblmx.so"""
    lib = native._lib.load()
    rc = getattr(lib, check)(str(path).encode(), None)
    return rc, lib.lmx_last_error().decode() if rc else ""


def test_readers_are_clean_under_asan_and_ubsan_and_agree_with_the_library(tmp_path):
    exe = tmp_path / "image_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)
    files = {"d": [], "y": []}

    def add(reader, name, data):
        p = tmp_path / f"{reader}_{name}.lmx"
        p.write_bytes(data)
        files[reader].append(p)

    intact = {}
    for arch, make in DINO_CONFIGS.items():
        cfg = make()
        emb = dino.DinoEmbedder(cfg, weights.synth_state_dict(dino.param_spec(cfg), 31), "cpu")
        path = tmp_path / f"{arch}.lmx"
        native.write_dino_image(emb, path)
        raw = intact[arch] = path.read_bytes()
        add("d", f"{arch}_intact", raw)
        for name, data, _ in TD._corruptions(cfg, raw):
            add("d", f"{arch}_{name}", data)
    dets = {}
    for name in ("n", "pose"):
        cfg, bn = TY.CONFIGS[name]()
        dets[name] = yolo.YoloDetector(cfg, yolo.synthetic_state_dict(cfg, 7, bn), "cpu")
    native.write_yolo_image(dets["n"], tmp_path / "n.lmx")
    native.write_yolo_image(dets["pose"], tmp_path / "pose.lmx", ("f16",))
    raw, praw = (tmp_path / "n.lmx").read_bytes(), (tmp_path / "pose.lmx").read_bytes()
    add("y", "n_intact", raw)
    add("y", "pose_intact", praw)
    for name, data, _ in TY._corruptions(raw):
        add("y", name, data)
    add("y", "pose_without_cv4", patch(praw, entry_offset(praw, "f16.model.22.cv4.1.0.w"), "<2s", b"xx"))
    add("y", "mask_claims_exact", patch(praw, 48 + 28, "<i", 3))
    # each image fed to the other kind's reader, and a path that does not exist
    add("y", "a_dino_image", intact["dinov2"])
    add("d", "a_yolo_image", praw)
    for reader in files:
        files[reader].append(tmp_path / "absent.lmx")
    assert len(files["d"]) == 2 * (1 + 16) + 2 and len(files["y"]) == 2 + 20 + 2 + 2

    try:
        for reader, check in (("d", "lmx_dino_image_check_host"), ("y", "lmx_yolo_image_check_host")):
            run = subprocess.run([str(exe), reader, *map(str, files[reader])], capture_output=True, text=True)
            assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
            assert run.stderr == "", run.stderr[-2000:]
            lines = run.stdout.splitlines()
            assert len(lines) == len(files[reader])
            outcomes = set()
            for line, path in zip(lines, files[reader]):
                rc, shown, msg = line.split("\t", 2)
                want = _library(check, path)
                assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
                outcomes.add(int(rc))
            assert outcomes == {0, -1}, outcomes  # the intact images read, everything else is LMX_EINVAL
    finally:
        for reader in files:
            for p in files[reader]:
                p.unlink(missing_ok=True)
