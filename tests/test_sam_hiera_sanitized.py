"""The reader of a Hiera SAM image (csrc/host_image.cpp, host_sam_image.cpp) parses untrusted bytes, and the block plan
(csrc/host_hiera_plan.cpp) fills arrays the caller sized from a count: both run once under AddressSanitizer and
UndefinedBehaviorSanitizer — as a stand-alone program (tests/sam_hiera_check_main.cpp), on the CPU, in a child process: nothing is
loaded into this interpreter.  The program reads the intact images and every corrupted file of tests/test_native_sam_hiera_host.py,
then plans the sweep of tests/test_hiera_plan_c_host.py (and what the plan refuses); it must exit 0 with an empty stderr (no sanitizer
report) and give, file by file and query by query, the return code, the message, the rows and the records liblmx.so gives."""
import ctypes as C
import dataclasses
import os
import subprocess

import test_hiera_plan_c_host as TP
import test_native_sam_hiera_host as TH
from lmx import kernels as K
from lmx import native, sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "sam_hiera_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_image.cpp", "host_sam_image.cpp",
                                                                                                       "host_hiera_plan.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FIELDS = [f for f, _ in native._lib.HieraBlock._fields_]


def _config_words(cfg):
    return [len(cfg.blocks), *cfg.blocks, *cfg.dims, *cfg.heads, *cfg.windows, len(cfg.global_blocks), *cfg.global_blocks, cfg.q_pool_stages, cfg.image]


def _library_check(path):
    lib = native._lib.load()
    rc = lib.lmx_sam_image_check_host(str(path).encode(), None)
    return rc, lib.lmx_last_error().decode() if rc else ""


def _library_plan(cfg, mode, args):
    """(return code, message, rows, records as flat integers) of the ctypes calls into liblmx.so"""
    lib = native._lib.load()
    c = K._hiera_config(cfg)
    nb = C.c_int(0)
    rc = lib.lmx_h_hiera_blocks(C.byref(c), C.byref(nb))
    if rc == 0:
        recs, rows = (native._lib.HieraBlock * nb.value)(), (C.c_int * nb.value)()
        if mode == 0:
            n, nh, nw, lowest = args
            rc = lib.lmx_h_hiera_plan(C.byref(c), n, nh, nw, lowest, recs, rows)
        else:
            n, lowest, given = args
            rows = (C.c_int * nb.value)(*given)
            rc = lib.lmx_h_hiera_plan_rows(C.byref(c), n, rows, lowest, recs)
    if rc:
        return rc, lib.lmx_last_error().decode(), [], []
    return 0, "", list(rows), [getattr(r, f) for r in recs for f in FIELDS]


def _queries():
    """[(cfg, mode, args)]: the sizes and batches of tests/test_hiera_plan_c_host.py for every configuration at every canvas, rows of
    the caller's, and what is refused"""
    out = []
    for name, base in TP.CONFIGS.items():
        for image in TP.IMAGES:
            cfg = dataclasses.replace(base, image=image)
            sizes = [sam.resize_longest_side(h, w, image) for h, w in TP.FRAMES] + [(nh, image) for nh in TP._heights(image)]
            for nh, nw in sizes:
                for n in TP.BATCHES:
                    for lowest in (0, 2):
                        out.append((cfg, 0, (n, nh, nw, lowest)))
    r8 = TP.R8
    for rows in ((152, 152, 152, 76, 76, 42, 64, 64), (256, 256, 256, 128, 128, 64, 64, 64), (152, 144, 152, 76, 76, 42, 64, 64),
                 (152, 152, 152, 76, 76, 70, 64, 64), (264, 256, 256, 128, 128, 64, 64, 64)):
        out.append((r8, 1, (2, 2, rows)))
    for change in (dict(blocks=(2, 2, 3, 0)), dict(global_blocks=(8,)), dict(image=1022), dict(windows=(8, 4, 0, 7)), dict(blocks=(60, 60, 60, 77))):
        out.append((dataclasses.replace(r8, **change), 0, (1, 576, 1024, 0)))
    for args in ((0, 576, 1024, 0), (1, 0, 1024, 0), (1, 576, 1028, 0), (1, 576, 1024, -1)):
        out.append((r8, 0, args))
    return out


def test_reader_and_plan_are_clean_under_asan_and_ubsan_and_agree_with_the_library(tmp_path):
    exe = tmp_path / "sam_hiera_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    model = TH.build()
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    # ---- the reader: the intact images, every corrupted file, an absent path
    files = []

    def add(name, data):
        p = tmp_path / f"{name}.lmx"
        p.write_bytes(data)
        files.append(p)

    raws = {}
    for name, plans in (("both", ("f16", "exact")), ("f16", ("f16",))):
        path = tmp_path / f"{name}_src.lmx"
        native.write_sam_image(*model, path, plans)
        raws[name] = path.read_bytes()
        path.unlink()
        add(f"{name}_intact", raws[name])
    cases = TH.corruptions(raws["both"], raws["f16"])
    for name, data, _ in cases:
        add(name, data)
    files.append(tmp_path / "absent.lmx")
    assert len(files) == 2 + len(cases) + 1 and len(cases) >= 35
    try:
        run = subprocess.run([str(exe), "check", *map(str, files)], capture_output=True, text=True)
        assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
        assert run.stderr == "", run.stderr[-2000:]
        lines = run.stdout.splitlines()
        assert len(lines) == len(files)
        outcomes = []
        for line, path in zip(lines, files):
            rc, shown, msg = line.split("\t", 2)
            want = _library_check(path)
            assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
            outcomes.append(int(rc))
        assert outcomes == [0, 0] + [-1] * (len(files) - 2), outcomes  # the intact images read, everything else is LMX_EINVAL
    finally:
        for p in files:
            p.unlink(missing_ok=True)

    # ---- the plan
    queries = _queries()
    assert len(queries) > 10000
    text = []
    for cfg, mode, args in queries:
        tail = [0, *args] if mode == 0 else [1, args[0], args[1], *args[2]]
        text.append(" ".join(str(int(v)) for v in _config_words(cfg) + tail))
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\n".join(text) + "\n")
    run = subprocess.run([str(exe), "plan", str(qfile)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(queries)
    refused = 0
    for line, (cfg, mode, args) in zip(lines, queries):
        rc, msg, rows, recs = line.split("\t")
        got = (int(rc), msg, [int(v) for v in rows.split()], [int(v) for v in recs.split()])
        assert got == _library_plan(cfg, mode, args), (cfg, mode, args, line)
        refused += got[0] != 0
    assert refused == 3 + 5 + 4
