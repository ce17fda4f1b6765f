"""The host arithmetic of the fused record (csrc/host_records.cpp) fills arrays the caller sized from a count — the stream of each SAM
pass, the row map and its flags — so it runs once under AddressSanitizer and UndefinedBehaviorSanitizer: as a stand-alone program
(tests/fused_check_main.cpp), on the CPU, in a child process; nothing is loaded into this interpreter.  The program runs the layout,
stream-plan and row-map sweeps of tests/test_native_fused_host.py with what they refuse; it must exit 0 with an empty stderr (no
sanitizer report) and give, query by query, the return code, the message and the numbers liblmx.so gives."""
import ctypes as C
import itertools
import os
import subprocess

import test_native_fused_host as TF
from lmx import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "fused_check_main.cpp"), os.path.join(CSRC, "host_records.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _queries():
    """[[kind, *integers]]: 0 layout, 1 stream plan, 2 row map"""
    q = [[0, *a] for a in TF.layout_queries()]
    q += [[0, 0, 8, 384, 300, 0], [0, 8, 8, 0, 300, 1], [0, 8, 8, 384, -3, 0], [0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1]]
    q += [[1, n, s, ("lanes", "rr").index(lay)] for n, s, lay in TF.plan_queries()]
    q += [[1, 3, 4, 2], [1, -1, 4, 0], [1, 5, -7, 0], [1, 5, 2 ** 31 - 1, 1]]
    q += [[2, n, len(idx), *idx] for n, idx in TF.ROW_MAP_CASES]
    q += [[2, n, len(idx), *idx] for n, idx, _ in TF.BAD_ROW_MAPS]
    q += [[2, n, k, *idx] for n in range(0, 7) for k in range(n + 1) for idx in itertools.combinations(range(n), k)]
    q += [[2, -1, 0], [2, 3, -1]]
    return q


def _library(q):
    """(return code, message, the numbers as text) of the ctypes calls into liblmx.so"""
    lib = _lib.load()
    kind, a = q[0], q[1:]
    if kind == 0:
        lay = _lib.RecordLayout()
        rc = lib.lmx_h_record_layout(*a, C.byref(lay))
        words = [lay.stride] + [x for f in lay.fields[:lay.n_fields] for x in (f.name.decode(), f.dtype, f.ndim, f.shape[0], f.shape[1], f.offset, f.nbytes)]
    elif kind == 1:
        pool, det, emb = C.c_int(0), C.c_int(0), C.c_int(0)
        sam = (C.c_int32 * max(1, a[0]))()
        rc = lib.lmx_h_stream_plan(*a, C.byref(pool), C.byref(det), C.byref(emb), sam)
        words = [pool.value, det.value, emb.value] + list(sam)[:max(0, a[0])]
    else:
        n, k, idx = a[0], a[1], a[2:]
        m, ran = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
        rc = lib.lmx_h_row_map(n, (C.c_int32 * max(1, len(idx)))(*idx), k, b"det_idx", m, ran)
        words = list(m)[:max(0, n)] + list(ran)[:max(0, n)]
    if rc:
        return rc, lib.lmx_last_error().decode(), ""
    return 0, "", " ".join(str(w) for w in words)


def test_host_records_are_clean_under_asan_and_ubsan_and_agree_with_the_library(tmp_path):
    exe = tmp_path / "fused_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]
    queries = _queries()
    assert len(queries) > 500
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\n".join(" ".join(str(int(v)) for v in q) for q in queries) + "\n")
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), str(qfile)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(queries)
    refused = 0
    for line, q in zip(lines, queries):
        rc, msg, words = line.split("\t")
        assert (int(rc), msg, words) == _library(q), (q, line)
        refused += int(rc) != 0
    assert refused == 3 + 2 + len(TF.BAD_ROW_MAPS) + 2
