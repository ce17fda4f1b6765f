"""The host half of the pose series — lmx_h_tleap_series and lmx_h_tleap_locomotion (csrc/host_tleap.cpp) over lmx_h_tcn_features
(csrc/host_tcn.cpp) and lmx_h_xfm_mask (csrc/host_xfm.cpp) — run under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program (tests/tleap_check_main.cpp), on the CPU, in a child process: nothing is loaded into this interpreter and nothing goes near the
GPU.  Every buffer of the program is exactly as long as the header says it must be.  The program must exit 0 with an empty stderr (no
sanitizer report) and print what liblmx.so itself computes."""
import os
import subprocess

import numpy as np
import torch

import tleapref as R
from lmx import _lib
from lmx import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "tleap_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_tleap.cpp", "host_tcn.cpp", "host_xfm.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COWS = [3, 19]


def _inputs(frame_counts, max_det, K_, ndim, seed):
    rng = np.random.default_rng(seed)
    F = len(frame_counts)
    boxes = rng.uniform(0, 1200, (F, max_det, 4)).astype(np.float32)
    boxes[..., 2:] = boxes[..., :2] + rng.uniform(0.2, 500, (F, max_det, 2)).astype(np.float32)
    scores = rng.uniform(0.3, 1, (F, max_det)).astype(np.float32)
    cls = rng.choice(np.array([0, 3, 7, 19], np.int32), (F, max_det)).astype(np.int32)
    kpts = None
    if K_:
        kpts = rng.uniform(0, 1300, (F, max_det, K_, ndim)).astype(np.float32)
        kpts[..., ndim - 1] = rng.uniform(0, 1, (F, max_det, K_)).astype(np.float32)
    return boxes, scores, cls, np.asarray(frame_counts, np.int32), kpts


def test_host_tleap_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "tleap_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    hexes = lambda vals: " ".join(float(v).hex() for v in vals)  # noqa: E731
    for K_, ndim, max_det, lengths, target, seed in ((0, 0, 3, [1, 9, 140], 125, 1), (20, 3, 4, [130, 2], 125, 2), (17, 2, 1, [5, 5, 5], 7, 3),
                                                     (23, 3, 2, [40], 125, 4), (0, 0, 1, [260], 125, 5)):
        counts = [(i * 3) % (max_det + 1) for i in range(sum(lengths))]
        boxes, scores, cls, counts, kpts = _inputs(counts, max_det, K_, ndim, seed)
        first = np.cumsum([0] + lengths).astype(np.int32)
        data = tmp_path / "input.bin"
        data.write_bytes(b"".join(a.tobytes() for a in (boxes, scores, cls, counts) + ((kpts,) if K_ else ()) + (first,)) + (b"" if K_ else np.asarray(COWS, np.int32).tobytes()))
        mode = K.TLEAP_TRAINED if K_ else K.TLEAP_HEURISTIC
        run = subprocess.run([str(exe), str(data), str(mode), str(K_), str(ndim), str(len(counts)), str(max_det), "720", "1280", str(len(lengths)),
                              str(target), "0" if K_ else str(len(COWS))], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (K_, run.returncode, run.stderr[-2000:])

        t = [torch.from_numpy(a) if a is not None else None for a in (boxes, scores, cls, counts, kpts)]
        rows, rec, series, mask = K.tleap_series(*t, (720, 1280), first, target, COWS, host=True)
        rec = rec.numpy().view(K.tleap_record_dtype()).reshape(-1)
        want = []
        for c in range(len(lengths)):
            want.append(f"rows {c} {int(rows[c])}")
            mine = rec[first[c] * max_det:first[c] * max_det + int(rows[c])]
            for r in mine:
                want.append(f"rec {r['frame']} {r['det']} {r['n_kp']} " + hexes(list(r["bbox"]) + [r["confidence"]] + list(r["keypoints"].reshape(-1))))
            for s in range(target):
                want.append(f"step {int(mask[c, s])} {sum(map(float, series[c, s])).hex()}")
            out = _lib.TleapLocomotion()
            loco = K.tleap_locomotion(mine, R.KEYPOINT_NAMES if K_ else R.HEURISTIC_NAMES)
            present = sum(1 << i for i, k in enumerate(out.KEYS) if k in loco)
            want.append(f"loco {present} " + hexes([loco.get(k, 0.0) for k in out.KEYS]))
        got = run.stdout.splitlines()
        assert len(got) == len(want), (K_, len(got), len(want))
        for a, b in zip(got, want):
            ak, bk = a.split(), b.split()
            first_float = {"rows": 3, "rec": 4, "step": 2, "loco": 2}[ak[0]]
            assert ak[:first_float] == bk[:first_float] and len(ak) == len(bk), (a, b)
            assert [float.fromhex(v) for v in ak[first_float:]] == [float.fromhex(v) for v in bk[first_float:]], (K_, a, b)
