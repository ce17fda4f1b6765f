"""The host half of the TCN gait model — the weight-image reader (csrc/host_tcn_image.cpp over host_image.cpp), lmx_h_tcn_features,
lmx_h_tcn_keep_bits and lmx_h_tcn_forward (csrc/host_tcn.cpp) — run once under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program (tests/tcn_check_main.cpp), on the CPU, in a child process: nothing is loaded into this interpreter and nothing
goes near the GPU.  The program must exit 0 with an empty stderr (no sanitizer report) and print what liblmx.so itself computes."""
import os
import struct
import subprocess

import numpy as np
import torch

import tcnref
from lmx import checkpoints, native, tcn
from lmx import kernels as K
from test_tcn_host import _pose_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "tcn_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_image.cpp", "host_tcn_image.cpp", "host_tcn.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_host_tcn_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "tcn_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    images = {}
    for i, (name, cfg) in enumerate(tcnref.CONFIGS.items()):
        _, folded = checkpoints.tcn_from_state_dict(tcnref.state_dict(cfg, 41 + i), cfg.dropout)
        images[name] = (cfg, folded, tmp_path / f"{name}.lmx")
        native.write_tcn_image(cfg, folded, images[name][2])
    raw = images["shipped"][2].read_bytes()
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    bad = {
        "cut_header": raw[:40], "cut_config": raw[:70], "cut_directory": raw[:dir_off + 3 * native.ENTRY_BYTES + 17],
        "cut_data": raw[:data_off + (len(raw) - data_off) // 2], "cut_last_byte": raw[:-1],
        "kind": raw[:12] + struct.pack("<I", native.KIND_YOLO) + raw[16:],
        "channels_24": raw[:48 + 16] + struct.pack("<i", 24) + raw[48 + 20:],
        "n_blocks_9": raw[:48 + 4] + struct.pack("<i", 9) + raw[48 + 8:],
        "n_blocks_negative": raw[:48 + 4] + struct.pack("<i", -3) + raw[48 + 8:],
        "k_4": raw[:48 + 8] + struct.pack("<i", 4) + raw[48 + 12:],
        "n_tensors_huge": raw[:20] + struct.pack("<I", 2 ** 20) + raw[24:],
        "offset_wraps": raw[:dir_off + 72] + struct.pack("<Q", 2 ** 64 - 64) + raw[dir_off + 80:],
        "p_nan": raw[:48 + 48] + struct.pack("<d", float("nan")) + raw[48 + 56:],
    }
    files = [p for _, _, p in images.values()]
    for name, data in bad.items():
        files.append(tmp_path / f"bad_{name}.lmx")
        files[-1].write_bytes(data)
    files.append(tmp_path / "absent.lmx")

    run = subprocess.run([str(exe), "check", *map(str, files)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(files)
    lib = native._lib.load()
    outcomes = []
    for line, path in zip(lines, files):
        rc, shown, msg = line.split("\t", 2)
        want_rc = lib.lmx_tcn_image_check_host(str(path).encode(), None)
        want = (want_rc, lib.lmx_last_error().decode() if want_rc else "")
        assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
        outcomes.append(int(rc))
    assert outcomes == [0] * 3 + [-1] * (len(bad) + 1), outcomes

    # features -> keep bits -> forward, on a pose file: the program prints what the library computes, bit for bit
    for name, T0, S, seed in (("shipped", 90, 10, 2 ** 63 + 12345), ("shipped", 300, 0, 7), ("deep", 1, 2, 1)):
        cfg, folded, path = images[name]
        frames = _pose_frames(T0, np.random.default_rng(T0))
        kp, nk, bb = np.zeros((T0, 20, 2)), np.zeros((T0,), np.int32), np.zeros((T0, 4))
        for t, f in enumerate(frames):
            nk[t] = len(f["keypoints"])
            kp[t, :nk[t]] = [[k["x"], k["y"]] for k in f["keypoints"]]
            bb[t] = f["bbox"]
        pose = tmp_path / "pose.bin"
        pose.write_bytes(kp.tobytes() + bb.tobytes() + nk.tobytes())
        run = subprocess.run([str(exe), "score", str(path), str(pose), str(T0), str(S), str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
        x = K.tcn_features(kp, nk, bb, 125)
        pred, stats, _ = tcn.TcnScorer(cfg, folded, backend="host").forward(torch.from_numpy(x)[None], [seed], S)
        want = [f"features {sum(map(float, x.flatten())).hex()}"]  # the program adds in this order, in doubles
        want += [f"site {s} kept {int(K.tcn_keep_bits(seed, max(S, 1) - 1, s, cfg.n_sites, 125 * 64, cfg.dropout).sum())}" for s in range(cfg.n_sites)]
        want += [f"pred {float(v).hex()}" for v in pred[0]] + [f"stats {float(stats[0, 0]).hex()} {float(stats[0, 1]).hex()}"]
        got = run.stdout.splitlines()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            gk, wk = g.split(), w.split()
            assert gk[0] == wk[0] and len(gk) == len(wk), (g, w)
            if gk[0] == "site":
                assert gk == wk, (g, w)
            else:
                assert [float.fromhex(v) for v in gk[1:]] == [float.fromhex(v) for v in wk[1:]], (g, w)
