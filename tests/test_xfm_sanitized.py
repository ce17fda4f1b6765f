"""The host half of the gait transformer — the weight-image reader (csrc/host_xfm_image.cpp over host_image.cpp), lmx_h_xfm_mask and
lmx_h_xfm_forward (csrc/host_xfm.cpp) and the features (csrc/host_tcn.cpp) — run once under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program (tests/xfm_check_main.cpp), on the CPU, in a child process: nothing is loaded into
this interpreter and nothing goes near the GPU.  The program must exit 0 with an empty stderr (no sanitizer report) and print what
liblmx.so itself computes."""
import os
import struct
import subprocess

import numpy as np
import torch

import xfmref
from lmx import checkpoints, native, xfm
from lmx import kernels as K
from test_xfm_host import _mask_arrays, _pose_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "xfm_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_image.cpp", "host_xfm_image.cpp", "host_xfm.cpp",
                                                                                                "host_tcn.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_host_xfm_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "xfm_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    images = {}
    for i, (name, cfg) in enumerate(xfmref.CONFIGS.items()):
        _, w = checkpoints.xfm_from_state_dict(xfmref.state_dict(cfg, 41 + i), n_heads=cfg.n_heads, dropout=cfg.dropout)
        images[name] = (cfg, w, tmp_path / f"{name}.lmx")
        native.write_xfm_image(cfg, w, images[name][2])
    raw = images["shipped"][2].read_bytes()
    dir_off, data_off = struct.unpack_from("<QQ", raw, 24)
    bad = {
        "cut_header": raw[:40], "cut_config": raw[:70], "cut_directory": raw[:dir_off + 3 * native.ENTRY_BYTES + 17],
        "cut_data": raw[:data_off + (len(raw) - data_off) // 2], "cut_last_byte": raw[:-1],
        "kind": raw[:12] + struct.pack("<I", native.KIND_TCN) + raw[16:],
        "d_model_24": raw[:48 + 4] + struct.pack("<i", 24) + raw[48 + 8:],
        "n_heads_0": raw[:48 + 8] + struct.pack("<i", 0) + raw[48 + 12:],
        "n_layers_9": raw[:48 + 12] + struct.pack("<i", 9) + raw[48 + 16:],
        "n_layers_negative": raw[:48 + 12] + struct.pack("<i", -3) + raw[48 + 16:],
        "ff_40": raw[:48 + 16] + struct.pack("<i", 40) + raw[48 + 20:],
        "max_len_100": raw[:48 + 24] + struct.pack("<i", 100) + raw[48 + 28:],
        "n_tensors_huge": raw[:20] + struct.pack("<I", 2 ** 20) + raw[24:],
        "offset_wraps": raw[:dir_off + 72] + struct.pack("<Q", 2 ** 64 - 64) + raw[dir_off + 80:],
        "p_nan": raw[:48 + 32] + struct.pack("<d", float("nan")) + raw[48 + 40:],
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
        want_rc = lib.lmx_xfm_image_check_host(str(path).encode(), None)
        want = (want_rc, lib.lmx_last_error().decode() if want_rc else "")
        assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
        outcomes.append(int(rc))
    assert outcomes == [0] * 3 + [-1] * (len(bad) + 1), outcomes

    # features and mask -> forward, on a pose file: the program prints what the library computes, bit for bit
    for name, T0, S, seed in (("shipped", 90, 10, 2 ** 63 + 12345), ("shipped", 300, 0, 7), ("wide", 1, 2, 1)):
        cfg, w, path = images[name]
        frames = _pose_frames(T0, np.random.default_rng(T0))
        kc, nk, dc = _mask_arrays(frames)
        kp, bb = np.zeros((T0, 20, 2)), np.zeros((T0, 4))
        for t, f in enumerate(frames):
            kp[t, :nk[t]] = [[k["x"], k["y"]] for k in f["keypoints"]]
            bb[t] = f["bbox"]
        pose = tmp_path / "pose.bin"
        pose.write_bytes(kp.tobytes() + bb.tobytes() + nk.tobytes() + kc.tobytes() + dc.tobytes())
        run = subprocess.run([str(exe), "score", str(path), str(pose), str(T0), str(S), str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
        x, mask = K.tcn_features(kp, nk, bb, 125), K.xfm_mask(kc, nk, dc, 125)
        pred, stats, sal, _ = xfm.XfmScorer(cfg, w, backend="host").forward(torch.from_numpy(x)[None], torch.from_numpy(mask)[None], [seed], S,
                                                                            saliency=S == 0)
        want = [f"features {sum(map(float, x.flatten())).hex()}", f"masked {int(mask.sum())}"]  # the program adds in this order, in doubles
        want += [f"pred {float(v).hex()}" for v in pred[0]] + [f"stats {float(stats[0, 0]).hex()} {float(stats[0, 1]).hex()}"]
        want += [f"saliency {float(v).hex()}" for v in sal[0]] if S == 0 else []
        got = run.stdout.splitlines()
        assert len(got) == len(want)
        for g, w_ in zip(got, want):
            gk, wk = g.split(), w_.split()
            assert gk[0] == wk[0] and len(gk) == len(wk), (g, w_)
            if gk[0] == "masked":
                assert gk == wk and 0 < int(gk[1]) < 125, (g, w_)
            else:
                assert [float.fromhex(v) for v in gk[1:]] == [float.fromhex(v) for v in wk[1:]], (g, w_)
