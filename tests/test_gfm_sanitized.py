"""The host half of the graph transformer — the weight-image reader (csrc/host_gfm_image.cpp over host_image.cpp) on whole, truncated
and corrupted images, the graph builder lmx_h_gfm_graph and lmx_h_gfm_forward (csrc/host_gfm.cpp) — run under
AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/gfm_check_main.cpp), on the CPU, in a child process:
nothing is loaded into this interpreter and nothing goes near the GPU.  Every buffer of the program is exactly as long as the header
says it must be.  The program must exit 0 with an empty stderr (no sanitizer report) and print what liblmx.so itself computes."""
import dataclasses
import os
import subprocess

import numpy as np
import torch

import gfmref
from lmx import checkpoints, gfm, native
from lmx import kernels as K
from test_gfm_host import bad_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "gfm_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_gfm.cpp", "host_image.cpp", "host_gfm_image.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_host_gfm_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "gfm_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    # the image reader over whole, truncated and corrupted files: the program prints what the library itself answers
    files = []
    for name, cfg in gfmref.CONFIGS.items():
        _, w = checkpoints.gfm_from_state_dict(gfmref.state_dict(cfg, 61), num_heads=cfg.n_heads, dropout=cfg.dropout)
        files.append(tmp_path / f"{name}.lmx")
        native.write_gfm_image(cfg, w, files[-1])
    bad = bad_images(files[0].read_bytes())
    for name, data in bad.items():
        files.append(tmp_path / f"bad_{name}.lmx")
        files[-1].write_bytes(data)
    files.append(tmp_path / "absent.lmx")
    run = subprocess.run([str(exe), "check", *map(str, files)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(files)
    lib, outcomes = native._lib.load(), []
    for line, path in zip(lines, files):
        rc, shown, msg = line.split("\t", 2)
        want_rc = lib.lmx_gfm_image_check_host(str(path).encode(), None)
        want = (want_rc, lib.lmx_last_error().decode() if want_rc else "")
        assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
        outcomes.append(int(rc))
    assert outcomes == [0] * 3 + [-1] * (len(bad) + 1), outcomes

    g = torch.Generator().manual_seed(3)
    tiny = dataclasses.replace(gfmref.TINY, dropout=0.1)  # the program draws with p = 0.1
    for name, cfg, N, k, timed, S, seed in (("shipped", gfmref.SHIPPED, 1, 5, 1, 2, 5), ("shipped", gfmref.SHIPPED, 2, 5, 1, 0, 7),
                                            ("shipped", gfmref.SHIPPED, gfm.MAX_NODES, 5, 1, 0, 7), ("tiny", tiny, gfm.MAX_NODES, 200, 0, 2, 2 ** 63 + 12345),
                                            ("tiny", tiny, 17, 0, 1, 0, 1), ("wide", gfmref.WIDE, 33, 3, 0, 10, 9)):
        _, w = checkpoints.gfm_from_state_dict(gfmref.state_dict(cfg, 61), num_heads=cfg.n_heads, dropout=cfg.dropout)
        packed = gfm.pack_tensors(cfg, w)
        assert list(packed) == list(K.gfm_tensor_shapes(*cfg.shape()))
        weights, graph = tmp_path / "weights.bin", tmp_path / "graph.bin"
        weights.write_bytes(b"".join(v.tobytes() for v in packed.values()))
        x = torch.randn((N, cfg.input_dim), generator=g).numpy()
        emb = torch.randn((N, 9), generator=g).numpy()
        emb[N // 2] = emb[0]  # ties
        ts = (torch.rand((N,), generator=g) * 86400.0 * 500).numpy().astype(np.float32)
        ts[N // 2] = ts[0]
        graph.write_bytes(x.tobytes() + emb.tobytes() + ts.tobytes())
        target = N // 3
        run = subprocess.run([str(exe), ",".join(map(str, cfg.shape())), str(weights), str(graph), str(N), "9", str(k), str(timed), str(S), str(seed),
                              str(target)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (name, N, run.returncode, run.stderr[-2000:])

        gr = gfm.build_graph(cfg, x, emb, ts if timed else None, k)
        host = gfm.GfmScorer(cfg, w, backend="host")
        pred, stats, node, attn, _, _ = host.forward(host.batch([gr], [target] if S == 0 else None), [seed], S, node=S == 0)
        want = [f"edge {s} {d} " + " ".join(float(v).hex() for v in a) for (s, d), a in zip(gr["edges"], gr["edge_attr"])]
        want += [f"degree {a} {b}" for a, b in zip(gr["deg_in"], gr["deg_out"])]
        pos = np.arange(1, N * N + 1, dtype=np.int64)
        want += [f"matrices {int((gr['idx'].reshape(-1).astype(np.int64) * pos).sum())} {int(((gr['win'].reshape(-1).astype(np.int64) + 2) * pos).sum())}"]
        want += [f"pred {float(v).hex()}" for v in pred[0]] + [f"stats {float(stats[0, 0]).hex()} {float(stats[0, 1]).hex()}"]
        want += [f"node {float(a).hex()} {float(b).hex()}" for a, b in zip(node, attn)] if S == 0 else []
        got = run.stdout.splitlines()
        assert len(got) == len(want), (name, N, len(got), len(want))
        for a, b in zip(got, want):
            ak, bk = a.split(), b.split()
            assert ak[0] == bk[0] and len(ak) == len(bk), (a, b)
            if ak[0] in ("degree", "matrices"):
                assert ak == bk, (a, b)
            else:
                first = 3 if ak[0] == "edge" else 1
                assert ak[:first] == bk[:first] and [float.fromhex(v) for v in ak[first:]] == [float.fromhex(v) for v in bk[first:]], (name, N, a, b)
