"""The host half of GraphGPS — the weight-image reader (csrc/host_gnn_image.cpp over host_image.cpp) on whole, truncated and corrupted
images, the graph builder lmx_h_gnn_graph with both encodings, lmx_h_gnn_laplacian and lmx_h_gnn_forward
(csrc/host_gnn.cpp) — run under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/gnn_check_main.cpp), on
the CPU, in a child process: nothing is loaded into this interpreter and nothing goes near the GPU.  Every buffer of the program is
exactly as long as the header says it must be.  The program must exit 0 with an empty stderr (no sanitizer report) and print what
liblmx.so itself computes."""
import dataclasses
import os
import subprocess

import numpy as np
import torch

import gnnref
from lmx import checkpoints, gnn, native
from lmx import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vision-sam3-yolo-lameless_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "gnn_check_main.cpp")] + [os.path.join(CSRC, f) for f in ("host_gnn.cpp", "host_image.cpp", "host_gnn_image.cpp")]
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_host_gnn_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    exe = tmp_path / "gnn_check_main"
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    compiles = [subprocess.Popen(["g++", *FLAGS, "-c", s, "-o", o]) for s, o in zip(SOURCES, objects)]  # side by side: the slow part
    assert [c.wait() for c in compiles] == [0] * len(SOURCES)
    subprocess.run(["g++", *FLAGS, *objects, "-o", str(exe)], check=True)

    # the image reader over whole, truncated and corrupted files: the program prints what the library itself answers
    files = []
    for name, cfg in gnnref.CONFIGS.items():
        _, w = checkpoints.gnn_from_state_dict(gnnref.state_dict(cfg, 61), num_heads=cfg.n_heads, dropout=cfg.dropout)
        files.append(tmp_path / f"{name}.lmx")
        native.write_gnn_image(cfg, w, files[-1])
    bad = gnnref.bad_images(files[0].read_bytes())
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
        want_rc = lib.lmx_gnn_image_check_host(str(path).encode(), None)
        want = (want_rc, lib.lmx_last_error().decode() if want_rc else "")
        assert shown == str(path) and (int(rc), msg) == want, (path.name, line, want)
        outcomes.append(int(rc))
    assert outcomes == [0] * 3 + [-1] * (len(bad) + 1), outcomes

    g = torch.Generator().manual_seed(3)
    tiny = dataclasses.replace(gnnref.TINY, dropout=0.1)  # the program draws with p = 0.1
    for name, cfg, N, k, timed, S, seed in (("shipped", gnnref.SHIPPED, 1, 5, 1, 0, 5), ("shipped", gnnref.SHIPPED, 2, 5, 1, 2, 7),
                                            ("shipped", gnnref.SHIPPED, gnn.MAX_NODES, 5, 1, 0, 7), ("tiny", tiny, gnn.MAX_NODES, 5, 0, 2, 2 ** 63 + 12345),
                                            ("tiny", tiny, 17, 1, 1, 0, 1), ("wide", gnnref.WIDE, 33, 3, 0, 10, 9)):
        _, w = checkpoints.gnn_from_state_dict(gnnref.state_dict(cfg, 61), num_heads=cfg.n_heads, dropout=cfg.dropout)
        packed = gnn.pack_tensors(cfg, w)
        assert list(packed) == list(K.gnn_tensor_shapes(*cfg.shape()))
        weights, graph = tmp_path / "weights.bin", tmp_path / "graph.bin"
        weights.write_bytes(b"".join(v.tobytes() for v in packed.values()))
        x = torch.randn((N, cfg.input_dim), generator=g).numpy()
        emb = torch.randn((N, 9), generator=g).numpy()
        emb[N // 2] = emb[0]  # ties
        ts = 1.7e9 + (torch.rand((N,), generator=g).double() * 86400.0 * 5).numpy()
        ts[N // 2] = ts[0]
        graph.write_bytes(x.tobytes() + emb.tobytes() + ts.tobytes())
        run = subprocess.run([str(exe), ",".join(map(str, cfg.shape())), str(weights), str(graph), str(N), "9", str(k), str(timed), str(S), str(seed)],
                             capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (name, N, run.returncode, run.stderr[-2000:])

        gr = gnn.build_graph(cfg, x, emb, ts if timed else None, k)
        host = gnn.GnnScorer(cfg, w, backend="host")
        mc, stats, gp, node, attw, _ = host.forward([gr], [seed], S)
        hexes = lambda vals: " ".join(float(v).hex() for v in vals)  # noqa: E731
        want = [f"edge {s} {d} " + hexes(a) for (s, d), a in zip(gr["edges"], gr["edge_attr"])]
        want += [f"ptr {v}" for v in gr["csr_ptr"]] + [f"csr {v}" for v in gr["csr_edge"]]
        want += [f"node {d} " + hexes(list(a) + list(b)) for d, a, b in zip(gr["deg"], gr["lap"], gr["rw"])]
        want += [f"eigenvalue {float(v).hex()}" for v in K.gnn_laplacian(gr["edges"], N)[0]]
        if S:
            want += ["mc " + hexes(list(mc[i]) + list(stats[i])) for i in range(N)]
        else:
            want += [f"graph {float(gp[0]).hex()}"] + [f"eval {float(a).hex()} {float(b).hex()}" for a, b in zip(node, attw)]
        got = run.stdout.splitlines()
        assert len(got) == len(want), (name, N, len(got), len(want))
        for a, b in zip(got, want):
            ak, bk = a.split(), b.split()
            assert ak[0] == bk[0] and len(ak) == len(bk), (a, b)
            if ak[0] in ("ptr", "csr"):
                assert ak == bk, (a, b)
            else:
                first = {"edge": 3, "node": 2}.get(ak[0], 1)
                assert ak[:first] == bk[:first] and [float.fromhex(v) for v in ak[first:]] == [float.fromhex(v) for v in bk[first:]], (name, N, a, b)
