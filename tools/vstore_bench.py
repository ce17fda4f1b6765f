"""Times the vector store's search (lmx_k_cosine_topk) on the GPU: galleries of 10^4, 10^5 and 10^6 rows at D = 1024, Q = 1, 8 and
64, top 5, beside torch.topk(G @ q.T, 5) in f32 on the same GPU and beside MemoryVectorStore.search (capped at 10^5 rows), and a
backlog of 64 through search_then_append beside 64 search-then-upsert steps over a store of 10^5.  Device events around warm,
alternating repeats; median and spread.  Writes what profiles/vstore_ab.txt holds.

    python tools/vstore_bench.py [--out FILE] [--max-rows 1000000]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lmx import kernels as K  # noqa: E402
from lmx import vstore  # noqa: E402
from lmx.services import runtime as R  # noqa: E402

D, TOPK, HBM, HBM_SPEC = 1024, 5, 6.3e12, 8.0e12


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def ab(fns, iters, repeats=7):
    """alternating repeats of the routes -> per route (median, min, max) seconds per call"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for t, fn in zip(times, fns):
            t.append(timed(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-rows", type=int, default=10 ** 6)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the vector store is measured on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    _, tile, _ = vstore.geometry(D)
    say(f"# {torch.cuda.get_device_name(dev)}; D = {D}, top {TOPK}; seconds per call: median [min .. max] over 7 alternating repeats")
    say(f"# bytes/s = N * D * 4 / time, for Q <= T = {tile} (one walk of the gallery); achievable HBM {HBM / 1e12} TB/s ({HBM_SPEC / 1e12} spec)")
    gen = torch.Generator(device=dev).manual_seed(0)
    for N in (10 ** 4, 10 ** 5, 10 ** 6):
        if N > args.max_rows:
            continue
        G = K.unit_rows(torch.randn((N, D), device=dev, generator=gen))
        for Q in (1, 8, 64):
            q = K.unit_rows(torch.randn((Q, D), device=dev, generator=gen))
            iters = max(3, min(200, int(2e9 / (N * D * 4 * max(1, Q // tile)))))
            (lmx, lo, hi), (tt, tlo, thi) = ab([lambda: K.cosine_topk(G, q, TOPK), lambda: torch.topk(G @ q.T, TOPK, dim=0)], iters)
            s1, i1 = K.cosine_topk(G, q, TOPK)
            s2, i2 = torch.topk(G @ q.T, TOPK, dim=0)
            agree = float((i1.long() == i2.T).float().mean())
            rate = f"  {N * D * 4 / lmx / 1e12:5.2f} TB/s = {N * D * 4 / lmx / HBM:4.0%} of achievable HBM" if Q <= tile else ""
            say(f"N {N:>8} Q {Q:>2}: lmx {lmx * 1e6:9.1f} us [{lo * 1e6:.1f} .. {hi * 1e6:.1f}]   torch G@q.T + topk {tt * 1e6:9.1f} us "
                f"[{tlo * 1e6:.1f} .. {thi * 1e6:.1f}]   x{tt / lmx:5.2f}   same slots {agree:.3f}{rate}")
        if N <= 10 ** 5:  # today's route: a Python loop over a dict (one timing; 10^6 rows would take 8 GB of float64 and tens of seconds)
            mem = R.MemoryVectorStore()
            host = G.cpu().numpy().astype(np.float64)
            for i in range(N):
                mem.points[i] = (host[i], {"video_id": str(i)})
            qh = K.unit_rows(torch.randn((1, D), device=dev, generator=gen)).cpu().numpy()[0].astype(np.float64)
            t0 = time.perf_counter()
            mem.search(qh, TOPK)
            say(f"N {N:>8} Q  1: MemoryVectorStore.search {time.perf_counter() - t0:.3f} s (one call)")
            del mem, host
        del G
    say("# MemoryVectorStore.search is capped at 10^5 rows: it grows linearly (a Python loop), 10^6 rows would be ten times the 10^5 figure")

    # a backlog of 64 over a store of 10^5: store calls only, the embeddings are given
    n0, B = min(10 ** 5, args.max_rows), 64
    rng = np.random.default_rng(1)
    store = vstore.DeviceVectorStore(dev, capacity=n0 + 4 * B)
    store.ensure_collection(D)
    store.append_many([f"old{i}" for i in range(n0)], rng.standard_normal((n0, D)).astype(np.float32), [{"video_id": f"old{i}"} for i in range(n0)])
    for tag in ("warm", "timed"):
        new = rng.standard_normal((2 * B, D))
        t0 = time.perf_counter()
        for j in range(B):
            store.search(new[j], TOPK)
            store.upsert(f"{tag}s{j}", new[j], {"video_id": f"{tag}s{j}"})
        t1 = time.perf_counter()
        store.search_then_append([f"{tag}b{j}" for j in range(B)], new[B:], [{"video_id": f"{tag}b{j}"} for j in range(B)], TOPK)
        t2 = time.perf_counter()
        if tag == "timed":
            say(f"backlog of {B} over {n0} rows, store calls only: {B} x (search, upsert) {1e3 * (t1 - t0):.2f} ms   search_then_append "
                f"{1e3 * (t2 - t1):.2f} ms   x{(t1 - t0) / (t2 - t1):.1f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
