"""Stage-3 attention projection (+ the LayerNorm that follows it) of Hiera-B+ in two serialized kernel traces of bench.py
(LMX_SERIAL=1 rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps S --warmup W): the parent's
256 x 256 residual GEMM followed by layernorm_rows_kernel<1, 0, 2>, against gemm2_rowln_kernel (lmx_gemm_desc.ln_out), which writes
the LayerNorm rows itself.

usage: python tools/rowln_proj_ab.py parent_kernel_trace.csv this_kernel_trace.csv [passes_per_trace]
       python tools/rowln_proj_ab.py --hbm label fetch_counter_collection.csv write_counter_collection.csv
(--hbm: HBM bytes per launch from two counter runs of the same command, `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE`, each a run
of its own; both counters are in KiB and FETCH_SIZE is doubled, the gfx950 correction of tools/pmc_summary.py)

In the parent's trace the projection is the f32-output 256x256x64 gemm2_kernel dispatch of 960 workgroups (122 880 rows x 448) that
follows an attention kernel (fc2, the same tiling and grid, follows fc1's f16-output GEMM) and is followed by the LayerNorm.
passes_per_trace (default 3: one warm-up step and two timed ones) splits the launches into equal runs in time order; the spread
of a figure is max - min of its per-run means."""
import csv
import statistics
import sys

PROJ = "gemm2_kernel<1, 256, 256, 64, 2, 0, 0"
ROWLN = "gemm2_rowln_kernel"
LN = "layernorm_rows_kernel<1, 0, 2>"
GRID = 960 * 1024  # 122 880 rows in 256-row tiles x 2 n-tiles, 1024 threads each


def load(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Grid_Size_X"])) for r in rows]


def runs(vals, n):
    k = len(vals) // n
    return [statistics.mean(vals[i * k:(i + 1) * k]) for i in range(n)]


def show(label, vals, n):
    per = runs(vals, n)
    print(f"  {label:44s} launches {len(vals):4d}  mean {statistics.mean(vals):7.1f} us  median {statistics.median(vals):7.1f}  min {min(vals):7.1f}"
          f"  per-run means {' '.join(f'{v:.1f}' for v in per)}  spread {max(per) - min(per):.1f}")
    return per


def main(parent, this, n=3):
    n = int(n)
    P, T = load(parent), load(this)
    proj, ln, pair = [], [], []
    for i in range(1, len(P) - 1):
        name, us, grid = P[i]
        if PROJ in name and grid == GRID and "attn" in P[i - 1][0] and LN in P[i + 1][0]:
            proj.append(us)
            ln.append(P[i + 1][1])
            pair.append(us + P[i + 1][1])
    rowln = [us for name, us, grid in T if ROWLN in name and grid == 960 * 512]
    print("parent:")
    show("projection (256x256x64, f32 + residual)", proj, n)
    show("layernorm_rows_kernel<1,0,2> after it", ln, n)
    pp = show("projection + LayerNorm", pair, n)
    print("this:")
    tp = show("gemm2_rowln_kernel (projection + LayerNorm)", rowln, n)
    d = statistics.mean(pair) - statistics.mean(rowln)
    print(f"pair - rowln: {d:.1f} us per launch; run-to-run spread of the parent's pair {max(pp) - min(pp):.1f} us, of rowln {max(tp) - min(tp):.1f} us")
    for label, tr in (("parent", P), ("this", T)):
        print(f"{label}: {sum(1 for name, _, _ in tr if LN in name)} launches of layernorm_rows_kernel<1, 0, 2>, "
              f"{sum(1 for name, _, _ in tr if ROWLN in name)} of gemm2_rowln_kernel, total GPU time {sum(us for _, us, _ in tr) / 1e3:.1f} ms")


def hbm(label, fetch, write):
    M, D = 122880, 448
    alg = {"rowln": 2 * M * D + 2 * D * D + 8 * M * D + 2 * M * D, "proj256": 2 * M * D + 2 * D * D + 8 * M * D, "ln_after_proj": 6 * M * D}
    tot = {}
    for tag, path, mul in (("read", fetch, 2), ("written", write, 1)):
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
        name = [r["Kernel_Name"] for r in rows]
        for i, r in enumerate(rows):
            k = None
            if ROWLN in name[i]:
                k = "rowln"
            elif PROJ in name[i] and int(r["Grid_Size"]) == GRID and i > 0 and "attn" in name[i - 1]:
                k = "proj256"
            elif LN in name[i] and i > 1 and PROJ in name[i - 1] and int(rows[i - 1]["Grid_Size"]) == GRID and "attn" in name[i - 2]:
                k = "ln_after_proj"
            if k:
                tot.setdefault(k, {}).setdefault(tag, []).append(float(r["Counter_Value"]) * 1024 * mul)
    for k, v in tot.items():
        rd, wr = statistics.mean(v["read"]), statistics.mean(v["written"])
        print(f"{label} {k:14s} launches {len(v['read']):4d}  read {rd / 1e6:6.1f} MB  written {wr / 1e6:6.1f} MB  total {(rd + wr) / 1e6:6.1f} MB"
              f"  algorithmic {alg[k] / 1e6:6.1f} MB  ratio {(rd + wr) / alg[k]:.2f}")


if __name__ == "__main__":
    if sys.argv[1] == "--hbm":
        hbm(*sys.argv[2:])
    else:
        main(*sys.argv[1:])
