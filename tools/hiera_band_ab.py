"""Two serialized kernel traces of bench.py side by side, per kernel and grid size
(LMX_SERIAL=1 rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 --steps 2 --warmup 1): the parent's, whose
Hiera blocks in front of the first global one run on whole 64-row grids, against a tree that runs them on the 42-row band
(HieraEncoder(band=True)).  A kernel of those blocks shows up with the same launch count and a smaller grid; everything else must
not move.

usage: python tools/hiera_band_ab.py parent_kernel_trace.csv this_kernel_trace.csv [min_ms]
Per kernel name (template arguments kept, cut at 100 characters) and per grid size (workgroups): launches, mean, shortest, longest and
total time in each trace; names whose time in either trace is under min_ms (default 0.5) are summed into one line.

The same serves two trees whose bands differ (HieraEncoder(band=True) against band="blocks": 168 / 84 against 152 / 76 rows).  GEMMs,
im2col and the LayerNorms change their workgroup count with the rows and get a line per arm; a persistent kernel keeps its grid of
256 workgroups in both arms, and every launch of it in a SAM pass is band-sized in both, so its two means compare directly.  The
joins of band="blocks" (38 -> 42 and 42 -> 64 rows) run on one capped grid and share a line: shortest and longest tell them apart."""
import csv
import sys


def load(path):
    acc = {}
    for r in csv.DictReader(open(path)):
        wg = max(1, int(r["Workgroup_Size_X"]) * int(r.get("Workgroup_Size_Y", 1) or 1) * int(r.get("Workgroup_Size_Z", 1) or 1))
        grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1) // wg
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        a = acc.setdefault(r["Kernel_Name"][:100], {}).setdefault(grid, [0, 0.0, us, us])
        a[0] += 1
        a[1] += us
        a[2], a[3] = min(a[2], us), max(a[3], us)
    return acc


def total(by_grid):
    return sum(a[1] for a in by_grid.values()) / 1e3


def main(parent, this, min_ms=0.5):
    P, T = load(parent), load(this)
    names = sorted(set(P) | set(T), key=lambda k: -max(total(P.get(k, {})), total(T.get(k, {}))))
    rest = [0.0, 0.0]
    for name in names:
        p, t = P.get(name, {}), T.get(name, {})
        if max(total(p), total(t)) < float(min_ms):
            rest[0] += total(p)
            rest[1] += total(t)
            continue
        print(f"{name}\n    total  parent {total(p):8.2f} ms   this {total(t):8.2f} ms   ({total(t) - total(p):+.2f})")
        for label, side in (("parent", p), ("this", t)):
            for grid, (n, us, lo, hi) in sorted(side.items(), key=lambda kv: -kv[1][1]):
                if us / 1e3 >= 0.05:
                    print(f"    {label:6s} workgroups {grid:8d}  launches {n:5d}  mean {us / n:8.1f} us  ({lo:.1f} .. {hi:.1f})  total {us / 1e3:8.2f} ms")
    print(f"(kernels under {min_ms} ms in both traces)\n    total  parent {rest[0]:8.2f} ms   this {rest[1]:8.2f} ms")
    tp, tt = sum(total(v) for v in P.values()), sum(total(v) for v in T.values())
    print(f"GPU time of all kernels: parent {tp:.1f} ms, this {tt:.1f} ms ({tt - tp:+.1f} ms over the trace)")
    print(f"launches: parent {sum(a[0] for v in P.values() for a in v.values())}, this {sum(a[0] for v in T.values() for a in v.values())}")


if __name__ == "__main__":
    main(*sys.argv[1:])
