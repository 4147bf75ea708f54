"""Kept steps of a bench run from a rocprofv3 kernel trace (CSV): per-kernel
totals, then for the steps that start at k_amg_rhs / k_amg_start the
V-cycle / w / update / k_amg_rnorm launches per step, the median busy time,
the time of the last seven launches before the chunk's end (the parent's
converging group, §4.8) and one step's launch list.

    python3 tools/kept_step_trace.py <dir>/t_kernel_trace.csv
"""
import csv
import statistics
import sys
from collections import defaultdict


def short(n):
    n = n.split("(")[0].split("<")[0]
    return n.replace("void ", "").replace("mfea::", "")


def main(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2].startswith(("k_assemble", "k_amg_rhs", "k_amg_start"))]
    steps = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    print(f"{len(rows)} launches, {len(steps)} steps")
    tot = defaultdict(list)
    for s, e, n in rows:
        tot[n].append((e - s) / 1e3)
    print(f"{'kernel':40s} {'launches':>8s} {'mean_us':>9s} {'per_step_us':>11s}")
    for n, v in sorted(tot.items(), key=lambda kv: -sum(kv[1])):
        print(f"{n:40s} {len(v):8d} {sum(v) / len(v):9.2f} {sum(v) / max(1, len(steps)):11.2f}")
    kept = [s for s in steps[1:-1] if s[0][2].startswith(("k_amg_rhs", "k_amg_start"))]
    if kept:
        print(f"kept steps: {len(kept)}")
        for key in ("k_amg_vapply", "k_amg_cg_w", "k_amg_cg_update", "k_amg_rnorm", "k_amg_down", "k_amg_up"):
            print(f"  {key} per kept step:", sorted(set(sum(1 for k in s if k[2] == key) for s in kept)))
        busy = [sum(e - s for s, e, _ in st) / 1e3 for st in kept]
        span = [(max(e for _, e, _ in st) - st[0][0]) / 1e3 for st in kept]
        print(f"  busy_us median {statistics.median(busy):.1f}  span_us median {statistics.median(span):.1f}")
        # the last group before the advance kernel: from the last k_amg_down pair to the advance
        last = []
        for st in kept:
            names = [k[2] for k in st]
            if "k_cg_advance" not in names:
                continue
            ia = names.index("k_cg_advance")
            # 7 launches before the advance (or before k_amg_rnorm)
            ib = ia - 1 if names[ia - 1] == "k_amg_rnorm" else ia
            if ib < 7:
                continue
            grp = st[ib - 7:ib]
            last.append((sum(e - s for s, e, _ in grp) / 1e3, (grp[-1][1] - grp[0][0]) / 1e3, [k[2] for k in grp]))
        if last:
            print(f"  last 7 launches before the chunk end: busy median {statistics.median(x[0] for x in last):.1f} us, "
                  f"span median {statistics.median(x[1] for x in last):.1f} us: {last[0][2]}")
        st = kept[len(kept) // 2]
        print("median-position kept step launches (name dur_us gap_before_us):")
        prev = st[0][0]
        for s, e, n in st:
            print(f"  {n:28s} {(e - s) / 1e3:7.2f} {(s - prev) / 1e3:7.2f}")
            prev = e


if __name__ == "__main__":
    main(sys.argv[1])
