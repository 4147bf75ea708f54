"""Kept GAMG steps under two grip vectors and under the same motion given as a
grip field, in one rocprofv3 kernel trace: the launches per
kept step of both forms, and the durations of the kernels the field reaches —
k_amg_start, the fused assembly, the reaction.

    rocprofv3 --kernel-trace --stats -d DIR -o field --output-format csv -- python tools/grip_field_trace.py run
    python tools/grip_field_trace.py report DIR

run: the planar golden mesh (3,644 nodes), GAMG, launches eager (option
"graph" 0: the same kernels in the same order), the vectors (0.6, 0.8, 0) /
(0, 1, 0).  One building step and ten kept steps with mfea_set_grip_motion,
then the uniform field of these vectors (mfea.fields.uniform) and ten kept
steps; then with keep_operator 0 (every step assembles) five steps under the
field, the field cleared, five under the vectors.  Nothing fails
(max_strain 1)."""
import csv
import glob
import os
import statistics
import sys
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = os.path.join(REPO, "tests", "golden", "meshes", "sim_20251117_175809")
KEPT, ASM = 10, 5
TOP, BOT = (0.6, 0.8, 0.0), (0.0, 1.0, 0.0)


def run():
    sys.path.insert(0, os.path.join(REPO, "mycelium-fea-project_amd"))
    import numpy as np
    import pandas as pd
    from mfea import Engine, fields, make_opts, PC_GAMG
    nodes = pd.read_csv(os.path.join(MESH, "nodes.csv"))
    elems = pd.read_csv(os.path.join(MESH, "elements.csv"))
    xyz = nodes[["x", "y", "z"]].values
    y = xyz[:, 1]
    top = nodes["node_id"].values[np.abs(y - y.max()) < 1.5]
    bot = nodes["node_id"].values[np.abs(y - y.min()) < 1.5]
    field = fields.uniform(len(xyz), top, TOP) + fields.uniform(len(xyz), bot, BOT)
    opts = make_opts(precond=PC_GAMG, rtol=1e-8, max_it=10000)
    with Engine(0) as e:
        e.set_option("graph", 0)
        e.set_mesh(xyz, elems[["n1", "n2"]].values)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_grip_motion(TOP, BOT)
        iters = []
        for d in [0.01 * (1 + 0.01 * k) for k in range(1 + KEPT)]:
            iters.append(e.step(d, -d, opts, 1.0)[2].iters)
        e.set_grip_field(field)
        for d in [0.01 * (1 + 0.01 * k) for k in range(KEPT)]:
            iters.append(e.step(d, -d, opts, 1.0)[2].iters)
        e.set_option("keep_operator", 0)
        for k in range(ASM):
            iters.append(e.step(0.01, -0.01, opts, 1.0)[2].iters)
        e.set_grip_field(None)
        for k in range(ASM):
            iters.append(e.step(0.01, -0.01, opts, 1.0)[2].iters)
        print("iterations per step:", iters, "kept steps:", e.get_option("op_kept_steps"))


def short(n):
    n = n.replace("void ", "").replace("mfea::", "").replace("(anonymous namespace)::", "")
    return n.split("(")[0]


def report(d):
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    print(f"{len(rows)} launches in {os.path.basename(path)}")
    # a kept step starts at its k_amg_start; the two forms by their template argument
    starts = [i for i, r in enumerate(rows) if r[2].startswith("k_amg_start")]
    steps = [rows[a:b] for a, b in zip(starts, starts[1:])]
    for form, fld in (("vectors (GripVec)", False), ("field (GripField)", True)):
        mine = [s for s in steps if ("GripField" in s[0][2]) == fld and s[1:] and
                not any(k[2].startswith("k_assemble") for k in s)]
        n = [len(s) for s in mine]
        busy = [sum(e - b for b, e, _ in s) / 1e3 for s in mine]
        if mine:
            print(f"kept steps, {form}: {len(mine)} steps, launches per step {sorted(set(n))}, "
                  f"busy_us median {statistics.median(busy):.1f}")
    tot = defaultdict(list)
    for b, e, n in rows:
        if n.startswith(("k_amg_start", "k_assemble", "k_reaction", "k_amg_rhs", "k_event_scan")):
            tot[n].append((e - b) / 1e3)
    print(f"{'kernel':64s} {'launches':>8s} {'median_us':>10s} {'min_us':>8s}")
    for n, v in sorted(tot.items()):
        print(f"{n:64s} {len(v):8d} {statistics.median(v):10.2f} {min(v):8.2f}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2])
