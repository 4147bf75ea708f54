"""Kept GAMG steps with and without nodal loads in one rocprofv3 kernel trace
(DESIGN.md §4.16): the launches per kept step of both forms, the durations of
the kernels the loads reach — k_amg_start and the fused assembly — and the
floating-mask launches of a Jacobi run whose activity moves.

    rocprofv3 --kernel-trace --stats -d DIR -o loads --output-format csv -- python tools/node_loads_trace.py run
    python tools/node_loads_trace.py report DIR

run: the planar golden mesh (3,644 nodes), launches eager (option "graph" 0:
the same kernels in the same order).  GAMG: one building step and ten kept
steps without loads, then an all-zero dead load — it takes the load kernels and
gives the same bits, so the same iteration counts: the launches compare one to
one — and ten kept steps; then with keep_operator 0 (every step assembles) five
steps under it, the load cleared, five without.  Then the self-weight of the
network (mfea.loads.self_weight) as a dead load: five kept GAMG steps (another
right-hand side: its own iteration count), and Jacobi: two steps, then three
times one element switched off (mfea_set_active) and a step.  Nothing fails
(max_strain 1)."""
import csv
import glob
import os
import statistics
import sys
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = os.path.join(REPO, "tests", "golden", "meshes", "sim_20251117_175809")
KEPT, ASM, MOVES = 10, 5, 3


def run():
    sys.path.insert(0, os.path.join(REPO, "mycelium-fea-project_amd"))
    import numpy as np
    import pandas as pd
    from mfea import Engine, loads, make_opts, PC_GAMG, PC_JACOBI
    nodes = pd.read_csv(os.path.join(MESH, "nodes.csv"))
    elems = pd.read_csv(os.path.join(MESH, "elements.csv"))
    xyz = nodes[["x", "y", "z"]].values
    e2n = elems[["n1", "n2"]].values
    y = xyz[:, 1]
    top = nodes["node_id"].values[np.abs(y - y.max()) < 1.5]
    bot = nodes["node_id"].values[np.abs(y - y.min()) < 1.5]
    weight = loads.self_weight(xyz, e2n, 1e-8, (0.0, -1.0, 0.0))
    opts = make_opts(precond=PC_GAMG, rtol=1e-8, max_it=10000)
    with Engine(0) as e:
        e.set_option("graph", 0)
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        iters = []
        for d in [0.01 * (1 + 0.01 * k) for k in range(1 + KEPT)]:
            iters.append(e.step(d, -d, opts, 1.0)[2].iters)
        e.set_node_loads(np.zeros_like(weight), "dead")
        for d in [0.01 * (1 + 0.01 * k) for k in range(KEPT)]:
            iters.append(e.step(d, -d, opts, 1.0)[2].iters)
        e.set_option("keep_operator", 0)
        for k in range(ASM):
            iters.append(e.step(0.01, -0.01, opts, 1.0)[2].iters)
        e.set_node_loads(None)
        for k in range(ASM):
            iters.append(e.step(0.01, -0.01, opts, 1.0)[2].iters)
        e.set_option("keep_operator", 1)
        e.set_node_loads(weight, "dead")
        for k in range(1 + ASM):  # (the first assembles: keep_operator was off)
            iters.append(e.step(0.01, -0.01, opts, 1.0)[2].iters)
        jac = make_opts(precond=PC_JACOBI, rtol=1e-8, max_it=100000)
        active = np.ones(len(e2n), dtype=np.uint8)
        for k in range(2 + MOVES):
            if k >= 2:
                active[17 * k] = 0
                e.set_active(active)
            iters.append(e.step(0.01, -0.01, jac, 1.0)[2].iters)
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
    for form, ld in (("no loads (LoadNone)", False), ("loads (NodeLoad)", True)):
        mine = [s for s in steps if ("NodeLoad" in s[0][2]) == ld and s[1:] and
                not any(k[2].startswith(("k_assemble", "k_cc_", "k_cg_rhs")) for k in s)]
        n = [len(s) for s in mine]
        busy = [sum(e - b for b, e, _ in s) / 1e3 for s in mine]
        if mine:
            print(f"kept steps, {form}: {len(mine)} steps, launches per step {sorted(set(n))}, "
                  f"busy_us median {statistics.median(busy):.1f}")
    # the Jacobi run: everything from its first RHS on; a step per k_cg_rhs
    jac = [i for i, r in enumerate(rows) if r[2].startswith("k_cg_rhs")]
    if jac:
        tail = rows[jac[0]:]
        cc = defaultdict(int)
        for _, _, n in tail:
            if n.startswith("k_cc_"):
                cc[n.split("<")[0]] += 1
        print(f"Jacobi under the load: {len(jac)} steps, {MOVES} of them after the activity moved; "
              f"floating-mask launches behind the first RHS: {dict(cc)} = {sum(cc.values())} "
              f"({sum(cc.values()) / MOVES:.0f} per moved step)")
        before = sum(1 for _, _, n in rows[:jac[0]] if n.startswith("k_cc_"))
        print(f"floating-mask launches in front of it (the GAMG phases and the load's first step): {before}")
    tot = defaultdict(list)
    for b, e, n in rows:
        if n.startswith(("k_amg_start", "k_assemble", "k_amg_rhs", "k_cg_rhs", "k_cc_")):
            tot[n].append((e - b) / 1e3)
    print(f"{'kernel':64s} {'launches':>8s} {'median_us':>10s} {'min_us':>8s}")
    for n, v in sorted(tot.items()):
        print(f"{n:64s} {len(v):8d} {statistics.median(v):10.2f} {min(v):8.2f}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else report(sys.argv[2])
