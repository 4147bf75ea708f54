"""What heterogeneity costs on a bench network: the uniform engine against
per-element properties (mfea_set_element_props) in the same process — device
times (HIP events, option phase_times 1) of the assembly and the post of an
assembling load step (option keep_operator 0: every step assembles), of an
event's post (mfea_event), and the GAMG iteration count.

The arrays are the tests' recipe: sections over a 4x range (A = A0·s, s
log-uniform in [0.5, 2], I = A·0.001), Weibull(6) strengths — scaled so that
nothing fails and every repetition runs on the same active set; "filled" is
the per-element path on arrays filled with the scalars (the kernels' cost
without the change of K).  Interleaved repetitions, medians.

    python3 tools/props_ab.py [--config C3_1M] [--reps 7] [--out profiles/props/C3.json]

Prints ONE JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mycelium-fea-project_amd"))


def recipe(n, A0):
    rng = np.random.default_rng(7)
    s = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n))
    A = A0 * s
    return A, A * 0.001, 0.018 * np.clip(rng.weibull(6.0, n), 0.2, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3_1M", choices=["C2_100k", "C3_1M"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mfea import Engine, make_opts, PC_GAMG, synth
    from mfea.synth import CONFIGS
    import fea_solver as fs

    nx, ny = CONFIGS[a.config]
    xyz, e2n = synth.tiled_mesh(nx, ny)
    top, bot = synth.grips(xyz)
    n = len(e2n)
    opts = make_opts(rtol=a.rtol, max_it=200000, precond=PC_GAMG)
    eng = Engine(0)
    eng.set_material(fs.E_mod, fs.A, fs.I)
    eng.set_mesh(xyz, e2n)
    eng.set_bc(top, bot)
    eng.set_active(None)
    A, I, s = recipe(n, fs.A)  # noqa: E741
    never = s * 1e6  # (strengths nothing reaches: the post's loads, no failure)
    cases = {
        "uniform": {},
        "filled": dict(E=np.full(n, float(fs.E_mod)), A=np.full(n, fs.A), I=np.full(n, fs.I),
                       max_strain=np.full(n, 1e6)),
        "recipe": dict(A=A, I=I, max_strain=never),
        "recipe_with_E": dict(E=np.full(n, float(fs.E_mod)), A=A, I=I, max_strain=never),
    }
    dy = fs.DISPLACEMENT_MAX / 2
    raw = {k: {"t_assemble_ms": [], "t_post_ms": [], "t_event_post_ms": [], "iters": []} for k in cases}
    with eng.options(phase_times=1, keep_operator=0):
        for rep in range(a.reps + 1):  # (repetition 0: warm-up — hierarchy, graphs, allocator)
            for name, props in cases.items():
                eng.set_element_props(**props)
                for _ in range(2):
                    _, na, st = eng.step(dy, -dy, opts, 1e6)
                assert na == n and st.status == 0
                # a terminal event (lam_max below every lam): the event pair's cost, no failure
                _, _, nf, _, ste = eng.event(dy, -dy, opts, 1e6, 1e-9, 1e-12)
                assert nf == 0
                if rep:
                    raw[name]["t_assemble_ms"].append(st.t_assemble_ms)
                    raw[name]["t_post_ms"].append(st.t_post_ms)
                    raw[name]["t_event_post_ms"].append(ste.t_post_ms)
                    raw[name]["iters"].append(st.iters)
            print(f"rep {rep} done", file=sys.stderr, flush=True)
    eng.close()
    med = {k: {q: float(np.median(v)) for q, v in r.items()} for k, r in raw.items()}
    out = {"config": a.config, "n_nodes": int(len(xyz)), "n_elems": int(n), "rtol": a.rtol, "reps": a.reps,
           "median": med,
           "assemble_ratio": {k: med[k]["t_assemble_ms"] / med["uniform"]["t_assemble_ms"] for k in cases},
           "post_ratio": {k: med[k]["t_post_ms"] / med["uniform"]["t_post_ms"] for k in cases},
           "event_post_ratio": {k: med[k]["t_event_post_ms"] / med["uniform"]["t_event_post_ms"] for k in cases},
           "raw": raw,
           "note": "device ms between HIP events (phase_times 1) of a load step that assembles (keep_operator 0) "
                   "and of a terminal mfea_event; GAMG iterations of that step; byte estimate of the row gather: "
                   "+16 B on about 81 B per slot"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
