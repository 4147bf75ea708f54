"""Same-box A/B of ONE engine option in one build, on the benchmark's timed loop.

Each value of the option runs in its own child process, alternated over
`--rounds` so box drift hits both alike.  A child builds the network as
bench.py does, sets the option, takes `--warmup` steps, then times `--steps`
steps exactly as bench.py's loop (set_active(None) + step, wall time over the
loop) and prints ms_per_step, the iterations and a hash of U.

    python tools/option_ab.py --option amg_start --values 0 1 --rounds 10
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a, value):
    sys.path.insert(0, os.path.join(REPO, "mycelium-fea-project_amd"))
    import numpy as np

    import fea_solver as fs
    from mfea import PC_GAMG, Engine, make_opts, synth
    from mfea.synth import CONFIGS
    dy = fs.DISPLACEMENT_MAX * 20 / (fs.N_STEPS - 1)
    opts = make_opts(rtol=1e-8, max_it=2000, precond=PC_GAMG)
    nx, ny = CONFIGS[a.config]
    xyz, e2n = synth.tiled_mesh(nx, ny, chords=a.config.startswith("C5"))
    top, bot = synth.grips(xyz)
    eng = Engine(0)
    for kv in a.set:  # options held fixed in both legs
        k, v = kv.split("=")
        eng.set_option(k, int(v))
    eng.set_option(a.option, value)
    eng.set_material(fs.E_mod, fs.A, fs.I)
    eng.set_mesh(xyz, e2n)
    eng.set_bc(top, bot)
    eng.set_active(None)

    def one_step():
        eng.set_active(None)
        return eng.step(dy, -dy, opts, fs.MAX_STRAIN)

    for _ in range(a.warmup):
        one_step()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        f, _, st = one_step()
    dt = time.perf_counter() - t0
    U = eng.displacement()
    print(json.dumps({"ms_per_step": 1e3 * dt / a.steps, "iters": st.iters, "relres": st.relres,
                      "bnorm": st.bnorm, "force": float(f),
                      "U_md5": hashlib.md5(np.ascontiguousarray(U).tobytes()).hexdigest()[:12]}))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", required=True)
    ap.add_argument("--values", nargs="+", type=int, default=[0, 1])
    ap.add_argument("--config", default="C3_1M")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--set", nargs="*", default=[], help="other options name=value, the same in every leg")
    a = ap.parse_args()
    if a.child is not None:
        child(a, a.child)
        return
    ms = {v: [] for v in a.values}
    for rnd in range(a.rounds):
        for v in a.values:
            out = subprocess.run([sys.executable, __file__, "--option", a.option, "--config", a.config,
                                  "--steps", str(a.steps), "--warmup", str(a.warmup), "--child", str(v),
                                  "--set", *a.set],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(json.dumps({"option": a.option, "value": v, "rc": out.returncode,
                                  "err": out.stderr[-2000:]}), flush=True)
                sys.exit(out.returncode)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            ms[v].append(r["ms_per_step"])
            print(json.dumps({"config": a.config, "option": a.option, "value": v, "round": rnd, **r}), flush=True)
    print(json.dumps({"config": a.config, "option": a.option, "summary": {
        str(v): {"median": statistics.median(x), "min": min(x), "max": max(x),
                 "stdev": statistics.stdev(x) if len(x) > 1 else 0.0} for v, x in ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
