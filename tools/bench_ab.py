"""Same-box A/B of two libmfea.so builds on the benchmark command itself.

`bench.py --gpus 1 --steps S --warmup W --no-cpu --no-full-run` once per
library and round, each in its own process (MFEA_LIB=...), alternated so box
drift hits both alike.  One JSON line per run (bench.py's own result line plus
the library and the round), then a summary: median, min, max and standard
deviation of ms_per_step per library (DESIGN.md §4.10's procedure).

    python tools/bench_ab.py --libs abso/libmfea_parent.so mycelium-fea-project_amd/libmfea.so \
        --config C3_1M --rounds 10 > profiles/x/bench_C3_parent_vs_new.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--config", default="C3_1M")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per run")
    a = ap.parse_args()
    ms = {lib: [] for lib in a.libs}
    for rnd in range(a.rounds):
        for lib in a.libs:
            env = dict(os.environ, MFEA_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                                  str(a.steps), "--warmup", str(a.warmup), "--config", a.config, "--no-cpu",
                                  "--no-full-run"], env=env, capture_output=True, text=True, timeout=a.timeout)
            if out.returncode != 0:  # a run that failed ends the alternation: nothing more starts on the GPU
                print(json.dumps({"lib": lib, "round": rnd, "rc": out.returncode, "err": out.stderr[-2000:]}),
                      flush=True)
                sys.exit(out.returncode if out.returncode > 0 else 1)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            ms[lib].append(r["ms_per_step"])
            print(json.dumps({"lib": os.path.basename(lib), "round": rnd, "config": a.config,
                              "ms_per_step": r["ms_per_step"], "cg_iters": r.get("cg_iters"),
                              "relres": r.get("relres"), "value": r.get("value")}), flush=True)
    print(json.dumps({"config": a.config, "summary": {
        os.path.basename(lib): {"median": statistics.median(x), "min": min(x), "max": max(x),
                                "stdev": statistics.stdev(x) if len(x) > 1 else 0.0, "runs": len(x)}
        for lib, x in ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
