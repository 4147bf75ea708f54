"""bench.py's plain run on the GPU, at the smallest config (C2_100k): the
result line of the timed steps alone, and --dump-outputs' files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_result_line_and_dumped_outputs(tmp_path):
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--config", "C2_100k", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "DOF/s" and out["higher_is_better"] is True and out["dtype"].startswith("f64")
    assert (out["steps"], out["warmup"], out["n_gpus"]) == (2, 1, 1)
    n_dof, n_elems = out["config"]["n_dof"], out["config"]["n_elems"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n_dof * 1e3 / out["ms_per_step"], rel=1e-9)
    assert out["relres"] <= 1e-8 and out["cg_iters"] > 0
    # everything measured outside the timed steps is --full's
    for k in ("roofline", "roofline_iteration", "step_breakdown_ms", "full_run", "jacobi_iters_1e8",
              "sor_iters_1e8", "cpu_baseline"):
        assert k not in out, k
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["active", "displacement", "n_active", "reaction_force", "stress"]
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in got.values())
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    assert got["displacement"].shape == (n_dof,) and got["stress"].shape == (n_elems,)
    assert got["active"].shape == (n_elems,) and got["active"].sum() == got["n_active"][0]
    assert np.abs(got["displacement"]).max() > 0 and got["reaction_force"].shape == (1,)
