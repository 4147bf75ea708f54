"""mfea_run / Engine.run: the whole load-step run as one call, every step's
records gathered on the device and copied out while the next step computes.

The cases are committed meshes with the load schedule dy_k = dmax·k/(n-1):
an early stop (n_active reaches 0), a fully clamped mesh (n_free = 0), a 3-DOF
mesh whose node count is no multiple of a wave or a block with a failure
mid-run, and a planar mesh with several new active sets (kept hierarchy)."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, load_mesh, read_rt
from test_gpu_parity import check_stress_records, force_close, rel

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

MAX_STRAIN = 0.018
JACOBI, GAMG = 0, 2
SENT_F, SENT_B = -777.25, 7  # sentinels of rows the run must not touch

# name: (mesh, grip tol, n_steps, dmax)
CASES = {
    "X_stop25": ("test_X", 0.5, 40, 0.06),
    "X_stop2": ("test_X", 0.5, 6, 2.0),
    "I_clamped": ("test_I", 1.5, 4, 0.06),
    "sim3d": ("sim_20251115_135507", 0.5, 8, 0.02),
    "planar": ("sim_20251117_175809", 1.5, 40, 0.02),
}
PCS = [JACOBI, GAMG]


def _opts(pc, **kw):
    from mfea import make_opts
    kw.setdefault("rtol", 1e-10)
    kw.setdefault("max_it", 200000)
    return make_opts(precond=pc, **kw)


def _schedule(n, dmax):
    dy = np.array([dmax * (k / (n - 1)) for k in range(n)])
    return dy, -dy


def _mesh(name, grip):
    nodes, elems = load_mesh(name)
    xyz = nodes[["x", "y", "z"]].values
    e2n = elems[["n1", "n2"]].values
    top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, grip)
    return nodes, xyz, e2n, top, bot


def _start(engine, case):
    """A fresh build of the case's mesh with every element active."""
    mesh, grip, n, dmax = CASES[case]
    _, xyz, e2n, top, bot = _mesh(mesh, grip)
    engine.set_mesh(xyz, e2n)
    engine.set_bc(top, bot)
    engine.set_active(None)
    return _schedule(n, dmax)


def _sentinel_out(engine, n):
    return {"U": np.full((n, 3 * engine.n_nodes), SENT_F), "stress": np.full((n, engine.n_elems), SENT_F),
            "active": np.full((n, engine.n_elems), SENT_B, dtype=np.uint8)}


def _loop(engine, case, opts):
    """The caller's loop: step + the three getters, stopping as the drop-in does."""
    from mfea import SolverFailure
    dyt, dyb = _start(engine, case)
    rec = {"U": [], "stress": [], "active": [], "force": [], "n_active": []}
    for k in range(len(dyt)):
        try:
            f, na, _ = engine.step(dyt[k], dyb[k], opts, MAX_STRAIN)
        except SolverFailure:
            break
        rec["force"].append(f)
        rec["n_active"].append(na)
        rec["U"].append(engine.displacement())
        rec["stress"].append(engine.stress())
        rec["active"].append(engine.active())
        if na == 0:
            break
    return {k: np.asarray(v) for k, v in rec.items()}


_cache = {}


def _pair(engine, case, pc):
    """(loop records, run result, the run's sentinel-filled arrays), computed
    once per case and preconditioner and shared by the tests (never modified).
    GAMG: option amg_rebuild_rent 0 in both — the rent rule reads a clock."""
    key = (case, pc)
    if key not in _cache:
        with engine.options(amg_rebuild_rent=0):
            loop = _loop(engine, case, _opts(pc))
            dyt, dyb = _start(engine, case)
            out = _sentinel_out(engine, len(dyt))
            run = engine.run(dyt, dyb, _opts(pc), MAX_STRAIN, out=out)
        _cache[key] = (loop, run, out)
    return _cache[key]


def _failure_steps(n_active, n_elems):
    prev = np.concatenate([[n_elems], n_active[:-1]])
    return np.flatnonzero(n_active < prev)


# ---------------------------------------------------------------------------
# 1. a run's last row is what the getters return right after it, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(CASES))
def test_last_row_equals_getters(engine, case, pc):
    loop, _, _ = _pair(engine, case, pc)
    n_done = len(loop["n_active"])
    fails = _failure_steps(loop["n_active"], loop["active"].shape[1])
    ks = {0, n_done - 1}
    if len(fails):
        ks |= {int(fails[0]), min(int(fails[0]) + 1, n_done - 1)}
    dyt, dyb = _start(engine, case)
    with engine.options(amg_rebuild_rent=0):
        for k in sorted(ks):
            engine.set_active(None)
            r = engine.run(dyt[:k + 1], dyb[:k + 1], _opts(pc), MAX_STRAIN)
            assert r["n_done"] == k + 1, k
            assert np.array_equal(r["U"][-1], engine.displacement()), k
            assert np.array_equal(r["stress"][-1], engine.stress()), k
            assert np.array_equal(r["active"][-1], engine.active()), k
            assert r["n_active"][k] == loop["n_active"][k], k
            assert r["n_active"][k] == int(r["active"][-1].sum()), k
            assert force_close(r["force"], loop["force"][:k + 1]), k


# ---------------------------------------------------------------------------
# 2. the run is the loop: same stop, same activity, the same bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(CASES))
def test_run_equals_loop(engine, case, pc):
    """Jacobi has no clock-dependent decision; GAMG runs with amg_rebuild_rent
    0 in both (the rent rule reads a clock).  Bitwise equality in both."""
    loop, run, out = _pair(engine, case, pc)
    n = run["n_done"]
    assert n == len(loop["n_active"])
    assert np.array_equal(run["n_active"], loop["n_active"])
    assert np.array_equal(run["active"], loop["active"])
    assert np.array_equal(run["U"], loop["U"])
    assert np.array_equal(run["stress"], loop["stress"])
    assert np.array_equal(run["force"], loop["force"])
    assert len(run["stats"]) == n and len(run["wall_s"]) == n and np.all(run["wall_s"] > 0)
    assert all(s["status"] == 0 for s in run["stats"])
    # rows the run did not reach stay as they were
    assert np.all(out["U"][n:] == SENT_F) and np.all(out["stress"][n:] == SENT_F)
    assert np.all(out["active"][n:] == SENT_B)


def _oracle(case):
    key = ("oracle", case)
    if key not in _cache:
        mesh, grip, n, dmax = CASES[case]
        nodes, xyz, e2n, _, _ = _mesh(mesh, grip)
        _cache[key] = fo.run_fea(xyz, nodes["node_id"].values, e2n, tol=grip, n_steps=n, disp_max=dmax)
    return _cache[key]


@pytest.mark.parametrize("case,n_done,reason", [
    ("X_stop25", 25, 1), ("X_stop2", 2, 1), ("I_clamped", 4, 0), ("sim3d", 8, 0), ("planar", 40, 0)])
def test_run_stops_as_the_oracle_does(engine, case, n_done, reason):
    """The step count of the oracle's run_fea on these inputs, its element
    counts and its activity, step by step."""
    ref = _oracle(case)
    _, run, _ = _pair(engine, case, JACOBI)
    assert run["n_done"] == n_done == len(ref["U"])
    assert run["stop_reason"] == reason
    assert np.array_equal(run["n_active"], ref["active"].sum(axis=1))
    assert np.array_equal(run["active"], ref["active"])


def test_failure_mid_run_and_clamped_records(engine):
    _, run, _ = _pair(engine, "sim3d", JACOBI)
    assert list(run["n_active"][:4]) == [1661, 1661, 1661, 1623]
    # test_I at grip 1.5: every node is a grip node — U is the prescribed values
    mesh, grip, n, dmax = CASES["I_clamped"]
    _, xyz, e2n, top, bot = _mesh(mesh, grip)
    _, run, _ = _pair(engine, "I_clamped", JACOBI)
    dyt, dyb = _schedule(n, dmax)
    assert run["stats"][0]["n_free"] == 0
    for k in range(n):
        known, vals = fo.known_dof_map(top, bot, dyt[k], dyb[k])
        U = np.zeros(3 * len(xyz))
        U[known] = vals
        assert np.array_equal(run["U"][k], U)


# ---------------------------------------------------------------------------
# 3. against the oracle (the reference's algorithm on the CPU)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", ["sim3d", "X_stop25"])
def test_run_matches_oracle(engine, case, pc):
    mesh, grip, n, dmax = CASES[case]
    nodes, xyz, e2n, top, bot = _mesh(mesh, grip)
    ref = _oracle(case)
    dyt, dyb = _start(engine, case)
    run = engine.run(dyt, dyb, _opts(pc, rtol=1e-13), MAX_STRAIN)
    assert run["U"].shape == ref["U"].shape
    for k in range(run["n_done"]):
        assert rel(run["U"][k], ref["U"][k]) <= 1e-10, k
    assert np.array_equal(run["active"], ref["active"])
    assert force_close(run["force"], np.asarray(ref["force"])[:, 1])
    check_stress_records(xyz, e2n, run["U"], run["stress"], run["active"])


# ---------------------------------------------------------------------------
# 4. a solver stop ends the run without an exception
# ---------------------------------------------------------------------------
def test_solver_stop(engine):
    """Jacobi with max_it 1 at rtol 1e-13: step 0 has a zero right-hand side
    and converges, step 1 cannot."""
    from mfea import _capi
    dyt, dyb = _start(engine, "planar")
    out = _sentinel_out(engine, 4)
    run = engine.run(dyt[:4], dyb[:4], _opts(JACOBI, rtol=1e-13, max_it=1), MAX_STRAIN, out=out)
    assert run["n_done"] == 1
    assert run["stop_reason"] == _capi.EMAXIT
    assert np.array_equal(run["U"][0], np.zeros(3 * engine.n_nodes))
    assert np.array_equal(run["stress"][0], np.zeros(engine.n_elems)) and run["active"][0].all()
    assert run["n_active"][0] == engine.n_elems and run["force"][0] == 0.0
    assert np.all(out["U"][1:] == SENT_F) and np.all(out["stress"][1:] == SENT_F)
    assert np.all(out["active"][1:] == SENT_B)


# ---------------------------------------------------------------------------
# 5. optional records, reuse of one engine, a one-step run, the pinned path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
def test_optional_records(engine, pc):
    _, full, _ = _pair(engine, "sim3d", pc)
    with engine.options(amg_rebuild_rent=0):
        dyt, dyb = _start(engine, "sim3d")
        run = engine.run(dyt, dyb, _opts(pc), MAX_STRAIN, keep=("stress",))
    assert run["U"] is None and run["active"] is None
    assert np.array_equal(run["stress"], full["stress"])
    assert np.array_equal(run["force"], full["force"])
    assert np.array_equal(run["n_active"], full["n_active"])


def test_reuse_across_meshes_and_one_step(engine):
    """Two runs on one engine with another mesh set in between: the node order
    and the staging slabs follow the current build."""
    refs = {c: _pair(engine, c, JACOBI)[1] for c in ("sim3d", "X_stop25", "planar")}
    for case in ("planar", "X_stop25", "sim3d"):
        dyt, dyb = _start(engine, case)
        run = engine.run(dyt, dyb, _opts(JACOBI), MAX_STRAIN)
        for name in ("U", "stress", "active", "force", "n_active"):
            assert np.array_equal(run[name], refs[case][name]), (case, name)
    dyt, dyb = _start(engine, "sim3d")
    one = engine.run(dyt[:1], dyb[:1], _opts(JACOBI), MAX_STRAIN)
    assert one["n_done"] == 1 and one["stop_reason"] == 0
    assert np.array_equal(one["U"][0], refs["sim3d"]["U"][0])


@pytest.mark.parametrize("case", ["sim3d", "X_stop25"])
def test_pinned_slab_path_equals_registered(engine, case):
    """Option run_register 0: the copies go through the pinned host slabs (the
    path taken when the record arrays cannot be page-locked)."""
    _, ref, _ = _pair(engine, case, JACOBI)
    with engine.options(run_register=0):
        dyt, dyb = _start(engine, case)
        out = _sentinel_out(engine, len(dyt))
        run = engine.run(dyt, dyb, _opts(JACOBI), MAX_STRAIN, out=out)
        assert engine.get_option("run_direct") == 0
    for name in ("U", "stress", "active", "force", "n_active"):
        assert np.array_equal(run[name], ref[name]), name
    n = run["n_done"]
    assert np.all(out["U"][n:] == SENT_F) and np.all(out["active"][n:] == SENT_B)


# ---------------------------------------------------------------------------
# 6. partitioned handles are refused
# ---------------------------------------------------------------------------
def test_partitioned_handle_is_refused(engine):
    from mfea import _capi
    dyt, dyb = _start(engine, "sim3d")
    try:
        engine.set_parts(2)
        with pytest.raises(_capi.MfeaError) as ei:
            engine.run(dyt, dyb, _opts(JACOBI), MAX_STRAIN)
        assert ei.value.code == _capi.ESTATE
        f, na, st = engine.step(dyt[1], dyb[1], _opts(JACOBI), MAX_STRAIN)
        assert st.status == 0 and na == engine.n_elems
    finally:
        engine.set_parts(1)


# ---------------------------------------------------------------------------
# 7. the drop-in: device_run=True writes what the loop writes
# ---------------------------------------------------------------------------
FILES = ("force_displacement.csv", "stress_record.csv", "node_displacements.csv", "active_elements.csv")


def _dropin(tmp_path, tag, case, pc, device_run):
    import fea_solver as fs
    mesh, grip, n, dmax = CASES[case]
    d = tmp_path / tag / mesh
    shutil.copytree(os.path.join(GOLDEN, "meshes", mesh), d)
    saved = (fs.N_STEPS, fs.DISPLACEMENT_MAX)
    fs.N_STEPS, fs.DISPLACEMENT_MAX = n, dmax
    try:
        with fs.get_engine().options(amg_rebuild_rent=0):
            res = fs.fea_solver(str(d), tol=grip, verbose=False, precond=pc, device_run=device_run)
    finally:
        fs.N_STEPS, fs.DISPLACEMENT_MAX = saved
    return d / "fea_results", res


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", ["X_stop25", "sim3d"])
def test_dropin_device_run_writes_the_same_files(tmp_path, case, pc):
    """Jacobi and GAMG (amg_rebuild_rent 0): byte-identical record files."""
    a, ra = _dropin(tmp_path, "loop", case, pc, False)
    b, rb = _dropin(tmp_path, "run", case, pc, True)
    for f in FILES:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    for k in ("force", "stress", "active", "U"):
        assert ra[k].shape == rb[k].shape and ra[k].dtype == rb[k].dtype, k
        assert np.array_equal(ra[k], rb[k]), k
    n_done = len(read_rt(b / "force_displacement.csv"))
    lines = (b / "solve_runtime.txt").read_text().splitlines()
    assert lines[0] == "step, runtime_s" and len(lines) == 1 + n_done
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == list(range(1, n_done + 1))
    assert (b / "runtime.txt").exists()
