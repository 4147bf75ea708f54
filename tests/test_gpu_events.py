"""mfea_event / mfea_run_events: event-driven failure runs — one solve at a
reference load per failure, each break at its exact load factor.

The semantics (include/mfea.h) are single IEEE f64 operations on the device's
own U₁, so NumPy reproduces smax, lam, the failing group and the stress row
bit for bit; the sequence of events is checked against a direct-solve oracle
formed here with the same rule."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, load_gen, load_mesh, read_rt

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

MAX_STRAIN = 0.018
E_MOD = fo.E_MOD
JACOBI, GAMG = 0, 2
PCS = [JACOBI, GAMG]
SENT_F, SENT_B = -777.25, 7  # sentinels of rows the run must not touch

# name: (mesh, grip tol, dref, lam_max, tie_rtol, events asked for)
CASES = {
    "X": ("test_X", 0.5, 0.06, np.inf, 1e-9, 8),
    "I_clamped": ("test_I", 1.5, 0.06, np.inf, 1e-9, 4),
    "y": ("test_y", 1.5, 0.06, np.inf, 1e-9, 6),
    "sim3d": ("sim_20251115_135507", 0.5, 0.02, 1.0, 1e-9, 6),
    "planar": ("sim_20251117_175809", 1.5, 0.02, 1.0, 1e-9, 12),
}
# the oracle sequence (tie_rtol 1e-6): name: (mesh, grip, dref, lam_max, events with failures, stop)
ORACLE = {
    "X": ("test_X", 0.5, 0.06, np.inf, 3, "unloaded"),
    "I_clamped": ("test_I", 1.5, 0.06, np.inf, 1, "unloaded"),
    "sim3d": ("sim_20251115_135507", 0.5, 0.02, 1.0, 3, "lam_max"),
    "planar": ("sim_20251117_175809", 1.5, 0.02, 1.0, 8, "lam_max"),
    "sim181147": ("sim_20251117_181147", 1.5, 0.02, 1.0, 7, "lam_max"),
    "sim181147_lam3": ("sim_20251117_181147", 1.5, 0.02, 3.0, 9, "lam_max"),
}


def _opts(pc, rtol=1e-13):
    from mfea import make_opts
    return make_opts(precond=pc, rtol=rtol, max_it=200000)


_meshes = {}


def _mesh(name, grip):
    if (name, grip) not in _meshes:
        nodes, elems = load_mesh(name)
        xyz = nodes[["x", "y", "z"]].values
        e2n = elems[["n1", "n2"]].values
        top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, grip)
        _meshes[(name, grip)] = (xyz, e2n, top, bot)
    return _meshes[(name, grip)]


def _start(engine, mesh, grip):
    xyz, e2n, top, bot = _mesh(mesh, grip)
    engine.set_mesh(xyz, e2n)
    engine.set_bc(top, bot)
    engine.set_active(None)
    return xyz, e2n


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit equality of f64 arrays; NaNs (any payload) match NaNs."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    a, b = np.atleast_1d(a).ravel(), np.atleast_1d(b).ravel()
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan]))


def rule(eps, act0, max_strain, tie_rtol, lam_max):
    """The event rule of include/mfea.h on a strain vector, in NumPy f64:
    (smax, lam, failing group, stress row)."""
    a = np.abs(eps)
    m = act0 & ~np.isnan(a)
    smax = np.float64(a[m].max()) if m.any() else np.float64(0.0)
    with np.errstate(divide="ignore"):
        lam = np.float64(max_strain) / smax
    breaks = bool(smax > 0.0 and lam <= lam_max)
    thr = smax * (np.float64(1.0) - np.float64(tie_rtol))
    group = (m & (a >= thr)) if breaks else np.zeros_like(act0)
    factor = lam if breaks else (np.float64(lam_max) if np.isfinite(lam_max) else np.float64(1.0))
    with np.errstate(invalid="ignore"):
        stress = np.where(act0, (E_MOD * eps) * factor, 0.0)
    return smax, lam, group, stress


def event_loop(engine, mesh, grip, dref, lam_max, tie, n_events, pc, *, check=True, floating=False, rtol=1e-13):
    """The caller's loop over mfea_event from a fresh build, with the bitwise
    anchor on the device's own U₁ checked at every event (check=True).  Returns
    the per-event records (U1 unscaled)."""
    xyz, e2n = _start(engine, mesh, grip)
    opts = _opts(pc, rtol)
    rec = {k: [] for k in ("lam", "force1", "n_failed", "n_active", "U1", "stress", "active", "group")}
    n_act = len(e2n)
    for k in range(n_events):
        act0 = engine.active()
        assert int(act0.sum()) == n_act
        fl = engine.floating() if floating else None
        lam, f1, nf, na, _ = engine.event(dref, -dref, opts, MAX_STRAIN, tie, lam_max)
        U1, stress, act1 = engine.displacement(), engine.stress(), engine.active()
        if check:
            eps = fo.element_strain(xyz, e2n, U1)
            smax, lam_np, group, stress_np = rule(eps, act0, MAX_STRAIN, tie, lam_max)
            assert same_bits(lam, lam_np), (k, lam, lam_np)
            assert np.array_equal(act1, act0 & ~group), k
            assert nf == int(group.sum()) and na == int(act1.sum()), k
            assert same_bits(stress, stress_np), k
            if n_act:
                # the same solve's reaction through mfea_post (K and U₁ are
                # still those of the event; inf fails nothing)
                f_post, na_post = engine.post(np.inf)
                assert same_bits(f1, f_post), (k, f1, f_post)
                assert na_post == na
            else:
                assert f1 == 0.0 and np.isinf(lam) and nf == 0
        if fl is not None and n_act:
            assert np.all(U1.reshape(-1, 3)[fl] == 0.0), k
        assert not np.any(act1 & ~act0), k  # activity only shrinks
        assert na == n_act - nf, k
        n_act = na
        for key, v in zip(rec, (lam, f1, nf, na, U1, stress, act1, act0 & ~act1)):
            rec[key].append(v)
        if nf == 0:
            break
    return {k: np.asarray(v) for k, v in rec.items()}


def _sentinel_out(engine, n):
    return {"U": np.full((n, 3 * engine.n_nodes), SENT_F), "stress": np.full((n, engine.n_elems), SENT_F),
            "active": np.full((n, engine.n_elems), SENT_B, dtype=np.uint8)}


_cache = {}


def _pair(engine, case, pc):
    """(loop records, run result, the run's sentinel arrays, the pinned-path run)
    once per case and preconditioner, shared and never modified."""
    key = (case, pc)
    if key not in _cache:
        mesh, grip, dref, lam_max, tie, n = CASES[case]
        with engine.options(amg_rebuild_rent=0):
            loop = event_loop(engine, mesh, grip, dref, lam_max, tie, n, pc)
            _start(engine, mesh, grip)
            out = _sentinel_out(engine, n)
            run = engine.run_events(dref, -dref, _opts(pc), MAX_STRAIN, tie, lam_max, n_events=n, out=out)
            direct = engine.get_option("run_direct")
            _start(engine, mesh, grip)
            with engine.options(run_register=0):
                pinned = engine.run_events(dref, -dref, _opts(pc), MAX_STRAIN, tie, lam_max, n_events=n)
                assert engine.get_option("run_direct") == 0
        _cache[key] = (loop, run, out, pinned, direct)
    return _cache[key]


# ---------------------------------------------------------------------------
# 1. bitwise anchor on the device's own U₁ (asserted inside event_loop)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(CASES))
def test_event_matches_the_rule_bit_for_bit(engine, case, pc):
    loop, _, _, _, _ = _pair(engine, case, pc)
    assert len(loop["lam"]) >= 1
    # the last event recorded is terminal, or the loop used every event asked for
    assert loop["n_failed"][-1] == 0 or len(loop["lam"]) == CASES[case][5]
    if case == "X":
        assert loop["n_failed"].tolist() == [2, 4, 8, 0] and np.isinf(loop["lam"][-1])
        assert loop["force1"][-1] == 0.0 and loop["n_active"][-1] == 0
        assert not loop["stress"][-1].any()
    if case == "I_clamped":
        assert loop["n_failed"].tolist() == [1, 0] and np.isinf(loop["lam"][-1])


# ---------------------------------------------------------------------------
# 2. run_events equals the event() loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(CASES))
def test_run_equals_loop(engine, case, pc):
    from mfea import EVENTS_COMPLETE, EVENTS_LAMBDA_MAX, EVENTS_UNLOADED
    loop, run, out, pinned, direct = _pair(engine, case, pc)
    m = run["n_done"]
    assert m == len(loop["lam"])
    for k in ("lam", "force1"):
        assert same_bits(run[k], loop[k]), k
    for k in ("n_failed", "n_active"):
        assert np.array_equal(run[k], loop[k]), k
    assert same_bits(run["stress"], loop["stress"])
    assert np.array_equal(run["active"], loop["active"])
    with np.errstate(invalid="ignore"):
        assert same_bits(run["U"], loop["lam"][:, None] * loop["U1"])
    # rows >= n_done keep their sentinels
    assert np.all(out["U"][m:] == SENT_F) and np.all(out["stress"][m:] == SENT_F)
    assert np.all(out["active"][m:] == SENT_B)
    # event_of against the activity rows
    ev = run["event_of"]
    assert ev.dtype == np.int32 and ev.shape == (len(loop["active"][0]),)
    expect = np.full(ev.shape, -1, dtype=np.int32)
    for k in range(m):
        expect[loop["group"][k]] = k
    assert np.array_equal(ev, expect)
    assert np.array_equal(ev < 0, run["active"][-1])
    if run["n_failed"][-1] == 0:
        want = EVENTS_UNLOADED if np.isinf(run["lam"][-1]) else EVENTS_LAMBDA_MAX
        assert run["stop_reason"] == want
        if want == EVENTS_LAMBDA_MAX:
            assert run["lam"][-1] > CASES[case][3]
    else:
        assert run["stop_reason"] == EVENTS_COMPLETE and m == CASES[case][5]
    # the pinned-slab path copies the same rows
    assert direct in (0, 1)
    for k in ("U", "stress", "lam", "force1"):
        assert same_bits(pinned[k], run[k]), k
    assert np.array_equal(pinned["active"], run["active"])
    assert np.array_equal(pinned["event_of"], ev) and pinned["stop_reason"] == run["stop_reason"]


@pytest.mark.parametrize("pc", [3, 4])  # MFEA_PC_SOR, MFEA_PC_ICC
def test_event_behind_a_chunked_solve(engine, pc):
    """SOR / ICC solves go on in chunks past the batch the event pair was
    enqueued behind: the pair is undone (activity, event_of, the failure list)
    and runs again after the solve.  The rule holds bit for bit at every event
    and the run's event_of names each element's event once."""
    mesh, grip, dref = "sim_20251115_135507", 0.5, 0.02
    loop = event_loop(engine, mesh, grip, dref, 1.0, 1e-9, 6, pc, rtol=1e-10)
    assert loop["n_failed"].tolist() == [1, 1, 1, 0]
    _start(engine, mesh, grip)
    run = engine.run_events(dref, -dref, _opts(pc, 1e-10), MAX_STRAIN, 1e-9, 1.0, n_events=6, keep=("active",))
    assert run["n_done"] == 4 and same_bits(run["lam"], loop["lam"])
    expect = np.full(run["event_of"].shape, -1, dtype=np.int32)
    for k in range(3):
        expect[loop["group"][k]] = k
    assert np.array_equal(run["event_of"], expect)
    assert np.array_equal(run["active"], loop["active"])


# ---------------------------------------------------------------------------
# 3. the oracle sequence: direct solves with the same rule
# ---------------------------------------------------------------------------
TIE3 = 1e-6


def oracle_sequence(mesh, grip, dref, lam_max, n_max):
    """fo.assemble_global_stiffness + fo.solve_system per event with the rule
    of include/mfea.h at tie_rtol 1e-6.  Asserts the oracle's own band: the
    failing group lies within 1e-12 of smax, every other active element at
    least 5e-5 below it — so a device solve at rtol 1e-13 classifies alike and
    lam agrees far inside 1e-6."""
    xyz, e2n, top, bot = _mesh(mesh, grip)
    act = np.ones(len(e2n), bool)
    seq, stop = [], "complete"
    known, vals = fo.known_dof_map(top, bot, dref, -dref)
    for _ in range(n_max):
        if not act.any():
            stop = "unloaded"
            break
        K = fo.assemble_global_stiffness(xyz, e2n, act)
        U = fo.solve_system(K, known, vals)
        f1 = (K @ U)[[3 * n + 1 for n in top]].sum()
        eps = fo.element_strain(xyz, e2n, U)
        smax, lam, group, _ = rule(eps, act, MAX_STRAIN, TIE3, lam_max)
        if not group.any():
            stop = "unloaded" if smax == 0.0 else "lam_max"
            break
        a = np.abs(eps)
        assert ((smax - a[group]) / smax).max() <= 1e-12, "oracle band: inside"
        rest = act & ~group & ~np.isnan(a)
        if rest.any():
            assert ((smax - a[rest]) / smax).min() >= 5e-5, "oracle band: outside"
        seq.append((lam, lam * f1, group))
        act = act & ~group
    return seq, stop


_oracle = {}


@pytest.mark.parametrize("pc", PCS)
@pytest.mark.parametrize("case", list(ORACLE))
def test_oracle_sequence(engine, case, pc):
    from mfea import EVENTS_LAMBDA_MAX, EVENTS_UNLOADED
    mesh, grip, dref, lam_max, n_fail, stop = ORACLE[case]
    n = n_fail + 2
    if case not in _oracle:
        _oracle[case] = oracle_sequence(mesh, grip, dref, lam_max, n)
    seq, ostop = _oracle[case]
    assert len(seq) == n_fail and ostop == stop
    _start(engine, mesh, grip)
    with engine.options(amg_rebuild_rent=0):
        run = engine.run_events(dref, -dref, _opts(pc), MAX_STRAIN, TIE3, lam_max, n_events=n, keep=("active",))
    assert run["n_done"] == n_fail + 1
    assert run["stop_reason"] == {"unloaded": EVENTS_UNLOADED, "lam_max": EVENTS_LAMBDA_MAX}[stop]
    prev = np.ones(len(seq[0][2]), bool)
    for k, (lam, force, group) in enumerate(seq):
        assert np.array_equal(prev & ~run["active"][k], group), k
        prev = run["active"][k]
        assert abs(run["lam"][k] - lam) <= 1e-6 * abs(lam), (k, run["lam"][k], lam)
        got = run["lam"][k] * run["force1"][k]
        assert abs(got - force) <= 1e-6 * abs(force), (k, got, force)
    if case == "X":
        assert [int(g.sum()) for _, _, g in seq] == [2, 4, 8]
        assert np.allclose([s[0] for s in seq], [0.3, 0.375, 0.6], rtol=1e-12)
    if case == "planar":
        from mfea import event_envelope
        lam = run["lam"][:n_fail]
        assert abs(lam[0] - 0.4625) < 1e-4 and np.any(np.diff(lam) < 0)  # avalanches
        disp, force = event_envelope(lam, run["force1"][:n_fail], 2 * dref)
        assert np.all(np.diff(disp) >= 0) and disp[-1] == lam.max() * 2 * dref


# ---------------------------------------------------------------------------
# 4. the reference's committed ramps: event 0 falls inside the first failing step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gen,mesh", [("gen_sim_20251117_175809_default.npz", "sim_20251117_175809"),
                                      ("gen_sim_20251115_135507_grip05.npz", "sim_20251115_135507")])
def test_first_event_inside_the_ramp_step(engine, gen, mesh):
    g = load_gen(gen)
    n, dmax, grip = int(g["n_steps"]), float(g["dmax"]), float(g["grip"])
    n_act = g["active"].sum(axis=1)
    k = int(np.flatnonzero(n_act < g["active"].shape[1])[0])  # first ramp step with a failure
    failed_k = ~g["active"][k]
    dref = dmax
    _start(engine, mesh, grip)
    with engine.options(amg_rebuild_rent=0):
        run = engine.run_events(dref, -dref, _opts(GAMG), MAX_STRAIN, 1e-9, np.inf, n_events=1, keep=("active",))
    lam0 = run["lam"][0]
    # step k - 1 did not exceed max_strain (strict >), step k did
    assert dmax * (k - 1) / (n - 1) <= lam0 * dref < dmax * k / (n - 1)
    group = ~run["active"][0]
    assert group.any() and not np.any(group & ~failed_k)


# ---------------------------------------------------------------------------
# 5. a long uncapped run: past rupture, floating pieces under the kept hierarchy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
def test_long_uncapped_run_invariants(engine, pc):
    mesh, grip, dref = "sim_20251115_135507", 0.5, 0.02
    with engine.options(amg_rebuild_rent=0):
        a = event_loop(engine, mesh, grip, dref, np.inf, 1e-9, 40, pc, floating=True)
        b = event_loop(engine, mesh, grip, dref, np.inf, 1e-9, 40, pc, check=False, floating=True)
    assert len(a["lam"]) == 40 or (a["n_failed"][-1] == 0 and np.isinf(a["lam"][-1]))
    for k in ("lam", "force1", "U1", "stress"):
        assert same_bits(a[k], b[k]), k
    assert np.array_equal(a["active"], b["active"])


# ---------------------------------------------------------------------------
# 6. no side effects on the step path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PCS)
def test_events_leave_the_step_path_alone(engine, pc):
    from mfea import Engine
    mesh, grip, dref = "sim_20251115_135507", 0.5, 0.02
    dy = np.array([dref * (k / 39) for k in range(40)])
    _start(engine, mesh, grip)
    with engine.options(amg_rebuild_rent=0):
        engine.run_events(dref, -dref, _opts(pc), MAX_STRAIN, 1e-9, 1.0, n_events=5, keep=())
        engine.set_active(None)
        after = engine.run(dy, -dy, _opts(pc), MAX_STRAIN)
    with Engine(0) as fresh:
        _start(fresh, mesh, grip)
        with fresh.options(amg_rebuild_rent=0):
            ref = fresh.run(dy, -dy, _opts(pc), MAX_STRAIN)
    assert after["n_done"] == ref["n_done"] and after["stop_reason"] == ref["stop_reason"]
    for k in ("U", "stress", "force"):
        assert same_bits(after[k], ref[k]), k
    assert np.array_equal(after["active"], ref["active"])
    assert np.array_equal(after["n_active"], ref["n_active"])


# ---------------------------------------------------------------------------
# 7. the drop-in
# ---------------------------------------------------------------------------
def test_dropin_events_writes_the_records(tmp_path, engine):
    import fea_solver as fs
    mesh, grip = "sim_20251115_135507", 0.5
    d = tmp_path / mesh
    shutil.copytree(os.path.join(GOLDEN, "meshes", mesh), d)
    with fs.get_engine().options(amg_rebuild_rent=0):
        fs.main([str(d), "--events", "--grip-length", str(grip), "--npy"])
    out = d / "fea_results"
    _start(engine, mesh, grip)
    with engine.options(amg_rebuild_rent=0):
        run = engine.run_events(fs.DISPLACEMENT_MAX, -fs.DISPLACEMENT_MAX, fs._opts(), fs.MAX_STRAIN, 1e-9, 1.0)
    m = run["n_done"]
    assert m == 4
    lines = (out / "failure_events.csv").read_text().splitlines()
    assert lines[0] == "event,lam,total_displacement,total_force,n_failed,n_active" and len(lines) == 1 + m
    span = 2 * fs.DISPLACEMENT_MAX
    for k, ln in enumerate(lines[1:]):
        ev, lam, disp, force, nf, na = ln.split(",")
        assert int(ev) == k + 1 and int(nf) == run["n_failed"][k] and int(na) == run["n_active"][k]
        assert same_bits(float(lam), run["lam"][k])
        assert same_bits(float(disp), run["lam"][k] * span)
        assert same_bits(float(force), run["lam"][k] * run["force1"][k])
    for f in ("force_displacement.csv", "stress_record.csv", "node_displacements.csv", "active_elements.csv"):
        assert len(read_rt(out / f)) == m, f
    fd = read_rt(out / "force_displacement.csv")
    assert same_bits(fd["total_displacement"].values, run["lam"] * span)
    assert np.array_equal(np.load(out / "event_of.npy"), run["event_of"])
