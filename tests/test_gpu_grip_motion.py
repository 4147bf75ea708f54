"""Grip motion vectors (mfea_set_grip_motion): shear, mixed-mode and
out-of-plane tests on every entry point.

The checker is the oracle's own assembly and direct solve: fo.solve_system
takes arbitrary prescribed values, so known_vals is built here top-then-bottom
as fo.known_dof_map builds it, from dy * t[c] as NumPy multiplies it.  The
event semantics of include/mfea.h are single IEEE operations on the device's
own U, so NumPy reproduces them bit for bit (the rule of test_gpu_events.py);
the default state (0,1,0), (0,1,0) is bit equality with a handle that never
called the setter."""
import numpy as np
import pytest

from conftest import load_mesh
from test_gpu_events import rule
from test_gpu_props import GRAPHS_OFF, GRAPHS_ON, het_K, recipe, same_bits

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

MAX_STRAIN = 0.018
JACOBI, BJACOBI, GAMG, SOR, ICC = 0, 1, 2, 3, 4
X, PLANAR, SIM3D = "test_X", "sim_20251117_175809", "sim_20251115_135507"
GRIP = {X: 0.5, PLANAR: 1.5, SIM3D: 0.5}
EX, EY, EZ = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
MIX2, MIX3 = (0.6, 0.8, 0.0), (0.48, 0.6, 0.64)
AMP = 0.05
U_ROUND = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from mfea import Engine
    e = Engine(0)
    e.set_option("amg_rebuild_rent", 0)
    yield e
    e.close()


_meshes, _K, _ref = {}, {}, {}


def mesh_of(name):
    if name not in _meshes:
        nodes, elems = load_mesh(name)
        xyz = nodes[["x", "y", "z"]].values
        e2n = elems[["n1", "n2"]].values
        top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, GRIP[name])
        _meshes[name] = (xyz, e2n, top, bot)
    return _meshes[name]


def K_of(name):
    """The oracle's K of the whole (all active) network, once per mesh."""
    if name not in _K:
        xyz, e2n, _, _ = mesh_of(name)
        _K[name] = fo.assemble_global_stiffness(xyz, e2n, np.ones(len(e2n), bool)).tocsr()
    return _K[name]


def known_map(top, bot, dy_top, dy_bot, t, b):
    """fo.known_dof_map with the grip vectors: filled top-then-bottom, a node
    in both bands takes the bottom value; each value one f64 product."""
    t, b = np.asarray(t, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = {}
    for n in top:
        d.update({3 * n + c: np.float64(dy_top) * t[c] for c in range(3)})
    for n in bot:
        d.update({3 * n + c: np.float64(dy_bot) * b[c] for c in range(3)})
    known = np.array(list(d.keys()), dtype=np.int64)
    return known, np.array([d[k] for k in known], dtype=np.float64)


def oracle(name, dy_top, dy_bot, t, b, K=None):
    """The direct solve, once per case (K given: not cached)."""
    key = (name, dy_top, dy_bot, tuple(t), tuple(b))
    if K is not None or key not in _ref:
        _, _, top, bot = mesh_of(name)
        known, vals = known_map(top, bot, dy_top, dy_bot, t, b)
        U = fo.solve_system(K_of(name) if K is None else K, known, vals)
        if K is not None:
            return U
        _ref[key] = U
    return _ref[key]


def start(e, name, t=EY, b=EY, props=None):
    xyz, e2n, top, bot = mesh_of(name)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot)
    e.set_active(None)
    e.set_grip_motion(t, b)
    if props is not None:
        e.set_element_props(**props)
    return xyz, e2n, top, bot


def opts(pc, rtol=1e-13):
    """rtol 1e-13; SOR / ICC on PETSc's preconditioned norm, their KSPCG default,
    as the project's tests of the sweep preconditioners state their bar."""
    from mfea import make_opts
    return make_opts(precond=pc, rtol=rtol, max_it=200000, norm=1 if pc in (SOR, ICC) else 0)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def grip_rows_exact(U, top, bot, dy_top, dy_bot, t, b):
    """U at the grip nodes equals dy * t[c] as NumPy multiplies it."""
    U3 = U.reshape(-1, 3)
    bot_set = set(int(n) for n in bot)
    only_top = np.array([n for n in top if int(n) not in bot_set], dtype=np.int64)
    want_t = np.float64(dy_top) * np.asarray(t, dtype=np.float64)
    want_b = np.float64(dy_bot) * np.asarray(b, dtype=np.float64)
    return (np.array_equal(U3[only_top], np.broadcast_to(want_t, (len(only_top), 3))) and
            np.array_equal(U3[bot], np.broadcast_to(want_b, (len(bot), 3))))


def work_force(t, S):
    """include/mfea.h: F = (top[0]·S[0] + top[1]·S[1]) + top[2]·S[2], f64."""
    t, S = np.asarray(t, dtype=np.float64), np.asarray(S, dtype=np.float64)
    return (t[0] * S[0] + t[1] * S[1]) + t[2] * S[2]


def reaction_ref(K, U, band):
    """Per component: the band's Σ (K·U)[3n+c] in extended precision, and the
    standard dot-product bound γ_n · Σ|K_ij|·|U_j| with n = the stored terms of
    the band's rows plus the row count."""
    ref, bound = np.zeros(3), np.zeros(3)
    Ul, Ua = U.astype(np.longdouble), np.abs(U)
    for c in range(3):
        rows = np.array([3 * int(n) + c for n in band], dtype=np.int64)
        Kb = K[rows].tocsr()
        ref[c] = float(np.sum(Kb.data.astype(np.longdouble) * Ul[Kb.indices]))
        n = Kb.nnz + len(rows)
        gamma = n * U_ROUND / (1.0 - n * U_ROUND)
        bound[c] = gamma * float(np.sum(np.abs(Kb.data) * Ua[Kb.indices]))
    return ref, bound


# ---------------------------------------------------------------------------
# 1. parity with the direct solve, through mfea_solve and through mfea_step
# ---------------------------------------------------------------------------
CASES = [(PLANAR, EX, EY, -AMP), (PLANAR, MIX2, EY, -AMP), (SIM3D, EX, EY, -AMP), (SIM3D, MIX2, EY, -AMP),
         (SIM3D, MIX3, EZ, -0.03)]
PARITY = ([(m, t, b, d, pc) for (m, t, b, d) in CASES for pc in (JACOBI, BJACOBI, GAMG, SOR, ICC)] +
          [(X, t, EY, -AMP, pc) for t in (EX, MIX2) for pc in (GAMG, JACOBI)])


@pytest.mark.parametrize("mesh,t,b,dy_bot,pc", PARITY)
def test_parity(eng, mesh, t, b, dy_bot, pc):
    _, _, top, bot = start(eng, mesh, t, b)
    Uref = oracle(mesh, AMP, dy_bot, t, b)
    gt, gb = eng.grip_motion()
    assert gt.tolist() == list(t) and gb.tolist() == list(b)
    # the separate RHS kernel: mfea_solve after mfea_assemble
    eng.assemble()
    st = eng.solve(AMP, dy_bot, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    print(f"{mesh} t={t} pc {pc}: solve iters {st.iters} rel {rel(U, Uref):.3e}")
    assert rel(U, Uref) <= 1e-10, (mesh, t, pc, rel(U, Uref))
    assert grip_rows_exact(U, top, bot, AMP, dy_bot, t, b)
    # the fused RHS of the assembly, then (K and the hierarchy kept) k_amg_start
    for k in range(2):
        _, _, st = eng.step(AMP, dy_bot, opts(pc), 1.0)
        assert st.status == 0
        U = eng.displacement()
        print(f"  step {k}: iters {st.iters} rel {rel(U, Uref):.3e}")
        assert rel(U, Uref) <= 1e-10, (mesh, t, pc, k, rel(U, Uref))
        assert grip_rows_exact(U, top, bot, AMP, dy_bot, t, b)


# ---------------------------------------------------------------------------
# 2. an out-of-plane motion on a planar mesh: 3 DOFs per node, and back
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_planar_z(eng, pc):
    from mfea import Engine
    _, _, top, bot = start(eng, PLANAR, EZ, EY)
    assert eng.info()["planar"] == 1
    eng.assemble()
    st = eng.solve(AMP, -AMP, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    Uref = oracle(PLANAR, AMP, -AMP, EZ, EY)
    print(f"planar z pc {pc}: iters {st.iters} rel {rel(U, Uref):.3e}")
    assert rel(U, Uref) <= 1e-10
    assert grip_rows_exact(U, top, bot, AMP, -AMP, EZ, EY)
    assert np.any(U.reshape(-1, 3)[:, 2] != 0.0)
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 3  # the handle was rebuilt with 3 DOFs per node
    # back to the tensile test: the 2-DOF path, the bits of a fresh handle
    eng.set_grip_motion(EY, EY)
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2
    U2 = eng.displacement()
    with Engine(0) as f:
        f.set_option("amg_rebuild_rent", 0)
        xyz, e2n, top, bot = mesh_of(PLANAR)
        f.set_mesh(xyz, e2n)
        f.set_bc(top, bot)
        f.set_active(None)
        f.assemble()
        assert f.solve(AMP, -AMP, opts(pc)).status == 0
        assert same_bits(U2, f.displacement())
    assert not np.any(U2.reshape(-1, 3)[:, 2])


# ---------------------------------------------------------------------------
# 3. the default state is the tensile engine, bit for bit
# ---------------------------------------------------------------------------
def _record(e):
    """step, run (3 steps), run_events (3 events) from a fresh build."""
    xyz, e2n, top, bot = mesh_of(PLANAR)

    def fresh():
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
    out = {}
    for pc, graphs, tag in ((GAMG, GRAPHS_ON, "gamg_on"), (GAMG, GRAPHS_OFF, "gamg_off"), (JACOBI, {}, "jacobi")):
        with e.options(**graphs):
            fresh()
            f, n, st = e.step(0.012, -0.012, opts(pc, 1e-12), MAX_STRAIN)
            out[tag, "step"] = (f, n, st.iters, e.displacement(), e.stress(), e.active())
            fresh()
            dys = np.array([0.006, 0.012, 0.018])
            out[tag, "run"] = e.run(dys, -dys, opts(pc, 1e-12), MAX_STRAIN)
            fresh()
            out[tag, "events"] = e.run_events(0.02, -0.02, opts(pc, 1e-12), MAX_STRAIN, 1e-9, 1.0, n_events=3)
    return out


def _same_record(a, b):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if key[1] == "step":
            assert same_bits(x[0], y[0]) and x[1] == y[1] and x[2] == y[2], key
            assert same_bits(x[3], y[3]) and same_bits(x[4], y[4]) and np.array_equal(x[5], y[5]), key
            continue
        assert x["n_done"] == y["n_done"] and x["stop_reason"] == y["stop_reason"], key
        for k in ("U", "stress") + (("force",) if key[1] == "run" else ("lam", "force1")):
            assert same_bits(x[k], y[k]), (key, k)
        assert np.array_equal(x["active"], y["active"]) and np.array_equal(x["n_active"], y["n_active"]), key
        assert [s["iters"] for s in x["stats"]] == [s["iters"] for s in y["stats"]], key


def test_default_identity():
    from mfea import Engine
    with Engine(0) as a:
        a.set_option("amg_rebuild_rent", 0)
        plain = _record(a)
    assert plain["gamg_on", "step"][1] < len(mesh_of(PLANAR)[1])  # elements failed
    assert plain["gamg_on", "events"]["n_failed"][0] > 0
    with Engine(0) as b:  # the default, set explicitly
        b.set_option("amg_rebuild_rent", 0)
        b.set_grip_motion(EY, EY)
        _same_record(_record(b), plain)
        t, bt = b.grip_motion()
        assert t.tolist() == list(EY) and bt.tolist() == list(EY)
    with Engine(0) as c:  # ... and come back to from a shear step
        c.set_option("amg_rebuild_rent", 0)
        start(c, PLANAR, EX, EX)
        _, _, st = c.step(0.01, -0.01, opts(GAMG), 1.0)
        assert st.status == 0
        c.set_grip_motion(EY, EY)
        _same_record(_record(c), plain)


# ---------------------------------------------------------------------------
# 4. a change of direction between steps: nothing stale, everything kept
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("phase_times", [0, 1])
@pytest.mark.parametrize("first,second", [(EY, EX), (EX, EY)], ids=["y_then_x", "x_then_y"])
def test_change_between_steps(eng, first, second, phase_times):
    K = K_of(PLANAR)
    _, _, top, _ = mesh_of(PLANAR)
    d = 0.01
    with eng.options(**GRAPHS_ON, phase_times=phase_times):
        start(eng, PLANAR, first, EY)
        for _ in range(2):  # (the second replays what the first captured / kept)
            f0, _, st = eng.step(d, -d, opts(GAMG), 1.0)
            assert st.status == 0
        assert rel(eng.displacement(), oracle(PLANAR, d, -d, first, EY)) <= 1e-10
        kept = eng.get_option("op_kept_steps"), eng.get_option("amg_setup_kept")
        eng.set_grip_motion(second, None)
        for k in range(2):
            f1, _, st = eng.step(d, -d, opts(GAMG), 1.0)
            assert st.status == 0 and st.amg_rebuilt == 0
            U = eng.displacement()
            assert rel(U, oracle(PLANAR, d, -d, second, EY)) <= 1e-10, (k, rel(U, oracle(PLANAR, d, -d, second, EY)))
            # a kept step: no assembly, no numeric setup
            assert eng.get_option("op_kept_steps") == kept[0] + k + 1
            assert eng.get_option("amg_setup_kept") == kept[1] + k + 1
            if phase_times:
                assert st.t_setup_ms == 0
            ref, bound = reaction_ref(K, U, top)
            assert abs(f1 - work_force(second, ref)) <= np.abs(second) @ bound + 4 * U_ROUND * abs(f1), k
            assert same_bits(f1, work_force(second, eng.reaction()[0]))
        assert f1 != f0


# ---------------------------------------------------------------------------
# 5. the reaction vector of both bands, and the work-conjugate force
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,t,b,dy_bot", [(PLANAR, EX, EY, -AMP), (PLANAR, MIX2, EY, -AMP), (PLANAR, EY, EY, -AMP),
                                             (SIM3D, MIX3, EZ, -0.03), (X, MIX2, EY, -AMP)])
def test_reaction(eng, mesh, t, b, dy_bot):
    _, _, top, bot = start(eng, mesh, t, b)
    K = K_of(mesh)
    f, _, st = eng.step(AMP, dy_bot, opts(GAMG), 1.0)
    assert st.status == 0
    U = eng.displacement()
    top3, bot3 = eng.reaction()
    bot_set = set(int(n) for n in bot)
    bands = ([n for n in top if int(n) not in bot_set], bot)  # (a node in both bands counts in the bottom one)
    for got, band in zip((top3, bot3), bands):
        ref, bound = reaction_ref(K, U, band)
        print(f"{mesh} t={t}: got {got} ref {ref} err {np.abs(got - ref)} bound {bound}")
        assert np.all(np.abs(got - ref) <= bound), (got, ref, bound)
    # the step's force: the header's expression on the device's own sums, bit
    # for bit; against the checker within the sums' bounds and the three
    # roundings of the expression
    assert same_bits(f, work_force(t, top3))
    ref, bound = reaction_ref(K, U, bands[0])
    assert abs(f - work_force(t, ref)) <= np.abs(t) @ bound + 4 * U_ROUND * np.abs(t) @ np.abs(ref)
    # NULL for either argument
    from mfea._capi import _lib, _ptr
    only = np.empty(3)
    assert _lib.mfea_get_reaction(eng._h, _ptr(only), None) == 0 and same_bits(only, top3)
    assert _lib.mfea_get_reaction(eng._h, None, _ptr(only)) == 0 and same_bits(only, bot3)
    assert _lib.mfea_get_reaction(eng._h, None, None) == 0
    if tuple(t) == EY:  # the tensile test: the y sum is total_force itself
        assert same_bits(f, top3[1])
        assert same_bits(eng.post(np.inf)[0], top3[1])


# ---------------------------------------------------------------------------
# 6. linearity in the direction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [PLANAR, SIM3D])
def test_linearity(eng, mesh):
    a, b = 0.6, 0.8
    U = {}
    for name, t in (("x", EX), ("y", EY), ("mix", (a, b, 0.0))):
        start(eng, mesh, t, EY)
        eng.assemble()
        # the bottom grip holds still: U is linear in the top direction alone
        assert eng.solve(AMP, 0.0, opts(GAMG)).status == 0
        U[name] = eng.displacement()
    assert rel(U["mix"], a * U["x"] + b * U["y"]) <= 1e-10


# ---------------------------------------------------------------------------
# 7. runs and events under shear
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_run_equals_step_loop_under_shear(eng, pc):
    dys = np.array([0.01, 0.02, 0.03, 0.04])
    n = len(mesh_of(PLANAR)[1])
    start(eng, PLANAR, EX, EY)
    loop = []
    for d in dys:
        f, na, st = eng.step(d, -d, opts(pc, 1e-12), MAX_STRAIN)
        assert st.status == 0
        loop.append((f, na, st.iters, eng.displacement(), eng.stress(), eng.active()))
    assert loop[-1][1] < n  # at least one step fails an element
    start(eng, PLANAR, EX, EY)
    run = eng.run(dys, -dys, opts(pc, 1e-12), MAX_STRAIN)
    assert run["n_done"] == len(dys)
    for k, row in enumerate(loop):
        assert same_bits(run["force"][k], row[0]) and run["n_active"][k] == row[1], k
        assert run["stats"][k]["iters"] == row[2], k
        assert same_bits(run["U"][k], row[3]) and same_bits(run["stress"][k], row[4]), k
        assert np.array_equal(run["active"][k], row[5]), k


@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_events_under_shear(eng, pc):
    from mfea import EVENTS_COMPLETE
    dref, tie, lam_max, n_events = 0.02, 1e-9, np.inf, 4
    xyz, e2n, top, _ = start(eng, PLANAR, EX, EY)
    rec = {k: [] for k in ("lam", "force1", "U1", "stress", "active", "n_failed")}
    for k in range(n_events):
        act0 = eng.active()
        lam, f1, nf, na, st = eng.event(dref, -dref, opts(pc), MAX_STRAIN, tie, lam_max)
        assert st.status == 0
        U1, stress, act1 = eng.displacement(), eng.stress(), eng.active()
        eps = fo.element_strain(xyz, e2n, U1)
        _, lam_np, group, stress_np = rule(eps, act0, MAX_STRAIN, tie, lam_max)
        assert same_bits(lam, lam_np), (k, lam, lam_np)
        assert nf == int(group.sum()) > 0 and na == int(act1.sum()), k
        assert np.array_equal(act1, act0 & ~group), k
        assert same_bits(stress, stress_np), k
        # F₁: the work-conjugate force of the event's own K and U₁
        assert same_bits(f1, work_force(EX, eng.reaction()[0])), k
        assert same_bits(f1, eng.post(np.inf)[0]), k
        for key, v in zip(rec, (lam, f1, U1, stress, act1, nf)):
            rec[key].append(v)
    start(eng, PLANAR, EX, EY)
    run = eng.run_events(dref, -dref, opts(pc), MAX_STRAIN, tie, lam_max, n_events=n_events)
    assert run["n_done"] == n_events and run["stop_reason"] == EVENTS_COMPLETE
    assert same_bits(run["lam"], rec["lam"]) and same_bits(run["force1"], rec["force1"])
    assert same_bits(run["stress"], rec["stress"]) and np.array_equal(run["active"], rec["active"])
    assert same_bits(run["U"], np.asarray(rec["lam"])[:, None] * np.asarray(rec["U1"]))
    assert np.array_equal(run["n_failed"], rec["n_failed"])


def test_event_out_of_plane_is_unloaded(eng):
    """Pure z on the planar mesh: the axial strain of an out-of-plane motion is
    zero to first order — one event, terminal, MFEA_EVENTS_UNLOADED."""
    from mfea import EVENTS_UNLOADED
    start(eng, PLANAR, EZ, EZ)
    run = eng.run_events(0.02, -0.02, opts(GAMG), MAX_STRAIN, 1e-9, np.inf, n_events=4)
    assert run["n_done"] == 1 and run["stop_reason"] == EVENTS_UNLOADED
    assert np.isinf(run["lam"][0]) and run["n_failed"][0] == 0 and run["active"][0].all()


@pytest.mark.parametrize("mode", ["loop", "device_run", "events"])
def test_dropin_under_shear(tmp_path, monkeypatch, mode):
    """fea_solver(..., grip_direction=...) on test_X: the records of a shear
    ramp against the oracle's shear solves; the process-wide handle is back at
    the tensile test after a call without the argument."""
    import os
    import shutil
    import fea_solver as fs
    from conftest import GOLDEN
    d = str(tmp_path / "test_X")
    shutil.copytree(os.path.join(GOLDEN, "meshes", X), d)
    monkeypatch.setattr(fs, "N_STEPS", 3)
    monkeypatch.setattr(fs, "DISPLACEMENT_MAX", 0.004)
    kw = dict(tol=GRIP[X], verbose=False, device_run=mode == "device_run", events=mode == "events")
    res = fs.fea_solver(d, grip_direction="1,0,0", **kw)
    t, b = fs.get_engine().grip_motion()
    assert t.tolist() == list(EX) and b.tolist() == list(EX)
    _, _, top, bot = mesh_of(X)
    top = [n for n in top if n not in set(bot)]
    if mode == "events":  # the row of an event: lam · U₁, the curve's first column lam · span
        assert len(res["U"]) >= 1
        U1 = oracle(X, 0.004, -0.004, EX, EX)
        lam = res["force"][0, 0] / 0.008
        assert rel(res["U"][0], lam * U1) <= 1e-10
    else:
        assert res["U"].shape[0] == 3
        for k in range(3):
            dy = 0.004 * (k / 2)
            if k:
                assert rel(res["U"][k], oracle(X, dy, -dy, EX, EX)) <= 1e-10, k
            ref, bound = reaction_ref(K_of(X), res["U"][k], top)
            assert abs(res["force"][k, 1] - ref[0]) <= bound[0] + 4 * U_ROUND * abs(ref[0]), k
            assert res["force"][k, 0] == dy - (-dy)
    assert os.path.exists(os.path.join(d, "fea_results", "force_displacement.csv"))
    fs.fea_solver(d, **kw)
    t, b = fs.get_engine().grip_motion()
    assert t.tolist() == list(EY) and b.tolist() == list(EY)


# ---------------------------------------------------------------------------
# 8. with per-element properties
# ---------------------------------------------------------------------------
def test_with_properties(eng):
    xyz, e2n, top, bot = mesh_of(PLANAR)
    n = len(e2n)
    A, I, strength = recipe(n)  # noqa: E741
    K = het_K(xyz, e2n, np.ones(n, bool), fo.E_MOD, A, I)
    d = 0.01
    Uref = oracle(PLANAR, d, -d, EX, EY, K=K)
    start(eng, PLANAR, EX, EY, props=dict(A=A, I=I, max_strain=strength))
    f, _, st = eng.step(d, -d, opts(GAMG), 1.0)  # (the strength array rules: elements may fail)
    assert st.status == 0
    U = eng.displacement()
    assert rel(U, Uref) <= 1e-10, rel(U, Uref)
    ref, bound = reaction_ref(K, U, [t for t in top if t not in set(bot)])
    assert abs(f - work_force(EX, ref)) <= np.abs(EX) @ bound + 4 * U_ROUND * abs(f)
    # one event: U₁ against the same solve, lam = min max_strain_e / |ε_e|
    start(eng, PLANAR, EX, EY, props=dict(A=A, I=I, max_strain=strength))
    lam, f1, nf, _, st = eng.event(d, -d, opts(GAMG), MAX_STRAIN, 1e-9, np.inf)
    assert st.status == 0 and nf >= 1
    U1 = eng.displacement()
    assert rel(U1, Uref) <= 1e-10, rel(U1, Uref)
    a = np.abs(fo.element_strain(xyz, e2n, U1))
    m = ~np.isnan(a) & (a > 0)
    assert same_bits(lam, np.min(strength[m] / a[m]))
    assert same_bits(f1, work_force(EX, eng.reaction()[0]))


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_errors():
    from mfea import Engine, MfeaError
    from mfea._capi import EINVAL, ESTATE, _lib, _ptr
    xyz, e2n, top, bot = mesh_of(X)
    with Engine(0) as e:
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_grip_motion(MIX2, EZ)
        for bad_t, bad_b in (((np.nan, 0, 0), None), (None, (0, np.inf, 0)), ((0, 0, 0), None), (None, (0.0, -0.0, 0)),
                             (EX, (0, 0, 0)), ((1, -np.inf, 0), EX)):
            with pytest.raises(MfeaError) as err:
                e.set_grip_motion(bad_t, bad_b)
            assert err.value.code == EINVAL, (bad_t, bad_b)
            t, b = e.grip_motion()  # the handle is unchanged
            assert t.tolist() == list(MIX2) and b.tolist() == list(EZ)
        # the getter accepts NULL for either argument
        one = np.empty(3)
        assert _lib.mfea_get_grip_motion(e._h, _ptr(one), None) == 0 and one.tolist() == list(MIX2)
        assert _lib.mfea_get_grip_motion(e._h, None, _ptr(one)) == 0 and one.tolist() == list(EZ)
        assert _lib.mfea_get_grip_motion(e._h, None, None) == 0
        # None leaves a direction as it is
        e.set_grip_motion(None, EX)
        t, b = e.grip_motion()
        assert t.tolist() == list(MIX2) and b.tolist() == list(EX)
        # the other setters keep the directions
        e.set_material(fo.E_MOD, fo.AREA, fo.INERTIA)
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_element_props(A=np.full(len(e2n), fo.AREA))
        t, b = e.grip_motion()
        assert t.tolist() == list(MIX2) and b.tolist() == list(EX)
        e.set_element_props()
        # a non-default direction, then partitions: MFEA_ESTATE at the next build
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.assemble()
        assert err.value.code == ESTATE
    with Engine(0) as e:  # partitions first: the setter refuses
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.set_grip_motion(EX, None)
        assert err.value.code == ESTATE
        t, b = e.grip_motion()
        assert t.tolist() == list(EY) and b.tolist() == list(EY)
        e.set_active(None)
        e.assemble()  # the default direction: the partitioned handle builds and runs
        assert e.solve(0.01, -0.01, opts(JACOBI)).status == 0
