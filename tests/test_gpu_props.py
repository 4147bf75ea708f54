"""Per-element section, modulus and failure strain (mfea_set_element_props).

The checker builds the heterogeneous K itself: fo.bar_stiffness_bulk
broadcasts over array E, A, I (12 * E * I is (12·E)·I elementwise, the engine's
rounding), its Ke go through the COO → csr_matrix construction of
fo.assemble_global_stiffness, and fo.solve_system solves.  The post and event
semantics of include/mfea.h are single IEEE operations on the device's own U,
so NumPy reproduces them bit for bit; the uniform identity (arrays filled with
the scalars) is bit equality with the uniform engine."""
import os
import shutil

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_mesh, read_rt

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

MAX_STRAIN = 0.018
JACOBI, BJACOBI, GAMG, SOR, ICC = 0, 1, 2, 3, 4
X, PLANAR, SIM3D = "test_X", "sim_20251117_175809", "sim_20251115_135507"
GRIP = {X: 0.5, "test_I": 1.5, PLANAR: 1.5, SIM3D: 0.5}
GRAPHS_ON = dict(batch_graph=1, combo_graph=1, step_graph=1, spec_post=1)
GRAPHS_OFF = dict(batch_graph=0, combo_graph=0, step_graph=0, spec_post=0)


# ---------------------------------------------------------------------------
# fixtures of the module: one handle, the meshes, the property recipe
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from mfea import Engine
    e = Engine(0)
    e.set_option("amg_rebuild_rent", 0)
    yield e
    e.close()


_meshes = {}


def mesh_of(name):
    if name not in _meshes:
        nodes, elems = load_mesh(name)
        xyz = nodes[["x", "y", "z"]].values
        e2n = elems[["n1", "n2"]].values
        top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, GRIP[name])
        _meshes[name] = (xyz, e2n, top, bot)
    return _meshes[name]


def recipe(n):
    """The property recipe: sections over a 4× range, Weibull strengths."""
    rng = np.random.default_rng(7)
    s = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n))
    A = fo.AREA * s
    I = A * 0.001  # noqa: E741
    strength = 0.018 * np.clip(rng.weibull(6.0, n), 0.2, None)
    return A, I, strength


def modulus(n):
    """A per-element modulus (beyond the recipe, whose E is the scalar): 0.5–2 × E."""
    return fo.E_MOD * np.exp(np.random.default_rng(11).uniform(np.log(0.5), np.log(2.0), n))


def start(e, name, bc=True, props=None):
    xyz, e2n, top, bot = mesh_of(name)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot) if bc else e.set_bc([], [])
    e.set_active(None)
    if props is not None:
        e.set_element_props(**props)
    return xyz, e2n, top, bot


def opts(pc, rtol=1e-13, norm=0):
    from mfea import make_opts
    return make_opts(precond=pc, rtol=rtol, max_it=200000, norm=norm)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def same_bits(a, b):
    """Bit equality of f64 arrays; NaNs (any payload) match NaNs."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    a, b = np.atleast_1d(a).ravel(), np.atleast_1d(b).ravel()
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and
                np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def _coo(xyz, e2n, active):
    eidx = np.flatnonzero(np.asarray(active, dtype=bool))
    n1, n2 = e2n[eidx, 0], e2n[eidx, 1]
    dof = np.concatenate([3 * n1[:, None] + np.arange(3), 3 * n2[:, None] + np.arange(3)], axis=1)
    return eidx, n1, n2, np.repeat(dof, 6, axis=1).ravel(), np.tile(dof, (1, 6)).ravel()


def _col(v, eidx):
    return v[eidx] if isinstance(v, np.ndarray) else v


def het_K(xyz, e2n, active, E, A, I):  # noqa: E741
    """fo.assemble_global_stiffness with per-element E, A, I: the same triplet
    stream through the same csr_matrix constructor."""
    xyz = np.asarray(xyz, dtype=np.float64)
    eidx, n1, n2, rows, cols = _coo(xyz, e2n, active)
    Ke, _ = fo.bar_stiffness_bulk(xyz[n1], xyz[n2], _col(E, eidx), _col(A, eidx), _col(I, eidx))
    n = 3 * len(xyz)
    return sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(n, n))


def check_het_assembly(dv, Kref, xyz, e2n, active, E, A, I):  # noqa: E741
    """The per-entry bound of tests/test_gpu_parity.py check_assembly, with
    fo.stiffness_magnitude called on each element's own E, A, I."""
    xyz = np.asarray(xyz, dtype=np.float64)
    eidx, n1, n2, rows, cols = _coo(xyz, e2n, active)
    M = fo.stiffness_magnitude(xyz[n1], xyz[n2], _col(E, eidx), _col(A, eidx), _col(I, eidx))
    n = 3 * len(xyz)
    mag = sp.csr_matrix((M.ravel(), (rows, cols)), shape=(n, n)).data
    k = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n)).data
    eps = np.finfo(float).eps
    d = np.abs(dv - Kref.data)
    one = k == 1
    assert np.all(d[one] <= 4 * eps * mag[one])
    wc = one & (np.abs(Kref.data) >= 0.5 * mag)
    ulp = np.spacing(np.abs(Kref.data[wc]))
    assert np.all(d[wc] <= 4 * ulp), np.max(d[wc] / ulp)
    assert np.all(d[~one] <= (k[~one] + 3) * eps * mag[~one])


def force_close(F, Fr):
    """The uniform reaction tests' tolerance (tests/test_gpu_parity.py)."""
    F, Fr = np.asarray(F), np.asarray(Fr)
    return np.all(np.abs(F - Fr) <= 1e-9 * np.max(np.abs(Fr)) + 1e-18)


# ---------------------------------------------------------------------------
# 1. K against the checker's heterogeneous K
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_E", [False, True])
@pytest.mark.parametrize("mesh", [X, SIM3D, PLANAR])
def test_K_matches_the_checker(eng, mesh, with_E):
    xyz, e2n, _, _ = start(eng, mesh, bc=False)
    n = len(e2n)
    A, I, _ = recipe(n)  # noqa: E741
    E = modulus(n) if with_E else fo.E_MOD
    active = np.random.default_rng(5).random(n) > 0.2
    assert not active.all()
    Kref = het_K(xyz, e2n, active, E, A, I)
    eng.set_active(active)
    eng.set_element_props(E=E if with_E else None, A=A, I=I)
    assert eng.get_option("element_props") == 1
    data = {}
    for kern in (0, 1, 2):
        with eng.options(asm_kernel=kern):
            eng.assemble()
            ip, ix, dv = eng.export_csr()
        assert np.array_equal(ip, Kref.indptr) and np.array_equal(ix, Kref.indices), kern
        check_het_assembly(dv, Kref, xyz, e2n, active, E, A, I)
        data[kern] = dv
    # the element pass + row pass sums in the row gather's order: its bits
    assert np.array_equal(data[2], data[0])
    # heterogeneous for real: not the uniform K
    Ku = fo.assemble_global_stiffness(xyz, e2n, active)
    assert not np.allclose(data[0], Ku.data, rtol=1e-3)


# ---------------------------------------------------------------------------
# 2. the uniform identity
# ---------------------------------------------------------------------------
def _filled(n, strength=MAX_STRAIN):
    return dict(E=np.full(n, fo.E_MOD), A=np.full(n, fo.AREA), I=np.full(n, fo.INERTIA),
                max_strain=np.full(n, strength))


def _ramp(e, mesh, pc, props, dys, max_strain=MAX_STRAIN, rtol=1e-12):
    """mfea_step over dys from a fresh build: per step force, n_active, iterations, K, U, stress, activity."""
    start(e, mesh, props=props)
    rec = []
    for d in dys:
        f, n, st = e.step(d, -d, opts(pc, rtol), max_strain)
        assert st.status == 0
        rec.append((f, n, st.iters, e.export_csr()[2], e.displacement(), e.stress(), e.active()))
    return rec


def _same_ramp(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x[0], y[0]), k
        assert x[1] == y[1] and x[2] == y[2], (k, x[1:3], y[1:3])
        for i in (3, 4, 5):
            assert same_bits(x[i], y[i]), (k, i)
        assert np.array_equal(x[6], y[6]), k


@pytest.mark.parametrize("pc", [JACOBI, GAMG])
@pytest.mark.parametrize("mesh,d0", [(X, 0.0055), (PLANAR, 0.004)])
def test_uniform_identity_steps(eng, mesh, d0, pc):
    n = len(mesh_of(mesh)[1])
    dys = [d0 * k for k in range(1, 7)]
    plain = _ramp(eng, mesh, pc, None, dys)
    assert plain[-1][1] < n  # elements failed on the way
    _same_ramp(_ramp(eng, mesh, pc, _filled(n), dys), plain)
    # one column at a time: each of the per-element paths alone
    for key in ("A", "max_strain"):
        _same_ramp(_ramp(eng, mesh, pc, {key: _filled(n)[key]}, dys), plain)


@pytest.mark.parametrize("mesh,dref,lam_max", [(X, 0.06, np.inf), (PLANAR, 0.02, 1.0)])
def test_uniform_identity_events(eng, mesh, dref, lam_max):
    n = len(mesh_of(mesh)[1])
    start(eng, mesh)
    plain = eng.run_events(dref, -dref, opts(GAMG), MAX_STRAIN, 1e-9, lam_max, n_events=8)
    start(eng, mesh, props=_filled(n))
    got = eng.run_events(dref, -dref, opts(GAMG), MAX_STRAIN, 1e-9, lam_max, n_events=8)
    assert got["n_done"] == plain["n_done"] and got["stop_reason"] == plain["stop_reason"]
    assert plain["n_failed"][0] > 0
    for k in ("lam", "force1", "stress", "U"):
        assert same_bits(got[k], plain[k]), k
    # (on these fixtures no element lies within rounding of the group's boundary)
    assert np.array_equal(got["active"], plain["active"])
    assert np.array_equal(got["event_of"], plain["event_of"])


# ---------------------------------------------------------------------------
# 3. the solve on a heterogeneous K
# ---------------------------------------------------------------------------
_direct = {}


def _direct_solve(mesh, dy):
    if mesh not in _direct:
        xyz, e2n, top, bot = mesh_of(mesh)
        A, I, _ = recipe(len(e2n))  # noqa: E741
        K = het_K(xyz, e2n, np.ones(len(e2n), bool), fo.E_MOD, A, I)
        known, vals = fo.known_dof_map(top, bot, dy, -dy)
        Af, b, free = fo.free_system(K, known, vals)
        _direct[mesh] = (K, Af, b, free, fo.solve_system(K, known, vals))
    return _direct[mesh]


@pytest.mark.parametrize("pc", [JACOBI, BJACOBI, GAMG, SOR, ICC])
@pytest.mark.parametrize("mesh", [PLANAR, SIM3D])
def test_solve_matches_direct(eng, mesh, pc):
    """The project's bar (tests/test_gpu_amg.py, tests/test_gpu_sweep.py): rtol
    1e-13 — for SOR / ICC on PETSc's preconditioned norm, their KSPCG default,
    as the uniform sweeps' test states it — U within 1e-10 of the direct solve,
    true residual within 1e-12."""
    dy = 0.01
    K, Af, b, free, Uref = _direct_solve(mesh, dy)
    A, I, _ = recipe(len(mesh_of(mesh)[1]))  # noqa: E741
    start(eng, mesh, props=dict(A=A, I=I))
    eng.assemble()
    st = eng.solve(dy, -dy, opts(pc, 1e-13, norm=1 if pc in (SOR, ICC) else 0))
    assert st.status == 0
    U = eng.displacement()
    print(f"{mesh} pc {pc}: iters {st.iters}, relL2(U) {rel(U, Uref):.3e}, "
          f"residual {np.linalg.norm(Af @ U[free] - b) / np.linalg.norm(b):.3e}")
    assert rel(U, Uref) <= 1e-10, (mesh, pc, rel(U, Uref))
    assert np.linalg.norm(Af @ U[free] - b) <= 1e-12 * np.linalg.norm(b)


# ---------------------------------------------------------------------------
# 4. the post: stress, failures, reaction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,dy", [(PLANAR, 0.012), (SIM3D, 0.012)])
def test_post_per_element(eng, mesh, dy):
    xyz, e2n, top, bot = mesh_of(mesh)
    n = len(e2n)
    A, I, strength = recipe(n)  # noqa: E741
    E = modulus(n)
    start(eng, mesh, props=dict(E=E, A=A, I=I))
    eng.assemble()
    assert eng.solve(dy, -dy, opts(GAMG)).status == 0
    U = eng.displacement()
    eps = fo.element_strain(xyz, e2n, U)
    a = np.abs(eps)
    top_e = int(np.nanargmax(a))  # the most strained element: made unbreakable
    tiny = int(np.nanargmin(np.where(a > 0, a, np.inf)))  # the least strained loaded one: made to fail
    strength = strength.copy()
    strength[top_e] = np.inf
    strength[tiny] = a[tiny] * 0.5
    eng.set_element_props(E=E, A=A, I=I, max_strain=strength)
    eng.assemble()  # (the change dropped K; the same bits)
    act0 = eng.active()
    assert act0.all()
    f, na = eng.post(MAX_STRAIN)
    with np.errstate(invalid="ignore"):
        fails = act0 & (a > strength)
    assert same_bits(eng.stress(), np.where(act0, E * eps, 0.0))
    act1 = eng.active()
    assert np.array_equal(act1, act0 & ~fails) and na == int(act1.sum())
    assert act1[top_e] and not act1[tiny] and fails.sum() >= 1
    # the scalar has no effect once the array is set
    for scalar in (1e-9, np.inf):
        eng.set_active(None)
        f2, na2 = eng.post(scalar)
        assert same_bits(f2, f) and na2 == na and np.array_equal(eng.active(), act1)
    # reaction: Σ_top (K·U)_y of the checker's unregularised K
    K = het_K(xyz, e2n, np.ones(n, bool), E, A, I)
    fr = (K @ U)[[3 * t + 1 for t in top]].sum()
    assert force_close([f], [fr]), (f, fr)
    # in a step: the weak element goes in the first loaded one, the unbreakable one stays
    eng.set_active(None)
    _, na3, st = eng.step(dy, -dy, opts(GAMG), MAX_STRAIN)
    assert st.status == 0 and na3 == na and not eng.active()[tiny] and eng.active()[top_e]


# ---------------------------------------------------------------------------
# 5. runs and invalidation
# ---------------------------------------------------------------------------
def _props(n, strength=True):
    A, I, s = recipe(n)  # noqa: E741
    return dict(A=A, I=I, max_strain=s) if strength else dict(A=A, I=I)


@pytest.mark.parametrize("pc", [JACOBI, GAMG])
def test_run_equals_step_loop(eng, pc):
    n = len(mesh_of(PLANAR)[1])
    dys = np.array([0.003 * k for k in range(1, 7)])
    loop = _ramp(eng, PLANAR, pc, _props(n), dys)
    assert loop[-1][1] < n
    start(eng, PLANAR, props=_props(n))
    run = eng.run(dys, -dys, opts(pc, 1e-12), MAX_STRAIN)
    assert run["n_done"] == len(dys)
    for k, row in enumerate(loop):
        assert same_bits(run["force"][k], row[0]) and run["n_active"][k] == row[1]
        assert run["stats"][k]["iters"] == row[2]
        assert same_bits(run["U"][k], row[4]) and same_bits(run["stress"][k], row[5])
        assert np.array_equal(run["active"][k], row[6])


def _step_rec(e, d, pc):
    f, n, st = e.step(d, -d, opts(pc, 1e-12), 1.0)  # (nothing fails at max_strain 1: the active set holds)
    assert st.status == 0
    return f, n, st.iters, e.export_csr()[2], e.displacement(), e.stress(), st.amg_rebuilt


@pytest.mark.parametrize("graphs", [GRAPHS_ON, GRAPHS_OFF], ids=["graphs_on", "graphs_off"])
@pytest.mark.parametrize("pc", [JACOBI, GAMG])
def test_props_change_between_steps(eng, pc, graphs):
    """A change of the properties on an unchanged active set drops the kept K,
    the kept hierarchy values and every captured graph that holds the old
    pointers or the old kernel choice: the next step equals a fresh handle's
    given the new properties, bit for bit — arrays → other arrays, uniform →
    arrays, arrays → uniform (NULL).  The symbolic hierarchy is kept."""
    from mfea import Engine
    n = len(mesh_of(PLANAR)[1])
    A, I, _ = recipe(n)  # noqa: E741
    E = modulus(n)
    configs = {"uniform": None, "a": dict(A=A, I=I), "b": dict(A=A[::-1].copy(), I=I[::-1].copy(), E=E),
               "e": dict(E=E)}
    seq = ["uniform", "a", "b", "uniform", "e", "a", "a"]
    d = 0.002
    with eng.options(**graphs):
        start(eng, PLANAR)
        got = []
        for name in seq:
            eng.set_element_props(**(configs[name] or {}))
            # two steps on each: the second replays what the first captured / kept
            got.append([_step_rec(eng, d, pc), _step_rec(eng, 2 * d, pc)])
    assert eng.get_option("op_kept_steps") > 0
    for k, g in enumerate(got):
        if k:  # the hierarchy's plan survived the change
            assert g[0][6] == 0 and g[1][6] == 0, k
    fresh = {}
    for name, p in configs.items():
        with Engine(0) as f:
            f.set_option("amg_rebuild_rent", 0)
            with f.options(**graphs):
                start(f, PLANAR, props=p)
                fresh[name] = [_step_rec(f, d, pc), _step_rec(f, 2 * d, pc)]
    for k, name in enumerate(seq):
        for s in range(2):
            a, b = got[k][s], fresh[name][s]
            assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (k, s, a[:3], b[:3])
            for i in (3, 4, 5):
                assert same_bits(a[i], b[i]), (k, s, i)


# ---------------------------------------------------------------------------
# 6. events with a strength array
# ---------------------------------------------------------------------------
def rule_pe(eps, act0, E, strength, tie_rtol, lam_max):
    """The per-element event rule of include/mfea.h in NumPy f64:
    (lam, lam_e, failing group, stress row)."""
    a = np.abs(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = act0 & (a > 0.0)
        lam_e = np.where(m, strength / a, np.inf)
    lam = np.float64(lam_e[m].min()) if m.any() else np.float64(np.inf)
    breaks = bool(np.isfinite(lam) and lam <= lam_max)
    thr = lam / (np.float64(1.0) - np.float64(tie_rtol))
    group = (m & (lam_e <= thr)) if breaks else np.zeros_like(act0)
    factor = lam if breaks else (np.float64(lam_max) if np.isfinite(lam_max) else np.float64(1.0))
    with np.errstate(invalid="ignore"):
        stress = np.where(act0, (E * eps) * factor, 0.0)
    return lam, lam_e, group, stress


# mesh: (dref, lam_max, events with failures, stop)
EVENTS = {X: (0.06, np.inf, 7, "unloaded"), PLANAR: (0.02, 1.0, 7, "lam_max"), SIM3D: (0.02, 1.0, 3, "lam_max")}
TIE = 1e-6
# After its seven breaks test_X is a rigid piece hanging on one grip: it carries
# no load, but its strains are the solve's rounding noise (≈ 1e-9 of the real
# ones) instead of exact zeros — the direct-solve oracle then sees lam ≈ 1.8e6
# where an exact solve gives +inf.  A load factor beyond NOISE (three decades
# above every real one here, three below the noise) counts as unloaded.
NOISE = 1e3
_oracle = {}


def oracle_sequence(mesh):
    """Direct solves with the rule above at tie_rtol 1e-6: the n_fail breaking
    events, how the run ends after them, and the smallest relative gap between
    the breaking element's lam_e and the runner-up's over those events (the
    test asserts > 1e-4: a device solve at rtol 1e-13 must break the same
    element)."""
    if mesh in _oracle:
        return _oracle[mesh]
    xyz, e2n, top, bot = mesh_of(mesh)
    dref, lam_max, n_fail, _ = EVENTS[mesh]
    n = len(e2n)
    A, I, strength = recipe(n)  # noqa: E741
    act = np.ones(n, bool)
    known, vals = fo.known_dof_map(top, bot, dref, -dref)
    seq, stop, gap = [], "breaks", np.inf
    for k in range(n_fail + 1):
        K = het_K(xyz, e2n, act, fo.E_MOD, A, I)
        U = fo.solve_system(K, known, vals)
        f1 = (K @ U)[[3 * t + 1 for t in top]].sum()
        eps = fo.element_strain(xyz, e2n, U)
        lam, lam_e, group, _ = rule_pe(eps, act, fo.E_MOD, strength, TIE, lam_max)
        if lam > lam_max:
            stop = "lam_max"
            break
        if lam > NOISE:
            stop = "unloaded"
            break
        if k == n_fail:
            break
        rest = lam_e[act & ~group]
        if rest.size and rest.min() <= NOISE:
            gap = min(gap, (rest.min() - lam) / lam)
        seq.append((lam, lam * f1, group))
        act = act & ~group
    _oracle[mesh] = (seq, stop, gap)
    return _oracle[mesh]


@pytest.mark.parametrize("pc", [JACOBI, GAMG])
@pytest.mark.parametrize("mesh", list(EVENTS))
def test_events_with_strengths(eng, mesh, pc):
    """The recipe's sequences at tie_rtol 1e-6 (direct-solve oracle; lam at the
    reference load ∓dref): test_X 7 single-element events, lam 0.27855 …
    0.44679, smallest gap to the runner-up 0.82 %; the planar mesh 7, lam
    0.21926 … 0.40684, then lam 4657.5 > lam_max; the 3-D mesh 3, lam 0.12176 …
    0.17986, then 12005.9 > lam_max.  After test_X's seventh break the rest is a
    rigid piece on one grip: the oracle's and the device's event 7 have lam
    1.7539e6 (rounding-noise strains, NOISE above), not +inf."""
    from mfea import EVENTS_COMPLETE, EVENTS_LAMBDA_MAX, EVENTS_UNLOADED
    xyz, e2n, top, bot = mesh_of(mesh)
    dref, lam_max, n_fail, stop = EVENTS[mesh]
    n = len(e2n)
    A, I, strength = recipe(n)  # noqa: E741
    props = dict(A=A, I=I, max_strain=strength)
    seq, ostop, gap = oracle_sequence(mesh)
    print(f"{mesh}: oracle events {len(seq)}, stop {ostop}, first lam {seq[0][0]:.6f}, smallest gap {gap:.3e}")
    assert gap > 1e-4
    assert len(seq) == n_fail and ostop == stop
    assert all(int(g.sum()) == 1 for _, _, g in seq)
    if mesh == PLANAR:
        # 0.4385 at the reference load ∓0.01 (a travel of 0.02); lam scales with
        # the inverse of the reference load, here ∓0.02 as in tests/test_gpu_events.py
        assert abs(2.0 * seq[0][0] - 0.4385) < 1e-4
    # the caller's loop, bit for bit from the device's own U₁
    start(eng, mesh, props=props)
    loop = {k: [] for k in ("lam", "force1", "stress", "active", "U1")}
    fails = []
    for k in range(n_fail + 1):
        act0 = eng.active()
        lam, f1, nf, na, st = eng.event(dref, -dref, opts(pc), 123.0, TIE, lam_max)  # (the scalar is unused)
        U1, stress, act1 = eng.displacement(), eng.stress(), eng.active()
        eps = fo.element_strain(xyz, e2n, U1)
        lam_np, _, group, stress_np = rule_pe(eps, act0, fo.E_MOD, strength, TIE, lam_max)
        assert same_bits(lam, lam_np), (k, lam, lam_np)
        assert np.array_equal(act1, act0 & ~group), k
        assert nf == int(group.sum()) and na == int(act1.sum()), k
        assert same_bits(stress, stress_np), k
        for key, v in zip(loop, (lam, f1, stress, act1, U1)):
            loop[key].append(v)
        fails.append(nf)
    # the oracle's sequence of element ids
    prev = np.ones(n, bool)
    for k, (lam, force, group) in enumerate(seq):
        assert np.array_equal(prev & ~loop["active"][k], group), k
        prev = loop["active"][k]
        assert abs(loop["lam"][k] - lam) <= 1e-6 * abs(lam), (k, loop["lam"][k], lam)
        got = loop["lam"][k] * loop["force1"][k]
        assert abs(got - force) <= 1e-6 * abs(force), (k, got, force)
    # ... and its end
    print(f"{mesh} pc {pc}: event {n_fail} lam {loop['lam'][-1]!r}, failed {fails[-1]}")
    if stop == "lam_max":
        assert fails[-1] == 0 and loop["lam"][-1] > lam_max
    else:
        assert loop["lam"][-1] > NOISE
    # run_events equals the loop
    start(eng, mesh, props=props)
    run = eng.run_events(dref, -dref, opts(pc), 123.0, TIE, lam_max, n_events=n_fail + 1)
    assert run["n_done"] == n_fail + 1
    if stop == "lam_max":
        assert run["stop_reason"] == EVENTS_LAMBDA_MAX
    else:
        assert run["stop_reason"] == (EVENTS_UNLOADED if np.isinf(run["lam"][-1]) else EVENTS_COMPLETE)
    for key in ("lam", "force1", "stress"):
        assert same_bits(run[key], np.asarray(loop[key])), key
    assert np.array_equal(run["active"], np.asarray(loop["active"]))
    with np.errstate(invalid="ignore"):
        assert same_bits(run["U"], np.asarray(loop["lam"])[:, None] * np.asarray(loop["U1"]))


def test_events_modulus_only(eng):
    """No strength array: the smax rule runs unchanged, E_e in the stress row."""
    xyz, e2n, _, _ = mesh_of(X)
    n = len(e2n)
    E = modulus(n)
    start(eng, X)
    plain = eng.run_events(0.06, -0.06, opts(GAMG), MAX_STRAIN, 1e-9, np.inf, n_events=3)
    start(eng, X, props=dict(E=np.full(n, fo.E_MOD)))
    same = eng.run_events(0.06, -0.06, opts(GAMG), MAX_STRAIN, 1e-9, np.inf, n_events=3)
    for key in ("lam", "force1", "stress", "U"):
        assert same_bits(same[key], plain[key]), key
    start(eng, X, props=dict(E=E))
    lam, f1, nf, na, _ = eng.event(0.06, -0.06, opts(GAMG), MAX_STRAIN, 1e-9, np.inf)
    eps = fo.element_strain(xyz, e2n, eng.displacement())
    smax = np.abs(eps).max()
    assert same_bits(lam, np.float64(MAX_STRAIN) / smax) and nf > 0
    assert same_bits(eng.stress(), (E * eps) * lam)


# ---------------------------------------------------------------------------
# 7. lifecycle
# ---------------------------------------------------------------------------
def _K(e):
    e.assemble()
    return e.export_csr()[2]


def test_lifecycle():
    from mfea import Engine, MfeaError
    from mfea._capi import EINVAL, ESTATE
    xyz, e2n, top, bot = mesh_of(X)
    n = len(e2n)
    A, I, s = recipe(n)  # noqa: E741
    with Engine(0) as e:
        with pytest.raises(MfeaError) as err:  # before a mesh
            e.set_element_props()
        assert err.value.code == ESTATE
        e.set_mesh(xyz, e2n)
        assert e.get_option("element_props") == 0
        p = e.element_props()  # nothing set: the scalars, NaN for the strength
        assert np.all(p["E"] == fo.E_MOD) and np.all(p["A"] == fo.AREA) and np.all(p["I"] == fo.INERTIA)
        assert np.isnan(p["max_strain"]).all()
        e.set_element_props(A=A, max_strain=s)
        p = e.element_props()  # the getter round-trips; columns not set: the scalar
        assert same_bits(p["A"], A) and same_bits(p["max_strain"], s)
        assert np.all(p["E"] == fo.E_MOD) and np.all(p["I"] == fo.INERTIA)
        # a later set_material changes only the columns given as NULL
        e.set_material(1234.0, 5.0, 6.0)
        p = e.element_props()
        assert same_bits(p["A"], A) and np.all(p["E"] == 1234.0) and np.all(p["I"] == 6.0)
        e.set_material(fo.E_MOD, fo.AREA, fo.INERTIA)
        # every EINVAL case leaves the previous properties in force
        bad = []
        for col in ("E", "A", "I"):
            for v in (-1.0, np.nan, np.inf):
                a = np.full(n, 1.0)
                a[n // 2] = v
                bad.append({col: a})
        for v in (0.0, -0.5, np.nan):
            a = np.full(n, 0.01)
            a[-1] = v
            bad.append({"max_strain": a})
        for b in bad:
            with pytest.raises(MfeaError) as err:
                e.set_element_props(**b)
            assert err.value.code == EINVAL, b
            p = e.element_props()
            assert same_bits(p["A"], A) and same_bits(p["max_strain"], s) and np.all(p["E"] == fo.E_MOD)
        ok = s.copy()
        ok[0] = np.inf  # +inf is a strength
        e.set_element_props(A=A, max_strain=ok)
        assert np.isinf(e.element_props()["max_strain"][0])
        # wrong length / dtype: refused by the Engine before the library sees it
        with pytest.raises(ValueError):
            e.set_element_props(A=A[:-1])
        with pytest.raises(ValueError):
            e.set_element_props(A=A.astype(np.float32))
        # set_bc and set_active keep the properties, set_mesh clears them
        e.set_bc(top, bot)
        e.set_active(None)
        assert e.get_option("element_props") == 1 and same_bits(e.element_props()["A"], A)
        K1 = _K(e)
        e.set_mesh(xyz, e2n)
        assert e.get_option("element_props") == 0 and np.all(e.element_props()["A"] == fo.AREA)
        e.set_bc(top, bot)
        e.set_active(None)
        K0 = _K(e)
        assert not np.array_equal(K0, K1)
        # all NULL: back to uniform
        e.set_element_props(A=A)
        e.set_element_props()
        assert e.get_option("element_props") == 0
        assert np.array_equal(_K(e), K0)
    # one partition only, in either order
    with Engine(0) as e:
        e.set_parts(2)
        e.set_mesh(xyz, e2n)
        with pytest.raises(MfeaError) as err:
            e.set_element_props(A=A)
        assert err.value.code == ESTATE
    with Engine(0) as e:
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_element_props(A=A)
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.assemble()
        assert err.value.code == ESTATE


# ---------------------------------------------------------------------------
# 8. the drop-in
# ---------------------------------------------------------------------------
def _props_file(path, n, cols):
    import pandas as pd
    order = np.random.default_rng(3).permutation(n)  # any order of ids
    pd.DataFrame({"elem_id": order, **{k: v[order] for k, v in cols.items()}}).to_csv(path, index=False)


def test_dropin_element_props(tmp_path, eng):
    import fea_solver as fs
    xyz, e2n, top, bot = mesh_of(X)
    n = len(e2n)
    A, I, s = recipe(n)  # noqa: E741
    d = tmp_path / X
    shutil.copytree(os.path.join(GOLDEN, "meshes", X), d)
    f = tmp_path / "props.csv"
    _props_file(f, n, {"max_strain": s, "A": A, "I": I})
    saved = (fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG)
    try:
        with fs.get_engine().options(amg_rebuild_rent=0):
            fs.main([str(d), "--element-props", str(f), "--grip-length", "0.5", "--disp-max", "0.06",
                     "--n-steps", "12"])
            ramp = {k: read_rt(d / "fea_results" / k) for k in
                    ("force_displacement.csv", "stress_record.csv", "active_elements.csv", "node_displacements.csv")}
            fs.main([str(d), "--element-props", str(f), "--grip-length", "0.5", "--disp-max", "0.06", "--events"])
        out = d / "fea_results"
        # the ramp against the Engine's
        dys = np.array([0.06 * (k / 11) for k in range(12)])
        start(eng, X, props=dict(A=A, I=I, max_strain=s))
        run = eng.run(dys, -dys, fs._opts(), MAX_STRAIN)
        m = run["n_done"]
        assert m == len(ramp["force_displacement.csv"]) and run["n_active"][-1] < n
        assert same_bits(ramp["force_displacement.csv"]["total_force"].values, run["force"])
        assert same_bits(ramp["stress_record.csv"].values[:, :-1], run["stress"])
        assert same_bits(ramp["node_displacements.csv"].values[:, :-1], run["U"])
        assert np.array_equal(ramp["active_elements.csv"].values[:, :-1].astype(bool), run["active"])
        # the events against the Engine's
        start(eng, X, props=dict(A=A, I=I, max_strain=s))
        ev = eng.run_events(0.06, -0.06, fs._opts(), MAX_STRAIN, 1e-9, 1.0)
        m = ev["n_done"]
        lines = (out / "failure_events.csv").read_text().splitlines()
        assert len(lines) == 1 + m and m >= 2
        for k, ln in enumerate(lines[1:]):
            _, lam, disp, force, nf, na = ln.split(",")
            assert int(nf) == ev["n_failed"][k] and int(na) == ev["n_active"][k]
            assert same_bits(float(lam), ev["lam"][k])
            assert same_bits(float(force), ev["lam"][k] * ev["force1"][k])
        assert same_bits(read_rt(out / "stress_record.csv").values[:, :-1], ev["stress"])
    finally:
        fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG = saved
