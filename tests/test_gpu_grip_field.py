"""Grip displacement fields (mfea_set_grip_field): a prescribed vector per grip
node on every entry point.

The checker is the oracle's assembly and direct solve with
known_vals[3n + c] = np.float64(a_n) * d[n, c], filled top then bottom as
fo.known_dof_map fills it.  The fields: R, a rigid rotation of the top band
about z through its centroid, the bottom band held (zero rows); A, an affine
displacement with a fixed non-symmetric H on both bands; Q (the 3-D mesh), a
rotation about (0.48, 0.6, 0.64).  No node is in both bands on the three
meshes.  The uniform identity is bit equality with a handle that only called
set_grip_motion."""
import os

import numpy as np
import pytest

from test_gpu_grip_motion import (AMP, EX, EY, GAMG, GRIP, ICC, JACOBI, BJACOBI, MAX_STRAIN, MIX2, PLANAR, SIM3D,
                                  SOR, U_ROUND, X, K_of, mesh_of, opts, reaction_ref, rel, work_force)
from test_gpu_events import rule
from test_gpu_props import GRAPHS_OFF, GRAPHS_ON, het_K, recipe, same_bits

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

H_AFF = np.array([[0.2, 0.7, -0.3], [-0.4, 1.0, 0.5], [0.3, -0.2, 0.6]])
Q_AXIS = (0.48, 0.6, 0.64)


@pytest.fixture(scope="module")
def eng():
    from mfea import Engine
    e = Engine(0)
    e.set_option("amg_rebuild_rent", 0)
    yield e
    e.close()


_fields, _ref = {}, {}


def field_of(name, tag):
    """The named field on the named mesh, once."""
    from mfea import fields
    if (name, tag) not in _fields:
        xyz, _, top, bot = mesh_of(name)
        assert not set(map(int, top)) & set(map(int, bot))
        if tag == "R":
            f = fields.rigid_rotation(xyz, top, (0.0, 0.0, 1.0))
        elif tag == "Q":
            f = fields.rigid_rotation(xyz, top, Q_AXIS)
        elif tag == "A":
            f = fields.affine(xyz, np.concatenate([top, bot]), H_AFF)
        elif tag == "U":  # the band vectors of the uniform identity
            f = fields.uniform(len(xyz), top, MIX2) + fields.uniform(len(xyz), bot, EY)
        elif tag == "Z":  # R with an out-of-plane tilt of the top band
            f = fields.rigid_rotation(xyz, top, (0.0, 0.0, 1.0)) + fields.rigid_rotation(xyz, top, (1.0, 0.0, 0.0))
        _fields[name, tag] = f
    return _fields[name, tag]


def known_map(top, bot, a_top, a_bot, d):
    m = {}
    for n in top:
        m.update({3 * n + c: np.float64(a_top) * d[n, c] for c in range(3)})
    for n in bot:
        m.update({3 * n + c: np.float64(a_bot) * d[n, c] for c in range(3)})
    known = np.array(list(m.keys()), dtype=np.int64)
    return known, np.array([m[k] for k in known], dtype=np.float64)


def oracle(name, tag, a_top, a_bot, K=None, bands=None):
    """The direct solve, once per case (K or bands given: not cached)."""
    key = (name, tag, a_top, a_bot)
    if K is not None or bands is not None or key not in _ref:
        _, _, top, bot = mesh_of(name) if bands is None else (None, None) + tuple(bands)
        known, vals = known_map(top, bot, a_top, a_bot, field_of(name, tag))
        U = fo.solve_system(K_of(name) if K is None else K, known, vals)
        if K is not None or bands is not None:
            return U
        _ref[key] = U
    return _ref[key]


def start(e, name, tag=None, props=None, motion=(EY, EY)):
    xyz, e2n, top, bot = mesh_of(name)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot)
    e.set_active(None)
    e.set_grip_motion(*motion)
    if tag is not None:
        e.set_grip_field(field_of(name, tag))
    if props is not None:
        e.set_element_props(**props)
    return xyz, e2n, top, bot


def grip_rows_exact(U, top, bot, a_top, a_bot, d):
    U3 = U.reshape(-1, 3)
    return (np.array_equal(U3[top], np.float64(a_top) * d[top]) and
            np.array_equal(U3[bot], np.float64(a_bot) * d[bot]))


def work_ref(K, U, band, d):
    """Σ_n d_n·(K U)_n over the band in extended precision, and the dot-product
    bound γ_n · Σ |d||K||U| with n = the stored terms of the band's rows plus
    three per row (the row's product and sums) plus the row count."""
    ref, bound, terms = np.longdouble(0.0), 0.0, 0
    Ul, Ua = U.astype(np.longdouble), np.abs(U)
    for c in range(3):
        rows = np.array([3 * int(n) + c for n in band], dtype=np.int64)
        Kb = K[rows].tocsr()
        w = np.repeat(d[np.asarray(band, dtype=np.int64), c], np.diff(Kb.indptr))
        ref += np.sum(w.astype(np.longdouble) * Kb.data.astype(np.longdouble) * Ul[Kb.indices])
        bound += float(np.sum(np.abs(w) * np.abs(Kb.data) * Ua[Kb.indices]))
        terms += Kb.nnz + 2 * len(rows)
    gamma = terms * U_ROUND / (1.0 - terms * U_ROUND)
    return float(ref), gamma * bound


# ---------------------------------------------------------------------------
# 1. parity with the direct solve, through mfea_solve and through mfea_step
# ---------------------------------------------------------------------------
ALL_PC = (JACOBI, BJACOBI, GAMG, SOR, ICC)
PARITY = ([(m, f, pc) for m in (PLANAR, SIM3D) for f in ("R", "A") for pc in ALL_PC] +
          [(SIM3D, "Q", pc) for pc in ALL_PC] + [(X, f, pc) for f in ("R", "A") for pc in (GAMG, JACOBI)])


@pytest.mark.parametrize("mesh,tag,pc", PARITY)
def test_parity(eng, mesh, tag, pc):
    _, _, top, bot = start(eng, mesh, tag)
    d = field_of(mesh, tag)
    Uref = oracle(mesh, tag, AMP, -AMP)
    got, is_set = eng.grip_field()
    assert is_set and same_bits(got, d + 0.0)  # (-0 is stored as 0)
    # the separate RHS kernel: mfea_solve after mfea_assemble
    eng.assemble()
    st = eng.solve(AMP, -AMP, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    print(f"{mesh} {tag} pc {pc}: solve iters {st.iters} rel {rel(U, Uref):.3e}")
    assert rel(U, Uref) <= 1e-10, (mesh, tag, pc, rel(U, Uref))
    assert grip_rows_exact(U, top, bot, AMP, -AMP, d)
    # the fused RHS of the assembly, then (K and the hierarchy kept) k_amg_start
    for k in range(2):
        _, _, st = eng.step(AMP, -AMP, opts(pc), 1.0)
        assert st.status == 0
        U = eng.displacement()
        print(f"  step {k}: iters {st.iters} rel {rel(U, Uref):.3e}")
        assert rel(U, Uref) <= 1e-10, (mesh, tag, pc, k, rel(U, Uref))
        assert grip_rows_exact(U, top, bot, AMP, -AMP, d)


# ---------------------------------------------------------------------------
# 2. the uniform identity: the rows equal to the band vectors
# ---------------------------------------------------------------------------
def _step_and_event(e, name, tag, pc, props):
    d = 0.012
    start(e, name, tag, props=props, motion=(MIX2, EY))
    f, n, st = e.step(d, -d, opts(pc, 1e-12), MAX_STRAIN)
    step = (f, n, st.iters, e.displacement(), e.stress(), e.active())
    start(e, name, tag, props=props, motion=(MIX2, EY))
    lam, f1, nf, na, st = e.event(0.02, -0.02, opts(pc, 1e-12), MAX_STRAIN, 1e-9, np.inf)
    return step, (lam, f1, nf, na, st.iters, e.displacement(), e.stress(), e.active())


@pytest.mark.parametrize("with_props", [False, True], ids=["uniform", "props"])
@pytest.mark.parametrize("pc,graphs", [(GAMG, GRAPHS_ON), (GAMG, GRAPHS_OFF), (JACOBI, {}), (ICC, {})],
                         ids=["gamg_on", "gamg_off", "jacobi", "icc"])
def test_uniform_identity(eng, pc, graphs, with_props):
    xyz, e2n, top, bot = mesh_of(PLANAR)
    n = len(e2n)
    props, K = None, K_of(PLANAR)
    if with_props:
        A, I, strength = recipe(n)  # noqa: E741
        props = dict(A=A, I=I, max_strain=strength)
        K = het_K(xyz, e2n, np.ones(n, bool), fo.E_MOD, A, I).tocsr()
    with eng.options(**graphs):
        vec_step, vec_event = _step_and_event(eng, PLANAR, None, pc, props)
        assert not eng.grip_field()[1]
        fld_step, fld_event = _step_and_event(eng, PLANAR, "U", pc, props)
        assert eng.grip_field()[1]
    assert vec_step[1] < n and vec_event[2] > 0  # elements failed in both
    # U, iterations, stress, activity, n_active: bit for bit
    assert fld_step[1] == vec_step[1] and fld_step[2] == vec_step[2]
    assert same_bits(fld_step[3], vec_step[3]) and same_bits(fld_step[4], vec_step[4])
    assert np.array_equal(fld_step[5], vec_step[5])
    # the force: Σ d·f against d·Σ f, both within the weighted sum's bound of the checker
    ref, bound = work_ref(K, vec_step[3], top, field_of(PLANAR, "U"))
    print(f"force field {fld_step[0]!r} vectors {vec_step[0]!r} ref {ref!r} bound {bound:.3e}")
    assert abs(fld_step[0] - ref) <= bound and abs(vec_step[0] - ref) <= bound
    # one event: lam, n_failed, n_active, iterations, U₁, stress and activity
    assert same_bits(fld_event[0], vec_event[0]) and fld_event[2:5] == vec_event[2:5]
    assert same_bits(fld_event[5], vec_event[5]) and same_bits(fld_event[6], vec_event[6])
    assert np.array_equal(fld_event[7], vec_event[7])


# ---------------------------------------------------------------------------
# 3. the generalised force of both bands, and the work identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,tag", [(PLANAR, "R"), (PLANAR, "A"), (SIM3D, "Q"), (SIM3D, "A"), (X, "A")])
def test_grip_work(eng, mesh, tag):
    _, _, top, bot = start(eng, mesh, tag)
    K, d = K_of(mesh), field_of(mesh, tag)
    f, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    U = eng.displacement()
    g_top, g_bot = eng.grip_work()
    for got, band in ((g_top, top), (g_bot, bot)):
        ref, bound = work_ref(K, U, band, d)
        print(f"{mesh} {tag}: got {got!r} ref {ref!r} err {abs(got - ref):.3e} bound {bound:.3e}")
        assert abs(got - ref) <= bound
    assert same_bits(f, g_top)  # the step's force is the top band's value
    assert same_bits(eng.post(np.inf)[0], g_top)
    from mfea._capi import _lib, _ptr
    one = np.empty(1)
    assert _lib.mfea_get_grip_work(eng._h, _ptr(one), None) == 0 and same_bits(one[0], g_top)
    assert _lib.mfea_get_grip_work(eng._h, None, _ptr(one)) == 0 and same_bits(one[0], g_bot)
    assert _lib.mfea_get_grip_work(eng._h, None, None) == 0
    # mfea_get_reaction is unchanged: plain component sums
    top3, _ = eng.reaction()
    ref3, bound3 = reaction_ref(K, U, top)
    assert np.all(np.abs(top3 - ref3) <= bound3)


def test_grip_work_without_a_field(eng):
    start(eng, PLANAR, None, motion=(EX, MIX2))
    f, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    g_top, g_bot = eng.grip_work()
    top3, bot3 = eng.reaction()
    assert same_bits(g_top, f) and same_bits(g_top, work_force(EX, top3))
    assert same_bits(g_bot, work_force(MIX2, bot3))


@pytest.mark.parametrize("mesh,tag", [(SIM3D, "Q"), (SIM3D, "A"), (PLANAR, "R")])
def test_work_identity(eng, mesh, tag):
    """2W = dy_top·G_top + dy_bot·G_bot + u_fᵀ(KU)_f: test_gpu_energy.py's
    construction and bar, with the generalised forces."""
    xyz, e2n, top, bot = mesh_of(mesh)
    n = len(e2n)
    A, I, _ = recipe(n)  # noqa: E741
    start(eng, mesh, tag, props=dict(A=A, I=I))
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    en = eng.energy(elements=False)
    W2 = 2.0 * (en["axial"] + en["bending"])
    g_top, g_bot = eng.grip_work()
    gap = W2 - (AMP * g_top + (-AMP) * g_bot)
    K = het_K(xyz, e2n, np.ones(n, bool), fo.E_MOD, A, I).tocsr()
    U = eng.displacement()
    known, _ = known_map(top, bot, AMP, -AMP, field_of(mesh, tag))
    free = np.setdiff1d(np.arange(len(U)), known)
    resid = float(U[free] @ (K @ U)[free])
    scale = float(np.abs(U) @ (abs(K) @ np.abs(U)))
    print(f"{mesh} {tag}: 2W {W2:.6e}, gap/2W {gap / W2:.2e}, |gap - resid| {abs(gap - resid):.2e} "
          f"against 1e-12 * |U||K||U| = {1e-12 * scale:.2e}")
    assert W2 > 0.0
    assert abs(gap - resid) <= 1e-12 * scale


# ---------------------------------------------------------------------------
# 4. a change between steps: nothing stale, everything kept
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("phase_times", [0, 1])
@pytest.mark.parametrize("order", ["y_R_y", "R_y_R"])
def test_change_between_steps(eng, order, phase_times):
    from mfea import Engine
    from test_gpu_grip_motion import oracle as vec_oracle
    d = 0.01
    seq = ["R" if c == "R" else None for c in order.split("_")]
    want = {None: vec_oracle(PLANAR, d, -d, EY, EY), "R": oracle(PLANAR, "R", d, -d)}
    with eng.options(**GRAPHS_ON, phase_times=phase_times):
        start(eng, PLANAR, seq[0])
        for _ in range(2):  # (the second replays what the first captured / kept)
            f_prev, _, st = eng.step(d, -d, opts(GAMG), 1.0)
            assert st.status == 0
        assert rel(eng.displacement(), want[seq[0]]) <= 1e-10
        for tag in seq[1:]:
            kept = eng.get_option("op_kept_steps"), eng.get_option("amg_setup_kept")
            eng.set_grip_field(None if tag is None else field_of(PLANAR, tag))
            for k in range(2):
                f, _, st = eng.step(d, -d, opts(GAMG), 1.0)
                assert st.status == 0 and st.amg_rebuilt == 0
                U = eng.displacement()
                assert rel(U, want[tag]) <= 1e-10, (tag, k, rel(U, want[tag]))
                # a kept step: no assembly, no numeric setup
                assert eng.get_option("op_kept_steps") == kept[0] + k + 1
                assert eng.get_option("amg_setup_kept") == kept[1] + k + 1
                if phase_times:
                    assert st.t_setup_ms == 0
                assert same_bits(f, eng.grip_work()[0])
            assert f != f_prev
            f_prev = f
            # the same bytes again drop nothing: still a kept step
            eng.set_grip_field(None if tag is None else field_of(PLANAR, tag).copy())
        if seq[-1] is None:  # the last tensile step: the bits of a fresh handle
            with Engine(0) as fresh:
                fresh.set_option("amg_rebuild_rent", 0)
                with fresh.options(**GRAPHS_ON, phase_times=phase_times):
                    start(fresh, PLANAR)
                    for _ in range(2):
                        f0, _, st0 = fresh.step(d, -d, opts(GAMG), 1.0)
                    assert st0.status == 0 and st0.iters == st.iters
                    assert same_bits(eng.displacement(), fresh.displacement()) and same_bits(f, f0)


# ---------------------------------------------------------------------------
# 5. z entries on a planar mesh: 3 DOFs per node, and back
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_planar_z(eng, pc):
    from mfea import Engine
    _, _, top, bot = start(eng, PLANAR, "R")
    assert eng.info()["planar"] == 1
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2  # every z entry zero: the 2-DOF lanes
    eng.set_grip_field(field_of(PLANAR, "Z"))
    eng.assemble()
    st = eng.solve(AMP, -AMP, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    Uref = oracle(PLANAR, "Z", AMP, -AMP)
    print(f"planar z pc {pc}: iters {st.iters} rel {rel(U, Uref):.3e}")
    assert rel(U, Uref) <= 1e-10
    assert grip_rows_exact(U, top, bot, AMP, -AMP, field_of(PLANAR, "Z"))
    assert np.any(U.reshape(-1, 3)[:, 2] != 0.0)
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 3
    # cleared: the 2-DOF path, the bits of a fresh handle
    eng.set_grip_field(None)
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2
    U2 = eng.displacement()
    with Engine(0) as f:
        f.set_option("amg_rebuild_rent", 0)
        start(f, PLANAR)
        f.assemble()
        assert f.solve(AMP, -AMP, opts(pc)).status == 0
        assert same_bits(U2, f.displacement())
    assert not np.any(U2.reshape(-1, 3)[:, 2])


# ---------------------------------------------------------------------------
# 6. runs and events under a rotation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_run_equals_step_loop(eng, pc):
    dys = np.array([0.01, 0.02, 0.03, 0.04])
    n = len(mesh_of(PLANAR)[1])
    start(eng, PLANAR, "R")
    loop = []
    for d in dys:
        f, na, st = eng.step(d, -d, opts(pc, 1e-12), MAX_STRAIN)
        assert st.status == 0
        loop.append((f, na, st.iters, eng.displacement(), eng.stress(), eng.active()))
    assert loop[-1][1] < n  # at least one step fails an element
    start(eng, PLANAR, "R")
    run = eng.run(dys, -dys, opts(pc, 1e-12), MAX_STRAIN)
    assert run["n_done"] == len(dys)
    for k, row in enumerate(loop):
        assert same_bits(run["force"][k], row[0]) and run["n_active"][k] == row[1], k
        assert run["stats"][k]["iters"] == row[2], k
        assert same_bits(run["U"][k], row[3]) and same_bits(run["stress"][k], row[4]), k
        assert np.array_equal(run["active"][k], row[5]), k


@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_events(eng, pc):
    from mfea import EVENTS_COMPLETE
    dref, tie, lam_max, n_events = 0.02, 1e-9, np.inf, 3
    xyz, e2n, top, _ = mesh_of(PLANAR)
    # the failure strain from the direct solve: the first break near lam = 0.5
    eps0 = np.abs(fo.element_strain(xyz, e2n, oracle(PLANAR, "R", dref, -dref)))
    max_strain = 0.5 * float(np.nanmax(eps0))
    start(eng, PLANAR, "R")
    rec = {k: [] for k in ("lam", "force1", "U1", "stress", "active", "n_failed")}
    for k in range(n_events):
        act0 = eng.active()
        lam, f1, nf, na, st = eng.event(dref, -dref, opts(pc), max_strain, tie, lam_max)
        assert st.status == 0
        U1, stress, act1 = eng.displacement(), eng.stress(), eng.active()
        eps = fo.element_strain(xyz, e2n, U1)
        _, lam_np, group, stress_np = rule(eps, act0, max_strain, tie, lam_max)
        assert same_bits(lam, lam_np), (k, lam, lam_np)
        assert nf == int(group.sum()) > 0 and na == int(act1.sum()), k
        assert np.array_equal(act1, act0 & ~group), k
        assert same_bits(stress, stress_np), k
        # F₁: the generalised force of the event's own K and U₁
        assert same_bits(f1, eng.grip_work()[0]), k
        assert same_bits(f1, eng.post(np.inf)[0]), k
        for key, v in zip(rec, (lam, f1, U1, stress, act1, nf)):
            rec[key].append(v)
    assert 0.4 < rec["lam"][0] < 0.6
    start(eng, PLANAR, "R")
    run = eng.run_events(dref, -dref, opts(pc), max_strain, tie, lam_max, n_events=n_events)
    assert run["n_done"] == n_events and run["stop_reason"] == EVENTS_COMPLETE
    assert same_bits(run["lam"], rec["lam"]) and same_bits(run["force1"], rec["force1"])
    assert same_bits(run["stress"], rec["stress"]) and np.array_equal(run["active"], rec["active"])
    assert same_bits(run["U"], np.asarray(rec["lam"])[:, None] * np.asarray(rec["U1"]))
    assert np.array_equal(run["n_failed"], rec["n_failed"])


# ---------------------------------------------------------------------------
# 7. lifetime and errors
# ---------------------------------------------------------------------------
def test_lifetime(eng):
    xyz, e2n, top, bot = start(eng, SIM3D, "A")
    d = field_of(SIM3D, "A")
    # other bands: the stored field is gathered again for the new rows
    top2, bot2 = fo.grip_nodes(xyz, np.arange(len(xyz)), 1.4 * GRIP[SIM3D])
    assert len(top2) > len(top) and len(bot2) > len(bot) and not set(top2) & set(bot2)
    full = H_AFF @ xyz.T  # (a field on every node: the new bands' rows are there)
    eng.set_grip_field(full.T.copy())
    _fields[SIM3D, "full"] = full.T.copy()
    eng.set_bc(top2, bot2)
    eng.set_active(None)
    assert eng.grip_field()[1]
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    Uref = oracle(SIM3D, "full", AMP, -AMP, bands=(top2, bot2))
    assert rel(eng.displacement(), Uref) <= 1e-10
    # the other setters keep it
    eng.set_bc(top, bot)
    eng.set_grip_field(d)
    eng.set_active(np.ones(len(e2n), dtype=np.uint8))
    eng.set_material(fo.E_MOD, fo.AREA, fo.INERTIA)
    eng.set_element_props(A=np.full(len(e2n), fo.AREA))
    eng.set_element_props()
    eng.set_grip_motion(EX, MIX2)
    got, is_set = eng.grip_field()
    assert is_set and same_bits(got, d + 0.0)  # (-0 is stored as 0)
    t, b = eng.grip_motion()  # the vectors are kept next to it, and read nowhere
    assert t.tolist() == list(EX) and b.tolist() == list(MIX2)
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    assert rel(eng.displacement(), oracle(SIM3D, "A", AMP, -AMP)) <= 1e-10
    # -0 is stored as 0
    z = d.copy()
    z[bot[0]] = (-0.0, 0.0, -0.0)
    eng.set_grip_field(z)
    assert not np.signbit(eng.grip_field()[0][bot[0]]).any()
    # mfea_set_mesh clears it; the getter then shows the band vectors row-wise
    eng.set_mesh(xyz, e2n)
    eng.set_bc(top, bot)
    got, is_set = eng.grip_field()
    assert not is_set
    want = np.zeros_like(d)
    want[top], want[bot] = EX, MIX2
    assert same_bits(got, want)
    eng.set_grip_motion(EY, EY)


def test_errors():
    from mfea import Engine, MfeaError
    from mfea._capi import EINVAL, ESTATE, _lib, _ptr
    xyz, e2n, top, bot = mesh_of(X)
    d = field_of(X, "A")
    with Engine(0) as e:
        with pytest.raises(MfeaError) as err:  # before a mesh
            e.set_grip_field(d)
        assert err.value.code == ESTATE
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_grip_field(d)
        for bad in (np.nan, np.inf, -np.inf):
            f = d.copy()
            f[top[0], 1] = bad
            with pytest.raises(MfeaError) as err:
                e.set_grip_field(f)
            assert err.value.code == EINVAL
            got, is_set = e.grip_field()  # the handle is unchanged
            assert is_set and same_bits(got, d + 0.0)  # (-0 is stored as 0)
        f = d.copy()
        f[[n for n in range(len(xyz)) if n not in set(top) | set(bot)][0], 0] = np.nan
        with pytest.raises(MfeaError) as err:  # ... a free node's row too
            e.set_grip_field(f)
        assert err.value.code == EINVAL
        # the getter accepts NULL for either argument
        flag = np.zeros(1, dtype=np.int32)
        assert _lib.mfea_get_grip_field(e._h, None, flag.ctypes.data_as(_lib.mfea_get_grip_field.argtypes[2])) == 0
        assert flag[0] == 1
        assert _lib.mfea_get_grip_field(e._h, None, None) == 0
        # a held band: zero rows are legal
        held = d.copy()
        held[bot] = 0.0
        e.set_grip_field(held)
        _, _, st = e.step(0.01, -0.01, opts(JACOBI), 1.0)
        assert st.status == 0
        assert not e.displacement().reshape(-1, 3)[bot].any()
        # a field, then partitions: MFEA_ESTATE at the next build
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.assemble()
        assert err.value.code == ESTATE
    with Engine(0) as e:  # partitions first: the setter refuses
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.set_grip_field(d)
        assert err.value.code == ESTATE
        assert not e.grip_field()[1]
        e.set_active(None)
        e.assemble()  # no field: the partitioned handle builds and runs
        assert e.solve(0.01, -0.01, opts(JACOBI)).status == 0


# ---------------------------------------------------------------------------
# 8. the drop-in solver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["loop", "device_run", "events"])
def test_dropin(tmp_path, mode):
    import shutil
    import pandas as pd
    import fea_solver as fs
    from conftest import GOLDEN
    from mfea import Engine
    dirn = str(tmp_path / "test_X")
    shutil.copytree(os.path.join(GOLDEN, "meshes", X), dirn)
    xyz, e2n, top, bot = mesh_of(X)
    d = field_of(X, "R")
    csv = str(tmp_path / "field.csv")
    with open(csv, "w") as f:  # the top band alone: the bottom takes its band vector
        f.write("node_id,dx,dy,dz\n")
        for n in top:
            f.write(f"{n},{float(d[n, 0])!r},{float(d[n, 1])!r},{float(d[n, 2])!r}\n")
    full = d.copy()
    full[bot] = EY
    dmax, steps = 0.004, 3
    try:
        fs.main([dirn, "--grip-field", csv, "--grip-length", str(GRIP[X]), "--n-steps", str(steps), "--disp-max",
                 str(dmax)] + {"loop": [], "device_run": ["--device-run"], "events": ["--events"]}[mode])
    finally:  # (main sets the module's constants)
        fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG = 40, 0.02, 0.018, 1e-12
    out = os.path.join(dirn, "fea_results")
    for name in ("stress_record.csv", "active_elements.csv", "node_displacements.csv", "force_displacement.csv"):
        assert os.path.exists(os.path.join(out, name)), name
    last = pd.read_csv(os.path.join(out, "node_displacements.csv"),
                       float_precision="round_trip").values[-1, :-1].astype(np.float64)  # (the step column is last)
    assert fs.get_engine().grip_field()[1]
    with Engine(0) as e:
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_grip_field(full)
        o = fs._opts(None, None, None)
        if mode == "events":
            run = e.run_events(dmax, -dmax, o, 0.018, 1e-9, 1.0)
            want = run["U"][run["n_done"] - 1]
        else:
            for k in range(steps):
                dy = dmax * (k / (steps - 1))
                _, _, st = e.step(dy, -dy, o, 0.018)
                assert st.status == 0
            want = e.displacement()
    assert len(last) == len(want) and np.linalg.norm(want) > 0
    assert rel(last, want) <= 1e-10, rel(last, want)
    if mode == "loop":  # ... and the direct solve of the last step
        known, vals = known_map(top, bot, dmax, -dmax, full)
        assert rel(last, fo.solve_system(K_of(X), known, vals)) <= 1e-10
