"""Strain energy per element on the device (mfea_get_energy, k_energy).

The device's rows are held bit for bit against csrc/energy.hpp run on the host
(tests/native/energy_main.cpp, the same header at the same contraction setting)
on the device's own U; the totals against an exactly rounded sum of the rows;
the physics against the oracle's heterogeneous K (the work identity) and
against central differences of the reported force through the whole engine.
Three meshes: one block (test_X, 14 elements), fewer blocks than the
reduction has shards (1,661 elements, 7 blocks) and more, with a ragged last
block (3,734 elements, 15 blocks)."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

import energy_ref as er
from conftest import GOLDEN, read_rt
from energy_ref import EY, PLANAR, SIM3D, X, same_bits
from test_gpu_props import GRAPHS_OFF, GRAPHS_ON, het_K

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

GAMG = 2
AMP = er.AMP
ULP = 2.0 ** -52
ROWS = ("w_axial", "w_bending", "g_axial", "g_bending")


@pytest.fixture(scope="module")
def eng():
    from mfea import Engine
    e = Engine(0)
    e.set_option("amg_rebuild_rent", 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return er.build_energy_main(tmp_path_factory.mktemp("energy_main"), sanitize=False)


def opts(rtol=1e-13, reg=1e-12):
    from mfea import make_opts
    return make_opts(precond=GAMG, rtol=rtol, max_it=200000, reg=reg)


def start(e, name, props=None, t=EY, b=EY):
    xyz, e2n, top, bot = er.mesh_of(name)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot)
    e.set_active(None)
    e.set_grip_motion(t, b)
    e.set_element_props(**(props or {}))
    return xyz, e2n, top, bot


def device_sections(e):
    """(EA_e, EI12_e) as the handle forms them, from what it says it uses."""
    p = e.element_props()
    return p["E"] * p["A"], (12.0 * p["E"]) * p["I"]


def rows_of(en):
    return [en[k] for k in ROWS]


# ---------------------------------------------------------------------------
# 1. the rows are the header's bits, the totals reproducible and well summed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("per_element", [False, True], ids=["uniform", "per_element"])
@pytest.mark.parametrize("name", er.MESHES)
def test_rows_are_the_headers_bits(eng, program, tmp_path, name, per_element):
    from mfea._capi import ElementEnergy, _lib, _ptr
    n = len(er.mesh_of(name)[1])
    props = er.props4(n) if per_element else None
    totals = {}
    for tag, graphs in (("on", GRAPHS_ON), ("off", GRAPHS_OFF)):
        with eng.options(**graphs):
            xyz, e2n, _, _ = start(eng, name, props)
            _, n_act, st = eng.step(AMP, -AMP, opts(), 1.0)
            assert st.status == 0 and n_act == n
            en = eng.energy()
            again = eng.energy()
            totals[tag] = (en["axial"], en["bending"])
            assert same_bits(totals[tag], (again["axial"], again["bending"]))
            for a, b in zip(rows_of(en), rows_of(again)):
                assert same_bits(a, b)
    assert same_bits(totals["on"], totals["off"])
    # (the last handle state: graphs off) the device's own U through the header on the host
    U = eng.displacement()
    EA, EI12 = device_sections(eng)
    want = er.run_energy_main(program, er.records(xyz, e2n, U, EA, EI12, np.ones(n, bool)), tmp_path)
    for k, (got, ref) in enumerate(zip(rows_of(en), want)):
        assert same_bits(got, ref), (ROWS[k], int(np.sum(got != ref)))
    assert same_bits(en["w_axial"], EA * en["g_axial"]) and same_bits(en["w_bending"], EI12 * en["g_bending"])
    # the totals: any summation order of n non-negative terms errs below
    # (n − 1)·2⁻⁵³ relative to first order; the bound doubles that
    for total, row in ((en["axial"], en["w_axial"]), (en["bending"], en["w_bending"])):
        exact = math.fsum(row)
        print(f"{name}: total {total:.17g}, |total - fsum|/fsum {abs(total - exact) / exact:.2e}")
        assert exact > 0.0 and abs(total - exact) <= n * ULP * exact
    # totals alone, and one row alone: written only where asked for, the same bits
    alone = eng.energy(elements=False)
    assert set(alone) == {"axial", "bending"} and same_bits((alone["axial"], alone["bending"]), totals["off"])
    one = np.full(n, -1.0)
    assert _lib.mfea_get_energy(eng._h, None, None, None, C.byref(ElementEnergy(None, _ptr(one), None, None))) == 0
    assert same_bits(one, en["w_bending"])
    assert _lib.mfea_get_energy(eng._h, None, None, None, None) == 0


# ---------------------------------------------------------------------------
# 2. the activity mask
# ---------------------------------------------------------------------------
def test_activity_mask(eng):
    xyz, e2n, _, _ = start(eng, SIM3D, er.props4(len(er.mesh_of(SIM3D)[1])))
    n = len(e2n)
    act0 = eng.active()
    assert act0.all()
    st = eng.solve(AMP, -AMP, opts())
    assert st.status == 0
    full = eng.energy()
    # a tenth off zeroes exactly those rows
    mask = er.tenth_off(SIM3D)
    part = eng.energy(active=mask)
    for a, b in zip(rows_of(part), rows_of(full)):
        assert np.all(a[~mask] == 0.0) and same_bits(a[mask], b[mask]) and np.any(b[~mask] > 0.0)
    assert part["axial"] < full["axial"] and part["bending"] < full["bending"]
    # a post that fails half of the strained elements (most of this sample hangs
    # loose and carries none), between mfea_solve and the next call
    eps = np.abs(fo.element_strain(xyz, e2n, eng.displacement()))
    _, n_act = eng.post(float(np.median(eps[eps > 1e-6])))
    after = eng.active()
    assert 0 < n_act < n and after.sum() == n_act
    # NULL: the handle's current activity, the post-failure one
    now, explicit = eng.energy(), eng.energy(active=after)
    for a, b in zip(rows_of(now), rows_of(explicit)):
        assert same_bits(a, b) and np.all(a[~after] == 0.0)
    assert same_bits((now["axial"], now["bending"]), (explicit["axial"], explicit["bending"]))
    # the pre-step mask: the rows of the call made between solve and post
    before = eng.energy(active=act0)
    for a, b in zip(rows_of(before), rows_of(full)):
        assert same_bits(a, b)
    assert same_bits((before["axial"], before["bending"]), (full["axial"], full["bending"]))


# ---------------------------------------------------------------------------
# 3. a caller's U
# ---------------------------------------------------------------------------
def test_callers_U(eng):
    start(eng, SIM3D, er.props4(len(er.mesh_of(SIM3D)[1])))
    assert eng.solve(AMP, -AMP, opts()).status == 0
    own = eng.energy()
    U = eng.displacement()
    given = eng.energy(U=U)
    twice = eng.energy(U=2.0 * U)
    tiny = np.finfo(np.float64).tiny
    for a, b, c in zip(rows_of(own), rows_of(given), rows_of(twice)):
        assert same_bits(a, b)
        assert np.all((a == 0.0) | (a >= tiny))  # no subnormal row: × 4 is exact
        assert same_bits(4.0 * a, c)
    assert same_bits((own["axial"], own["bending"]), (given["axial"], given["bending"]))
    # ... and the handle's own displacement is what it was
    assert same_bits(eng.displacement(), U)


# ---------------------------------------------------------------------------
# 4. the work identity against the oracle's heterogeneous K
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("motion", list(er.MOTIONS))
def test_work_identity(eng, motion):
    t, b = er.MOTIONS[motion]
    n = len(er.mesh_of(SIM3D)[1])
    props = er.props4(n)
    xyz, e2n, top, bot = start(eng, SIM3D, props, t, b)
    _, _, st = eng.step(AMP, -AMP, opts(), 1.0)
    assert st.status == 0
    en = eng.energy(elements=False)
    W2 = 2.0 * (en["axial"] + en["bending"])
    S_top, S_bot = eng.reaction()
    gap = W2 - (AMP * float(np.asarray(t) @ S_top) + (-AMP) * float(np.asarray(b) @ S_bot))
    K = het_K(xyz, e2n, np.ones(n, bool), props["E"], props["A"], props["I"]).tocsr()
    U = eng.displacement()
    known, _ = er.known_map(top, bot, AMP, -AMP, t, b)
    free = np.setdiff1d(np.arange(len(U)), known)
    resid = float(U[free] @ (K @ U)[free])
    scale = float(np.abs(U) @ (abs(K) @ np.abs(U)))
    print(f"{motion}: 2W {W2:.6e}, gap/2W {gap / W2:.2e}, u_f.(KU)_f/2W {resid / W2:.2e}, "
          f"|gap - resid| {abs(gap - resid):.2e} against 1e-12 * |U||K||U| = {1e-12 * scale:.2e}")
    assert W2 > 2.0 * er.LOADED
    assert abs(gap - resid) <= 1e-12 * scale


# ---------------------------------------------------------------------------
# 5. the gradient of the reported force, through the whole engine
# ---------------------------------------------------------------------------
def test_force_gradient_end_to_end(eng):
    """(F(θ_e + h) − F(θ_e − h)) / 2h through set_element_props and a step,
    against 2 · dW/dθ_e / (dy_top − dy_bot) from energy_gradient().  reg = 0: a
    regularised solve minimises W + ½ reg |u_f|², not W, and 1e-12 is 1e-5 of
    this mesh's bending stiffness (tests/test_energy_cpu.py measures what that
    does to dW/dI_e)."""
    n = len(er.mesh_of(X)[1])
    props = er.props4(n)
    o = opts(reg=0.0)
    with eng.options(**GRAPHS_OFF):
        start(eng, X, props)
        _, _, st = eng.step(AMP, -AMP, o, 1.0)
        assert st.status == 0
        en = eng.energy()
        grad = eng.energy_gradient()
        W = en["axial"] + en["bending"]
        heavy = np.flatnonzero(en["w_axial"] + en["w_bending"] >= 0.02 * W)
        assert len(heavy) >= 4
        worst = {}
        for e in heavy:
            for k in ("E", "A", "I"):
                h = 1e-4 * props[k][e]
                F = []
                for sign in (+1.0, -1.0):
                    p = {**props, k: props[k].copy()}
                    p[k][e] += sign * h
                    eng.set_element_props(**p)
                    f, _, st = eng.step(AMP, -AMP, o, 1.0)
                    assert st.status == 0
                    F.append((f, p[k][e]))
                fd = (F[0][0] - F[1][0]) / (F[0][1] - F[1][1])
                want = 2.0 * grad[k][e] / (AMP - (-AMP))
                err = abs(fd - want) / abs(want)
                worst[k] = max(worst.get(k, 0.0), err)
                print(f"element {int(e)} d/d{k}: central difference {fd:.9e}, from the energy rows {want:.9e}, "
                      f"relative error {err:.2e}")
                assert err <= 1e-6, (int(e), k)
        print("worst relative error per property:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------
# 6. the call changes nothing a later call can see
# ---------------------------------------------------------------------------
def _three_steps(e, with_energy):
    xyz, e2n, top, bot = er.mesh_of(PLANAR)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot)
    e.set_active(None)
    out = []
    mask = er.tenth_off(PLANAR)
    for d in (0.004, 0.008, 0.014):
        f, n_act, st = e.step(d, -d, opts(1e-12), 0.018)
        assert st.status == 0
        out.append((f, n_act, st.iters, e.displacement(), e.stress(), e.active()))
        if with_energy:
            en = e.energy()
            assert en["axial"] > 0.0
            e.energy(U=0.5 * out[-1][3], active=mask, elements=False)
    return out, e.get_option("op_kept_steps")


@pytest.mark.parametrize("graphs", [GRAPHS_ON, GRAPHS_OFF], ids=["graphs_on", "graphs_off"])
def test_invisible_to_later_calls(graphs):
    from mfea import Engine
    res = []
    for with_energy in (False, True):
        with Engine(0) as e:
            e.set_option("amg_rebuild_rent", 0)
            for k, v in graphs.items():
                e.set_option(k, v)
            res.append(_three_steps(e, with_energy))
    (plain, kept_plain), (probed, kept_probed) = res
    n = len(er.mesh_of(PLANAR)[1])
    assert plain[0][1] == n and plain[1][1] == n and plain[2][1] < n  # kept step, then failures
    assert kept_plain >= 1 and kept_probed == kept_plain
    for a, b in zip(plain, probed):
        assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
        assert same_bits(a[3], b[3]) and same_bits(a[4], b[4]) and np.array_equal(a[5], b[5])


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def test_errors():
    from mfea import Engine, MfeaError
    from mfea._capi import ESTATE
    xyz, e2n, top, bot = er.mesh_of(X)
    with Engine(0) as e:
        with pytest.raises(MfeaError) as err:  # before set_mesh
            e.energy()
        assert err.value.code == ESTATE
        e.set_mesh(xyz, e2n)
        with pytest.raises(MfeaError) as err:  # no boundary conditions
            e.energy()
        assert err.value.code == ESTATE
        e.set_bc(top, bot)
        assert e.energy()["axial"] == 0.0  # no assembly, no solve needed: U = 0
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.energy()
        assert err.value.code == ESTATE
        with pytest.raises(ValueError):
            Engine.energy(e, U=np.zeros(3))


# ---------------------------------------------------------------------------
# 8. the command line's three run modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["loop", "device_run", "events"])
def test_dropin_energy(tmp_path, monkeypatch, mode):
    import fea_solver as fs
    d = str(tmp_path / "test_X")
    shutil.copytree(os.path.join(GOLDEN, "meshes", X), d)
    monkeypatch.setattr(fs, "N_STEPS", 3)
    monkeypatch.setattr(fs, "DISPLACEMENT_MAX", 0.004 if mode != "events" else 0.06)
    args = [d, "--energy", "--grip-length", str(er.GRIP[X]), "--n-steps", "3", "--npy",
            "--disp-max", str(fs.DISPLACEMENT_MAX)]
    fs.main(args + {"loop": [], "device_run": ["--device-run"], "events": ["--events", "--max-events", "3"]}[mode])
    out = os.path.join(d, "fea_results")
    en = read_rt(os.path.join(out, "energy.csv"))
    assert list(en.columns) == ["step", "total_displacement", "axial_energy", "bending_energy"]
    force = read_rt(os.path.join(out, "force_displacement.csv"))
    n_rows = len(force)
    assert len(en) == n_rows >= (3 if mode != "events" else 1)
    assert np.array_equal(en["total_displacement"].values, force["total_displacement"].values)
    active = np.load(os.path.join(out, "active_elements.npy"))
    n = active.shape[1]
    for name, col in (("element_energy_axial", "axial_energy"), ("element_energy_bending", "bending_energy")):
        rows = read_rt(os.path.join(out, name + ".csv")).drop(columns="step").values  # (the stress record's layout)
        assert rows.shape == (n_rows, n) and same_bits(rows, np.load(os.path.join(out, name + ".npy")))
        for k in range(n_rows):
            exact = math.fsum(rows[k])
            assert abs(en[col].values[k] - exact) <= n * ULP * exact, (name, k)
            # the row counts the elements active BEFORE the step / event
            before = np.ones(n, bool) if k == 0 else active[k - 1]
            assert np.all(rows[k][~before] == 0.0)
            if k and mode != "events":  # (after a break an element may hang between unloaded nodes)
                assert np.all(rows[k][before] > 0.0)
    if mode == "events":
        assert not active[0].all() and en["axial_energy"].values[0] > 0.0
        return
    # a step without failures: W = ½ · total_displacement · total_force, up to
    # the free rows' term of the work identity.  The solve is the regularised
    # one, (K_ff + reg·I) u_f = b_f, so (K U)_f = −reg·u_f to the PCG's rtol
    # (1e-13): u_fᵀ(KU)_f = −reg·|u_f|², and — K annihilates a translation, so
    # the three bands' y sums add to zero — the bottom band's reaction is
    # −F + reg·Σ u_fy.  Both are formed from the U record and taken out; what is
    # left is the 1e-9 bar's.
    assert active.all()
    _, _, top, bot = er.mesh_of(X)
    U = np.load(os.path.join(out, "node_displacements.npy")).reshape(n_rows, -1, 3)
    free = np.setdiff1d(np.arange(U.shape[1]), np.concatenate([top, bot]))
    for k in range(1, n_rows):
        W2 = 2.0 * (en["axial_energy"].values[k] + en["bending_energy"].values[k])
        span, F = force["total_displacement"].values[k], force["total_force"].values[k]
        uf = U[k][free]
        reg_terms = -fs.REG * (float(np.sum(uf * uf)) + 0.5 * span * float(np.sum(uf[:, 1])))
        print(f"{mode} step {k + 1}: 2W {W2:.9e}, span*F {span * F:.9e}, gap/2W {(W2 - span * F) / W2:.3e}, "
              f"regularisation terms/2W {reg_terms / W2:.3e}, left {(W2 - span * F - reg_terms) / W2:.2e}")
        assert abs(W2 - span * F - reg_terms) <= 1e-9 * W2
