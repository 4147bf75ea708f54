"""mfea_step keeps K and the GAMG hierarchy's values while what they were
formed from holds (option keep_operator): every result is bit
for bit that of a step which assembles and sets up (keep_operator 0), the
counters op_kept_steps / amg_setup_kept show that the kept path really ran,
and every change of an input re-forms what depends on it.

Each test builds its own engines: the counters are totals since the handle's
creation."""
import numpy as np
import pytest

from conftest import load_mesh

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (grip nodes only)

NO_FAILURE = 1e30  # a failure strain no element reaches


def _network(kind):
    """planar: the reference's 22,125-DOF network (2 DOFs per node, >= 3
    levels); 3d: the non-planar mesh of test_gpu_amg (3 DOFs per node)."""
    name, band = {"planar": ("sim_20251117_181147", 1.5), "3d": ("sim_20251115_135507", 0.5)}[kind]
    nodes, elems = load_mesh(name)
    xyz = nodes[["x", "y", "z"]].values
    top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, band)
    return xyz, elems[["n1", "n2"]].values, top, bot


_MESH = {}


def _mesh(kind):
    if kind not in _MESH:
        _MESH[kind] = _network(kind)
    return _MESH[kind]


def _engine(kind, keep, material=None, **options):
    from mfea import Engine
    eng = Engine(0)
    eng.set_option("keep_operator", keep)
    for k, v in options.items():
        eng.set_option(k, v)
    if material is not None:
        eng.set_material(*material)
    xyz, e2n, top, bot = _mesh(kind)
    eng.set_mesh(xyz, e2n)
    eng.set_bc(top, bot)
    eng.set_active(None)
    return eng


def _gamg(**kw):
    from mfea import PC_GAMG, make_opts
    return make_opts(**{"rtol": 1e-8, "max_it": 2000, "precond": PC_GAMG, **kw})


def _counters(eng):
    return eng.get_option("op_kept_steps"), eng.get_option("amg_setup_kept")


def _record(eng, dy, opts, max_strain=NO_FAILURE):
    f, na, st = eng.step(dy, -dy, opts, max_strain)
    return {"force": f, "n_active": na, "iters": st.iters, "relres": st.relres, "levels": st.amg_levels,
            "U": eng.displacement(), "stress": eng.stress()}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


DYS = [fo.DISPLACEMENT_MAX * k / (fo.N_STEPS - 1) for k in (3, 11, 7, 20, 1)]


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("collapse", [0, -1])
@pytest.mark.parametrize("fuse", [0, 1])
def test_kept_steps_equal_fresh_steps_bitwise(kind, collapse, fuse):
    out = {}
    for keep in (1, 0):
        eng = _engine(kind, keep, amg_fuse_setup=fuse, amg_collapse=collapse)
        try:
            out[keep] = [_record(eng, dy, _gamg()) for dy in DYS]
            kept = _counters(eng)
        finally:
            eng.close()
        # (the equalities that keep this test from passing with the feature off)
        assert kept == ((4, 4) if keep else (0, 0)), (keep, kept)
    if kind == "planar":
        assert out[1][0]["levels"] >= 3
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)
    assert not np.array_equal(out[1][0]["U"], out[1][1]["U"])  # (the steps do differ)


def _failure_run(keep, through_run):
    """The 40 load steps of the reference's network, failures included
    (bench.full_run_reference's mesh, grip band, material and strain)."""
    import fea_solver as fs
    eng = _engine("planar", keep, material=(fs.E_mod, fs.A, fs.I))
    dys = np.array([fs.DISPLACEMENT_MAX * k / (fs.N_STEPS - 1) for k in range(fs.N_STEPS)])
    try:
        if through_run:
            r = eng.run(dys, -dys, _gamg(), fs.MAX_STRAIN)
            rec = {"force": r["force"], "n_active": r["n_active"], "U": r["U"], "stress": r["stress"],
                   "active": r["active"], "iters": np.array([s["iters"] for s in r["stats"]]),
                   "relres": np.array([s["relres"] for s in r["stats"]]),
                   "rebuilt": np.array([s["amg_rebuilt"] for s in r["stats"]])}
            return rec, None, _counters(eng), eng.n_elems
        rows, per_step = [], []
        for dy in dys:
            before = _counters(eng)
            f, na, st = eng.step(dy, -dy, _gamg(), fs.MAX_STRAIN)
            after = _counters(eng)
            per_step.append((after[0] - before[0], after[1] - before[1]))
            rows.append((f, na, st.iters, st.relres, st.amg_rebuilt, eng.displacement(), eng.stress(), eng.active()))
        names = ("force", "n_active", "iters", "relres", "rebuilt", "U", "stress", "active")
        rec = {n: np.array([r[i] for r in rows]) for i, n in enumerate(names)}
        return rec, per_step, _counters(eng), eng.n_elems
    finally:
        eng.close()


@pytest.mark.parametrize("through_run", [False, True], ids=["steps", "mfea_run"])
def test_failure_run_reforms_exactly_on_new_sets(through_run):
    from bench import new_set_steps
    on, per_step, total, n_elems = _failure_run(1, through_run)
    off, _, total_off, _ = _failure_run(0, through_run)
    assert total_off == (0, 0)
    assert len(on["force"]) == 40 and on["n_active"][-1] < n_elems  # (elements did fail)
    for k in on:
        assert np.array_equal(on[k], off[k]), k
    new_set = new_set_steps([int(n) for n in on["n_active"]], n_elems)
    assert 0 < sum(new_set) < 39
    # K: exactly the steps on a new set assemble.  The hierarchy's values: the
    # same steps, and a step that rebuilt the hierarchy itself (a kept one
    # that degraded is rebuilt on the step AFTER the one that showed it, which
    # may run on an unchanged set: its new arrays hold no values yet)
    want_k = [1 - c for c in new_set[1:]]
    want_s = [(1 - c) * (1 - int(r)) for c, r in zip(new_set[1:], on["rebuilt"][1:])]
    if per_step is not None:
        assert per_step[0] == (0, 0)
        assert [p[0] for p in per_step[1:]] == want_k
        assert [p[1] for p in per_step[1:]] == want_s
    assert total == (sum(want_k), sum(want_s))


def test_set_material_between_steps_reforms_k_and_the_graphs():
    import fea_solver as fs
    m1 = (fs.E_mod, fs.A, fs.I)
    m2 = (1.5 * fs.E_mod, fs.A, 4.0 * fs.I)
    dy = DYS[1]
    graphs = {"batch_graph": 1, "combo_graph": 1}
    eng = _engine("planar", 1, material=m1, **graphs)
    try:
        first = _record(eng, DYS[0], _gamg())
        _record(eng, dy, _gamg())
        assert _counters(eng) == (1, 1)
        eng.set_material(*m2)
        changed = _record(eng, dy, _gamg())
        assert _counters(eng) == (1, 1)  # the step after the change: not kept
        again = _record(eng, dy, _gamg())
        assert _counters(eng) == (2, 2)
    finally:
        eng.close()
    fresh_eng = _engine("planar", 1, material=m2, **graphs)
    try:
        _record(fresh_eng, DYS[0], _gamg())
        fresh = _record(fresh_eng, dy, _gamg())
    finally:
        fresh_eng.close()
    _same(changed, fresh, "after set_material")
    _same(again, fresh, "kept after set_material")
    assert not np.array_equal(first["stress"], changed["stress"])


def _mask_and_back(eng, _):
    a = np.ones(eng.n_elems, np.uint8)
    a[::97] = 0
    eng.set_active(a)
    eng.set_active(None)


def _jacobi_step(eng, out):
    from mfea import PC_BLOCK_JACOBI, make_opts
    out.append(_record(eng, DYS[2], make_opts(rtol=1e-8, max_it=200000, precond=PC_BLOCK_JACOBI)))


def _assemble(eng, _):
    eng.assemble()


def _max_it_step(eng, out):
    from mfea import SolverFailure
    from mfea._capi import EMAXIT
    with pytest.raises(SolverFailure) as e:
        eng.step(DYS[2], -DYS[2], _gamg(max_it=2), NO_FAILURE)
    assert e.value.code == EMAXIT


# change, the options of the steps after it, whether K too must be re-formed
# (reg, the preconditioner kind and an explicit assembly leave K what it was:
# only the hierarchy's values depend on them / are older than it)
INVALIDATIONS = {
    "set_active": (_mask_and_back, {}, True),
    "reg": (None, {"reg": 1e-9}, False),
    "jacobi_between": (_jacobi_step, {}, False),
    "assemble": (_assemble, {}, False),
    "max_it": (_max_it_step, {}, True),
}


@pytest.mark.parametrize("name", list(INVALIDATIONS))
def test_invalidation_reforms_once_then_keeps(name):
    change, after_kw, k_too = INVALIDATIONS[name]
    out = {}
    for keep in (1, 0):
        eng = _engine("planar", keep)
        try:
            rec = [_record(eng, DYS[0], _gamg()), _record(eng, DYS[1], _gamg())]
            c0 = _counters(eng)
            if change is not None:
                change(eng, rec)
            c1 = _counters(eng)
            rec.append(_record(eng, DYS[3], _gamg(**after_kw)))
            c2 = _counters(eng)
            rec.append(_record(eng, DYS[4], _gamg(**after_kw)))
            c3 = _counters(eng)
        finally:
            eng.close()
        out[keep] = rec
        if not keep:
            assert c3 == (0, 0)
            continue
        assert c0 == (1, 1)
        assert c2[1] == c1[1], (name, "the step after the change kept the setup")
        assert c3[1] == c2[1] + 1, (name, "the step after that did not")
        assert c2[0] == c1[0] + (0 if k_too else 1), (name, "K after the change")
        assert c3[0] == c2[0] + 1
    assert len(out[1]) == len(out[0])
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, (name, k))


def test_rtol_change_keeps():
    out = {}
    for keep in (1, 0):
        eng = _engine("planar", keep)
        try:
            rec = [_record(eng, DYS[0], _gamg()), _record(eng, DYS[1], _gamg())]
            rec += [_record(eng, DYS[3], _gamg(rtol=1e-11, max_it=500)), _record(eng, DYS[4], _gamg(rtol=1e-11, max_it=500))]
            assert _counters(eng) == ((3, 3) if keep else (0, 0))
        finally:
            eng.close()
        out[keep] = rec
    assert out[1][2]["iters"] > out[1][1]["iters"]  # (the tolerance did change the solve)
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)


def _writable_options():
    from mfea import _capi
    return [(n, bool(f & _capi.OPT_KEEPS_KEPT)) for n, _, f in _capi.option_info() if f & _capi.OPT_WRITABLE]


@pytest.mark.parametrize("name,keeps", _writable_options())
def test_setting_an_option_keeps_or_drops_the_kept_operator(name, keeps):
    """Setting an option — here to the value it has, so nothing else changes —
    drops the kept K and hierarchy values unless the option's table row says
    it keeps them (mfea_debug_option_info's MFEA_OPT_KEEPS_KEPT; keep_operator
    itself keeps when set to 1).  Either way the next step's results are those
    of the kept step before it at the same grip displacement, bit for bit."""
    keeps = keeps or name == "keep_operator"
    eng = _engine("3d", 1)
    try:
        _record(eng, DYS[0], _gamg())
        kept = _record(eng, DYS[1], _gamg())
        c1 = _counters(eng)
        assert c1 == (1, 1)  # (the second step was a kept one)
        eng.set_option(name, 1 if name == "keep_operator" else eng.get_option(name))
        after = _record(eng, DYS[1], _gamg())
        c2 = _counters(eng)
    finally:
        eng.close()
    assert c2 == ((2, 2) if keeps else (1, 1)), (name, c2)
    assert after["force"] == kept["force"] and np.array_equal(after["U"], kept["U"])
