"""The closing check of the one-partition GAMG solve (option amg_close,
DESIGN.md §4.8): every chunk ends by testing ‖r‖² of its last update, the
planned batch is one (V-cycle, w = A u, update) group shorter, and a solve of
n iterations applies n V-cycles instead of n + 1.  Every result is bit for bit
that of amg_close 0 in the same build; amg_last_cycles / amg_close_hits show
which path really ran.

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


def _engine(kind, close, material=None, **options):
    from mfea import Engine
    eng = Engine(0)
    eng.set_option("amg_close", close)
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


def _record(eng, dy, opts, max_strain=NO_FAILURE):
    """One step's results, a solver stop included (its code, and the state it left)."""
    from mfea import SolverFailure
    try:
        f, na, st = eng.step(dy, -dy, opts, max_strain)
        code = 0
    except SolverFailure as e:
        f, na, st, code = np.nan, -1, e.stats, e.code
    return {"force": f, "n_active": na, "iters": st.iters, "status": st.status, "code": code,
            "relres": st.relres, "bnorm": st.bnorm, "levels": st.amg_levels,
            "U": eng.displacement(), "stress": eng.stress(), "active": eng.active(),
            "cycles": eng.get_option("amg_last_cycles"), "hits": eng.get_option("amg_close_hits")}


RESULTS = ("force", "n_active", "iters", "status", "code", "relres", "bnorm", "U", "stress", "active")


def _same(a, b, what):
    for k in RESULTS:
        assert np.array_equal(a[k], b[k], equal_nan=(k == "force")), (what, k, a[k], b[k])


DYS = [fo.DISPLACEMENT_MAX * k / (fo.N_STEPS - 1) for k in (3, 11, 7, 20, 1)]


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("collapse", [0, -1])
def test_kept_steps_run_iters_cycles(kind, collapse):
    out = {}
    for close in (1, 0):
        eng = _engine(kind, close, amg_collapse=collapse)
        try:
            out[close] = [_record(eng, dy, _gamg()) for dy in DYS]
            merged = eng.get_option("amg_merged")
            kept = eng.get_option("amg_setup_kept")
        finally:
            eng.close()
        assert kept == 4
        if kind == "planar":  # (the merged levels: automatic on this network around a level-2 collapse)
            assert merged == (1 if collapse else 0) and out[close][0]["levels"] >= 3
        # (the equalities that keep this test from passing with the feature off)
        for k in range(1, len(DYS)):
            r, before = out[close][k], out[close][k - 1]
            assert r["status"] == 0 and r["iters"] > 1
            assert r["cycles"] == r["iters"] + (0 if close else 1), (close, k, r["cycles"], r["iters"])
            assert r["hits"] - before["hits"] == (1 if close else 0), (close, k)
        assert close or out[0][-1]["hits"] == 0
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)
    assert not np.array_equal(out[1][0]["U"], out[1][1]["U"])  # (the steps do differ)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_plan_too_long_stops_inside_the_chunk(kind):
    """A first solve plans for 16 iterations, more than these networks take at
    rtol 1e-3 (16 and 21 at 1e-8): an update inside the batch finds the
    convergence, the check is never reached."""
    out = {}
    for close in (1, 0):
        eng = _engine(kind, close)
        try:
            out[close] = _record(eng, DYS[1], _gamg(rtol=1e-3))
        finally:
            eng.close()
        assert 0 < out[close]["iters"] <= 15 and out[close]["hits"] == 0
        assert out[close]["cycles"] == (16 if close else 17)  # (the entry's, then the batch's)
    _same(out[1], out[0], kind)


def test_plan_too_short_goes_on_in_small_chunks():
    out = {}
    for close in (1, 0):
        eng = _engine("planar", close)
        try:
            out[close] = [_record(eng, DYS[1], _gamg(rtol=1e-5)), _record(eng, DYS[1], _gamg(rtol=1e-5)),
                          _record(eng, DYS[1], _gamg(rtol=1e-10))]
        finally:
            eng.close()
        a, b, c = out[close]
        # the second solve ends at its check; the third's planned batch (b.iters − 1 groups, or
        # b.iters) ends with a check that fails — it would have reported b.iters iterations —
        # and the solve goes on in chunks of two groups, each with its own check
        d = c["iters"] - b["iters"]
        assert d > 1 and c["status"] == 0 and b["hits"] == close
        k = (d + 1) // 2  # the small chunks it takes
        assert c["cycles"] == b["iters"] + 2 * k + (0 if close else 1), (close, b["iters"], c["iters"], c["cycles"])
        # (an even distance: the last small chunk's check is what ends it)
        assert c["hits"] - b["hits"] == (1 if close and d % 2 == 0 else 0)
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_max_it_at_the_edge(kind):
    free = {}
    out = {}
    for close in (1, 0):
        eng = _engine(kind, close)
        try:
            _record(eng, DYS[0], _gamg())
            free[close] = _record(eng, DYS[1], _gamg())
            n = free[close]["iters"]
            out[close] = [_record(eng, DYS[1], _gamg(max_it=m)) for m in (n - 1, n, n + 1)]
        finally:
            eng.close()
    _same(free[1], free[0], "free")
    n = free[1]["iters"]
    from mfea._capi import EMAXIT
    assert [r["code"] for r in out[1]] == [EMAXIT, 0, 0]
    assert [r["iters"] for r in out[1]] == [n - 1, n, n]
    assert [r["hits"] - free[1]["hits"] for r in out[1]] == [0, 1, 2]
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_zero_right_hand_side(kind):
    out = {}
    for close in (1, 0):
        eng = _engine(kind, close)
        try:
            out[close] = [_record(eng, 0.0, _gamg()), _record(eng, 0.0, _gamg()), _record(eng, DYS[1], _gamg())]
        finally:
            eng.close()
        for r in out[close][:2]:
            assert r["iters"] == 0 and r["status"] == 0 and not r["U"].any()
        assert out[close][2]["iters"] > 0
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_preconditioned_norm_keeps_its_path(kind):
    from mfea._capi import NORM_PRECONDITIONED
    out = {}
    for close in (1, 0):
        eng = _engine(kind, close)
        try:
            out[close] = [_record(eng, dy, _gamg(norm=NORM_PRECONDITIONED)) for dy in DYS[:3]]
        finally:
            eng.close()
        for r in out[close][1:]:
            assert r["hits"] == 0 and r["cycles"] == r["iters"] + 1 and r["status"] == 0
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)


def _failure_run(close, through_run):
    """The 40 load steps of the reference's network, failures included
    (bench.full_run_reference's mesh, grip band, material and strain)."""
    import fea_solver as fs
    eng = _engine("planar", close, material=(fs.E_mod, fs.A, fs.I))
    dys = np.array([fs.DISPLACEMENT_MAX * k / (fs.N_STEPS - 1) for k in range(fs.N_STEPS)])
    try:
        if through_run:
            r = eng.run(dys, -dys, _gamg(), fs.MAX_STRAIN)
            rec = {"force": r["force"], "n_active": r["n_active"], "U": r["U"], "stress": r["stress"],
                   "active": r["active"]}
            for k in ("iters", "status", "relres", "bnorm", "amg_rebuilt"):
                rec[k] = np.array([s[k] for s in r["stats"]])
        else:
            rows = []
            for dy in dys:
                f, na, st = eng.step(dy, -dy, _gamg(), fs.MAX_STRAIN)
                rows.append((f, na, st.iters, st.status, st.relres, st.bnorm, st.amg_rebuilt, eng.displacement(),
                             eng.stress(), eng.active()))
            names = ("force", "n_active", "iters", "status", "relres", "bnorm", "amg_rebuilt", "U", "stress", "active")
            rec = {n: np.array([r[i] for r in rows]) for i, n in enumerate(names)}
        return rec, eng.get_option("amg_close_hits"), eng.n_elems
    finally:
        eng.close()


@pytest.mark.parametrize("through_run", [False, True], ids=["steps", "mfea_run"])
def test_failure_run_records_equal(through_run):
    on, hits, n_elems = _failure_run(1, through_run)
    off, hits_off, _ = _failure_run(0, through_run)
    assert hits_off == 0 and hits > 0
    assert len(on["force"]) == 40 and on["n_active"][-1] < n_elems  # (elements did fail)
    for k in on:
        assert np.array_equal(on[k], off[k]), k


def _grip_adjacent_mask(kind):
    """Every second element with a node in a grip switched off: known
    couplings of free rows whose K blocks are exact zeros."""
    _, e2n, top, bot = _mesh(kind)
    grip = np.zeros(int(e2n.max()) + 1, bool)
    grip[np.asarray(top)] = True
    grip[np.asarray(bot)] = True
    at_grip = np.flatnonzero(grip[e2n[:, 0]] | grip[e2n[:, 1]])
    assert len(at_grip) >= 4
    a = np.ones(len(e2n), np.uint8)
    a[at_grip[::2]] = 0
    return a


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("mask", [False, True], ids=["all_active", "grip_elements_off"])
def test_start_as_one_launch_equals_three(kind, mask):
    """Option amg_start: the RHS, the CG's state and level-0 b of a kept step
    as one launch (k_amg_start) against the three launches, bit for bit."""
    out = {}
    for start in (1, 0):
        eng = _engine(kind, 1, amg_start=start)
        try:
            if mask:
                eng.set_active(_grip_adjacent_mask(kind))
            out[start] = [_record(eng, dy, _gamg()) for dy in DYS]
            fused = eng.get_option("amg_start_fused")
            kept = eng.get_option("amg_setup_kept")
        finally:
            eng.close()
        # (the equalities that keep this test from passing with the option off)
        assert kept == 4 and fused == (4 if start else 0), (start, kept, fused)
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)
    assert out[1][1]["bnorm"] > 0 and not np.array_equal(out[1][0]["U"], out[1][1]["U"])
