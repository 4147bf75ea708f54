"""The lazy p, x chain of the one-partition GAMG solve (option amg_lazy_px,
DESIGN.md §4.10): the update moves s, r and level 0's x only, every V-cycle of
a chunk keeps its u in a slot of its own, and a replay at the chunk's end runs
the p and x fma chains of the chunk's updates.  Every result is bit for bit
that of amg_lazy_px 0 in the same build; amg_px_replays shows which path ran.

Each test builds its own engines: the counter is a total since the handle's
creation."""
import numpy as np
import pytest

from conftest import load_mesh

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (grip nodes only)

NO_FAILURE = 1e30  # a failure strain no element reaches


def _network(kind):
    """planar: the reference's 22,125-DOF network (2 DOFs per node, >= 3
    levels, merged automatically); 3d: the non-planar mesh of test_gpu_amg."""
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


def _engine(kind, lazy, material=None, parts=0, **options):
    from mfea import Engine
    eng = Engine(0)
    eng.set_option("amg_lazy_px", lazy)
    for k, v in options.items():
        eng.set_option(k, v)
    if material is not None:
        eng.set_material(*material)
    if parts:
        eng.set_parts(parts, -1)
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
            "replays": eng.get_option("amg_px_replays")}


RESULTS = ("force", "n_active", "iters", "status", "code", "relres", "bnorm", "U", "stress", "active")


def _same(a, b, what):
    for k in RESULTS:
        assert np.array_equal(a[k], b[k], equal_nan=(k == "force")), (what, k, a[k], b[k])


DYS = [fo.DISPLACEMENT_MAX * k / (fo.N_STEPS - 1) for k in (3, 11, 7, 20, 1)]


def _both(kind, steps, lazy_runs=True, **engine_kw):
    """steps(eng) -> list of records, with the option on and off; the records
    equal bit for bit, the replays counted only where the path under test ran."""
    out = {}
    for lazy in (1, 0):
        eng = _engine(kind, lazy, **engine_kw)
        try:
            assert eng.get_option("amg_lazy_px") == lazy and eng.get_option("amg_px_slots") >= 2
            out[lazy] = steps(eng)
        finally:
            eng.close()
        for k, r in enumerate(out[lazy]):
            before = out[lazy][k - 1]["replays"] if k else 0
            # (every solve that ran the lazy chain queued a replay; none with the option off)
            assert (r["replays"] > before) == bool(lazy and lazy_runs), (lazy, k, r["replays"], before)
    assert len(out[1]) == len(out[0])
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        _same(a, b, k)
    return out[1]


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("collapse", [0, -1])
def test_kept_steps(kind, collapse):
    """Five kept steps; the merged (collapse -1 on the planar network) and the
    unmerged level-0 up launches write the slots."""
    merged = {}

    def steps(eng):
        recs = [_record(eng, dy, _gamg()) for dy in DYS]
        merged["m"] = eng.get_option("amg_merged")
        assert eng.get_option("amg_setup_kept") == 4
        return recs

    recs = _both(kind, steps, amg_collapse=collapse)
    if kind == "planar":
        assert merged["m"] == (1 if collapse else 0) and recs[0]["levels"] >= 3
    for r in recs:
        assert r["status"] == 0 and r["iters"] > 1
    assert not np.array_equal(recs[0]["U"], recs[1]["U"])  # (the steps do differ)


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("chunk", [1, 2, 3, 4])
def test_caller_chunks(kind, chunk):
    """The 15-20 iterations span several chunks and stop inside one: at its
    first launch, its last, in its middle (chunk sizes are rounded up to even)."""
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg(chunk=chunk)) for dy in DYS[:3]])
    for r in recs:
        assert r["status"] == 0 and r["iters"] > 4
    # several chunks each: more replays than solves
    assert recs[-1]["replays"] > 2 * len(recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_loose_tolerance_stops_in_the_first_chunk(kind):
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg(rtol=1e-2)) for dy in DYS[:3]])
    for r in recs:
        assert r["status"] == 0 and 0 < r["iters"] <= 8  # (the first solve plans for 16)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_big_chunk_16(kind):
    """Chunks of 16 groups with the entry's update: every slot in use."""
    recs = _both(kind, lambda eng: [_record(eng, DYS[1], _gamg(rtol=1e-12)), _record(eng, DYS[2], _gamg(rtol=1e-12)),
                                    _record(eng, DYS[3], _gamg())],
                 amg_big_chunk=16, batch_graph=0)
    # (the second solve's plan, the first's count, holds a whole chunk of 16 groups)
    assert recs[0]["iters"] > 17 and recs[1]["iters"] > 17 and all(r["status"] == 0 for r in recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_batch_longer_than_the_slots(kind):
    """A planned batch of more groups than slots (rtol 1e-12, one graph of its
    exact length): replays inside the chunk whenever the slots are full."""
    def steps(eng):
        assert eng.get_option("amg_px_slots") == 17
        recs = [_record(eng, DYS[1], _gamg(rtol=1e-12)), _record(eng, DYS[1], _gamg(rtol=1e-12))]
        assert recs[0]["iters"] > 18
        return recs

    recs = _both(kind, steps)
    # the second solve: one batch of iters − 1 groups, 1 + (groups − 1) // 16 replays
    groups = recs[1]["iters"] - 1
    assert recs[1]["status"] == 0 and recs[1]["iters"] == recs[0]["iters"]
    assert recs[1]["replays"] - recs[0]["replays"] == 1 + (groups - 1) // 16 >= 2


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("close", [0, 1])
def test_with_and_without_the_closing_check(kind, close):
    """amg_close 1: the replay rides in the closing check's launch; 0: its own."""
    hits = {}

    def steps(eng):
        recs = [_record(eng, dy, _gamg()) for dy in DYS[:3]]
        hits["h"] = eng.get_option("amg_close_hits")
        return recs

    _both(kind, steps, amg_close=close)
    assert (hits["h"] > 0) == bool(close)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_preconditioned_norm(kind):
    from mfea._capi import NORM_PRECONDITIONED
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg(norm=NORM_PRECONDITIONED)) for dy in DYS[:3]])
    assert all(r["status"] == 0 and r["iters"] > 1 for r in recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_max_it_leaves_the_same_state(kind):
    from mfea._capi import EMAXIT
    recs = _both(kind, lambda eng: [_record(eng, DYS[0], _gamg()), _record(eng, DYS[1], _gamg(max_it=5)),
                                    _record(eng, DYS[2], _gamg())])
    assert [r["code"] for r in recs] == [0, EMAXIT, 0] and recs[1]["iters"] == 5
    assert recs[1]["U"].any()


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_first_solve_one_chunk_at_a_time(kind):
    """The first solve of a handle (no plan), caller's chunks, no batch graph."""
    recs = _both(kind, lambda eng: [_record(eng, DYS[1], _gamg(chunk=2))], batch_graph=0, combo_graph=0)
    assert recs[0]["status"] == 0 and recs[0]["replays"] >= recs[0]["iters"] // 2


def test_new_active_set():
    """A few elements fail at a low max_strain: the next step sets up and
    solves on a new active set."""
    import fea_solver as fs
    thr = {}

    def steps(eng):
        first = _record(eng, DYS[3], _gamg())
        if "t" not in thr:
            eps = np.sort(np.abs(first["stress"]) / fs.E_mod)
            thr["t"] = 0.5 * (eps[-5] + eps[-6])  # the five most strained elements fail
        failing = _record(eng, DYS[3], _gamg(), thr["t"])
        return [first, failing, _record(eng, DYS[3], _gamg(), thr["t"]), _record(eng, DYS[1], _gamg(), thr["t"])]

    recs = _both("planar", steps, material=(fs.E_mod, fs.A, fs.I))
    assert recs[0]["n_active"] > recs[1]["n_active"] >= recs[0]["n_active"] - 8
    assert not np.array_equal(recs[1]["U"], recs[2]["U"])  # (the failed elements change the solution)
    assert all(r["status"] == 0 for r in recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_keep_operator_off(kind):
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg()) for dy in DYS[:3]], keep_operator=0)
    assert all(r["status"] == 0 for r in recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_graphs_off(kind):
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg()) for dy in DYS[:3]], graph=0)
    assert all(r["status"] == 0 for r in recs)


def test_partitioned_keeps_its_kernels():
    recs = _both("planar", lambda eng: [_record(eng, dy, _gamg()) for dy in DYS[:2]], lazy_runs=False, parts=2)
    assert all(r["status"] == 0 and r["replays"] == 0 for r in recs)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_sor_keeps_its_kernels(kind):
    from mfea import PC_SOR
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg(precond=PC_SOR)) for dy in DYS[:2]], lazy_runs=False)
    assert all(r["status"] == 0 and r["replays"] == 0 for r in recs)
