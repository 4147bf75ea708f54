"""Level 0's last up sweep and the CG's w = A u as one launch over block-local
rows (option amg_fuse_l0, amg.hip k_amg_up_w).  With the
option on against off at the SAME level-0 window every result is bit for bit
the same: the fused launch runs k_amg_up's and k_amg_cg_w's row bodies on the
same values and publishes the same partials.  amg_fused_l0 shows which path
ran.  The window alone (1408 against 4096 rows) moves rows inside windows, so
the partial sums' order and the last bits, not the iteration count."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_mesh

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (grip nodes only)

NO_FAILURE = 1e30  # a failure strain no element reaches
B = 1408


def _network(kind):
    """planar: the reference's 22,125-DOF network (2 DOFs per node, 7 k level-0
    rows: five blocks of 1408, the last one partial); 3d: the non-planar mesh
    (3 DOFs per node); c2: 1 × 5 tiles of the planar one."""
    if kind == "c2":
        from mfea import synth
        xyz, e2n = synth.tiled_mesh(1, 5)
        return (xyz, e2n) + synth.grips(xyz)
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


def _engine(kind, fuse, window=B, parts=0, **options):
    from mfea import Engine
    eng = Engine(0)
    eng.set_option("amg_fuse_l0", fuse)
    eng.set_option("amg_l0_window", window)
    for k, v in {"amg_merge": 0, **options}.items():
        eng.set_option(k, v)
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
    f, na, st = eng.step(dy, -dy, opts, max_strain)
    return {"force": f, "n_active": na, "iters": st.iters, "status": st.status, "relres": st.relres,
            "bnorm": st.bnorm, "levels": st.amg_levels, "U": eng.displacement(), "stress": eng.stress(),
            "active": eng.active(), "fused": eng.get_option("amg_fused_l0"),
            "window": eng.get_option("amg_l0_window_used")}


RESULTS = ("force", "n_active", "iters", "status", "relres", "bnorm", "U", "stress", "active")
DYS = [fo.DISPLACEMENT_MAX * k / (fo.N_STEPS - 1) for k in (3, 11, 7)]


def _both(kind, steps, applies=True, **engine_kw):
    """steps(eng) -> list of records with the option on and off at the same
    window; bit for bit equal, the fused launch in use only where it applies."""
    out = {}
    for fuse in (1, 0):
        eng = _engine(kind, fuse, **engine_kw)
        try:
            out[fuse] = steps(eng)
        finally:
            eng.close()
        for r in out[fuse]:
            assert r["fused"] == int(bool(fuse and applies)), (fuse, r["fused"])
            assert r["status"] == 0
    assert len(out[1]) == len(out[0])
    for k, (a, b) in enumerate(zip(out[1], out[0])):
        for key in RESULTS:
            assert np.array_equal(a[key], b[key]), (k, key, a[key], b[key])
    return out[1]


@pytest.mark.parametrize("kind", ["planar", "3d"])
@pytest.mark.parametrize("lazy", [0, 1])
def test_fused_equals_unfused(kind, lazy):
    """Three kept steps: nd = 2 and 3, the slim and the fat update."""
    recs = _both(kind, lambda eng: [_record(eng, dy, _gamg()) for dy in DYS], amg_lazy_px=lazy)
    assert all(r["window"] == B and r["levels"] >= 2 and r["iters"] > 4 for r in recs)
    assert not np.array_equal(recs[0]["U"], recs[1]["U"])  # (the steps do differ)


@pytest.mark.parametrize("kind", ["planar", "3d"])
def test_more_updates_than_slots_in_one_chunk(kind):
    """rtol 1e-13: the second solve is one planned batch of more than 16
    groups, so its u slots wrap around and a replay runs inside the chunk."""
    recs = _both(kind, lambda eng: [_record(eng, DYS[1], _gamg(rtol=1e-13)), _record(eng, DYS[1], _gamg(rtol=1e-13))])
    assert recs[0]["iters"] > 17 and recs[1]["iters"] == recs[0]["iters"]


def _floating_free(xyz, e2n, active, top, bot):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = len(xyz)
    a = e2n[active]
    _, lab = connected_components(sp.coo_matrix((np.ones(len(a)), (a[:, 0], a[:, 1])), shape=(n, n)), directed=False)
    anchored = np.zeros(lab.max() + 1, bool)
    grip = np.concatenate([top, bot])
    anchored[lab[grip]] = True
    fl = ~anchored[lab]
    fl[grip] = False
    return fl


def test_failed_network_on_a_kept_hierarchy():
    """6 % of the elements knocked out (seeded) behind an intact solve: the
    intact set's hierarchy is kept, floating pieces stay exactly at zero."""
    xyz, e2n, top, bot = _mesh("planar")
    active = np.random.default_rng(7).random(len(e2n)) > 0.06
    fl = _floating_free(xyz, e2n, active, top, bot)
    assert fl.sum() > 20

    def steps(eng):
        first = _record(eng, DYS[1], _gamg(rtol=1e-13))
        eng.set_active(active)
        second = _record(eng, DYS[1], _gamg(rtol=1e-13))
        assert eng.get_option("amg_reused") == 1
        assert np.all(second["U"].reshape(-1, 3)[fl] == 0.0)
        return [first, second]

    recs = _both("planar", steps, amg_reuse=1, amg_rebuild_pct=100000, amg_rebuild_rent=0)
    assert recs[1]["n_active"] == int(active.sum()) < recs[0]["n_active"]


def test_c2_unmerged():
    """1 × 5 tiles (33.9 k level-0 rows, 25 blocks) with its levels 0 and 1 not merged."""
    recs = _both("c2", lambda eng: [_record(eng, DYS[1], _gamg()), _record(eng, DYS[2], _gamg())])
    assert all(r["iters"] > 4 for r in recs)


def test_window_alone_keeps_the_iteration_count():
    """1408- against 4096-row windows, both unfused: the same iteration count
    and U within 1e-10 of the direct solve (tests/golden, as test_gpu_amg)."""
    sysz = np.load(os.path.join(GOLDEN, "sys_sim_20251117_181147_step20.npz"))
    dy = float(sysz["dy"])
    out = {}
    for window in (B, 4096):
        eng = _engine("planar", 0, window=window)
        try:
            tight = _record(eng, dy, _gamg(rtol=1e-13))
            loose = _record(eng, dy, _gamg())
        finally:
            eng.close()
        assert tight["window"] == window and tight["fused"] == 0 and tight["status"] == 0
        err = np.linalg.norm(tight["U"] - sysz["U"]) / np.linalg.norm(sysz["U"])
        print(f"window {window}: iterations {tight['iters']} / {loose['iters']}, U error {err:.3e}")
        assert err <= 1e-10
        out[window] = (tight["iters"], loose["iters"])
    assert out[B] == out[4096], out


def test_merged_plan_keeps_its_launches():
    def steps(eng):
        return [dict(_record(eng, dy, _gamg()), merged=eng.get_option("amg_merged")) for dy in DYS[:2]]

    recs = _both("planar", steps, applies=False, amg_merge=1)
    assert all(r["merged"] == 1 for r in recs)


def test_partitioned_keeps_its_launches():
    _both("planar", lambda eng: [_record(eng, dy, _gamg()) for dy in DYS[:2]], applies=False, parts=2)


def test_sor_keeps_its_launches():
    from mfea import PC_SOR
    _both("planar", lambda eng: [_record(eng, dy, _gamg(precond=PC_SOR)) for dy in DYS[:2]], applies=False)
