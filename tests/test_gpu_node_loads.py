"""Nodal loads (mfea_set_node_loads): a force vector per free node, dead or
proportional, on every entry point.

The checker is the oracle's own free system: A, b, free = fo.free_system(K,
known, vals) and U_f = spsolve(A, b + q[free]), with q the load as the header
defines it — f in dead mode, np.float64(dy_top) * f in proportional mode — and
zeroed on the floating nodes, which the checker finds with
scipy.sparse.csgraph.connected_components on the active element graph.

The meshes carry a displacement of about 1e6 per unit force, so the load sets
are of the order 1e-8: P, point loads on five interior nodes, and S, the
self-weight of every element along −y.  In proportional mode the same arrays
are scaled by 1 / AMP, so both modes load the network alike at dy_top = AMP.

Bars.  U: test_gpu_grip_field's, relative error <= 1e-10 at rtol 1e-13.  Sums
(load_work, bnorm): the dot-product bound γ_n of their n terms.  Everything
called an identity is bit equality."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components
from scipy.sparse.linalg import spsolve

from test_gpu_grip_motion import (AMP, EY, GAMG, GRIP, ICC, JACOBI, BJACOBI, MAX_STRAIN, PLANAR, SIM3D, SOR,
                                  U_ROUND, X, K_of, mesh_of, opts, rel)
from test_gpu_grip_field import field_of, known_map as field_known_map
from test_gpu_events import rule
from test_gpu_props import GRAPHS_OFF, GRAPHS_ON, het_K, recipe, same_bits

pytestmark = pytest.mark.gpu

import fea_oracle as fo  # noqa: E402  (checker only)

ALL_PC = (JACOBI, BJACOBI, GAMG, SOR, ICC)
DEAD, PROP = "dead", "proportional"
PT_VEC = (2.0e-8, -4.0e-8, 0.0)  # the point load; on the 3-D mesh with a z part
PT_VEC3 = (2.0e-8, -4.0e-8, 1.5e-8)
SW = 1.0e-8                      # weight per length of the self-weight


@pytest.fixture(scope="module")
def eng():
    from mfea import Engine
    e = Engine(0)
    e.set_option("amg_rebuild_rent", 0)
    yield e
    e.close()


_loads, _ref, _Kact = {}, {}, {}


def gamma(n):
    return n * U_ROUND / (1.0 - n * U_ROUND)


def free_nodes(name):
    xyz, _, top, bot = mesh_of(name)
    g = np.zeros(len(xyz), bool)
    g[top] = g[bot] = True
    return np.flatnonzero(~g)


def loads_of(name, tag, mode=DEAD):
    """The named load set on the named mesh, once: P point loads on five
    interior nodes spread over the free nodes, S the self-weight along −y, Z (the
    planar mesh) P with an out-of-plane part, 0 all zeros.  Proportional: the
    same array over AMP."""
    from mfea import loads
    if (name, tag) not in _loads:
        xyz, e2n, _, _ = mesh_of(name)
        fr = free_nodes(name)
        pick = fr[np.linspace(0, len(fr) - 1, 7).astype(int)[1:-1]] if len(fr) >= 7 else fr
        if tag == "P":
            f = loads.point(len(xyz), pick, PT_VEC3 if name == SIM3D else PT_VEC)
        elif tag == "S":
            f = loads.self_weight(xyz, e2n, SW, (0.0, -1.0, 0.0))
        elif tag == "Z":
            f = loads.point(len(xyz), pick, PT_VEC3)
        elif tag == "0":
            f = np.zeros((len(xyz), 3))
        _loads[name, tag] = f
    f = _loads[name, tag]
    return f / AMP if mode == PROP else f


def K_active(name, active):
    """The oracle's K of an activity other than all-active, once per mask."""
    key = (name, np.asarray(active, dtype=np.uint8).tobytes())
    if key not in _Kact:
        xyz, e2n, _, _ = mesh_of(name)
        _Kact[key] = fo.assemble_global_stiffness(xyz, e2n, np.asarray(active, dtype=bool)).tocsr()
    return _Kact[key]


def floating_nodes(name, active=None):
    """Free nodes whose component of the active element graph holds no grip node
    (a node with no active element is a component of its own)."""
    xyz, e2n, top, bot = mesh_of(name)
    n = len(xyz)
    on = np.ones(len(e2n), bool) if active is None else np.asarray(active, dtype=bool)
    G = sp.coo_matrix((np.ones(int(on.sum())), (e2n[on, 0], e2n[on, 1])), shape=(n, n))
    _, lab = connected_components(G, directed=False)
    grip = np.zeros(n, bool)
    grip[top] = grip[bot] = True
    anchored = np.zeros(lab.max() + 1, bool)
    anchored[lab[grip]] = True
    return ~anchored[lab] & ~grip


def check(name, f, mode, a_top, a_bot, *, active=None, K=None, field=None, cache=None):
    """The checker's solve.  Returns a dict: U (3N), A, rhs, free, q (N x 3, the
    effective load: scaled, zero on grips and floating nodes), fl (the floating
    mask)."""
    if cache is not None and cache in _ref:
        return _ref[cache]
    xyz, e2n, top, bot = mesh_of(name)
    if K is None:
        K = K_of(name) if active is None else K_active(name, active)
    if field is None:
        known, vals = fo.known_dof_map(top, bot, a_top, a_bot)
    else:
        known, vals = field_known_map(top, bot, a_top, a_bot, field)
    A, b, free = fo.free_system(K, known, vals)
    fl = floating_nodes(name, active)
    q = (np.float64(a_top) * f if mode == PROP else f.copy()) + 0.0
    q[fl] = 0.0
    q[top] = 0.0
    q[bot] = 0.0
    rhs = b + q.ravel()[free]
    U = np.zeros(3 * len(xyz))
    U[free] = spsolve(A.tocsc(), rhs)
    U[known] = vals
    out = dict(U=U, A=A, rhs=rhs, free=free, q=q, fl=fl, known=known, vals=vals, K=K)
    if cache is not None:
        _ref[cache] = out
    return out


def start(e, name, f=None, mode=DEAD, tag=None, props=None):
    xyz, e2n, top, bot = mesh_of(name)
    e.set_mesh(xyz, e2n)
    e.set_bc(top, bot)
    e.set_active(None)
    e.set_grip_motion(EY, EY)
    e.set_grip_field(None if tag is None else field_of(name, tag))
    if props is not None:
        e.set_element_props(**props)
    e.set_node_loads(f, mode)
    return xyz, e2n, top, bot


def grip_rows(U, top, bot):
    U3 = U.reshape(-1, 3)
    return U3[top].copy(), U3[bot].copy()


# ---------------------------------------------------------------------------
# 1. U against the checker: solve after assemble, two steps, both modes
# ---------------------------------------------------------------------------
PARITY = ([(PLANAR, s, pc, m) for s in ("P", "S") for pc in ALL_PC for m in (DEAD, PROP)] +
          [(SIM3D, "P", pc, DEAD) for pc in ALL_PC] + [(SIM3D, "S", pc, PROP) for pc in (GAMG, JACOBI)] +
          [(X, "P", pc, m) for pc in (GAMG, JACOBI) for m in (DEAD, PROP)])


def _parity(eng, mesh, pc, want, top, bot):
    """mfea_solve after mfea_assemble (the separate RHS kernel), then two steps
    (the assembly's fused RHS, then — K and the hierarchy kept — k_amg_start)."""
    eng.assemble()
    st = eng.solve(AMP, -AMP, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    print(f"  solve iters {st.iters} rel {rel(U, want):.3e}")
    assert rel(U, want) <= 1e-10, rel(U, want)
    rows = grip_rows(U, top, bot)
    for k in range(2):
        _, _, st = eng.step(AMP, -AMP, opts(pc), 1.0)
        assert st.status == 0
        U = eng.displacement()
        print(f"  step {k}: iters {st.iters} rel {rel(U, want):.3e}")
        assert rel(U, want) <= 1e-10, (k, rel(U, want))
        assert all(same_bits(a, b) for a, b in zip(grip_rows(U, top, bot), rows))
    return rows


@pytest.mark.parametrize("mesh,tag,pc,mode", PARITY)
def test_parity(eng, mesh, tag, pc, mode):
    f = loads_of(mesh, tag, mode)
    _, _, top, bot = start(eng, mesh, f, mode)
    got, m, is_set = eng.node_loads()
    assert is_set and m == mode and same_bits(got, f + 0.0)
    ref = check(mesh, f, mode, AMP, -AMP, cache=(mesh, tag, mode))
    assert not ref["fl"].any()
    # the load matters: the checker without it is far from the checker with it
    assert rel(check(mesh, loads_of(mesh, "0"), DEAD, AMP, -AMP, cache=(mesh, "0"))["U"], ref["U"]) > 1e-3
    print(f"{mesh} {tag} pc {pc} {mode}")
    rows = _parity(eng, mesh, pc, ref["U"], top, bot)
    # the grip rows: bit for bit what they are without loads
    eng.set_node_loads(None)
    _, _, st = eng.step(AMP, -AMP, opts(pc), 1.0)
    assert st.status == 0
    assert all(same_bits(a, b) for a, b in zip(grip_rows(eng.displacement(), top, bot), rows))


@pytest.mark.parametrize("pc,mode", [(GAMG, DEAD), (JACOBI, PROP)])
def test_parity_with_a_grip_field(eng, pc, mode):
    f = loads_of(PLANAR, "P", mode)
    _, _, top, bot = start(eng, PLANAR, f, mode, tag="R")
    ref = check(PLANAR, f, mode, AMP, -AMP, field=field_of(PLANAR, "R"))
    print(f"field R, P, pc {pc} {mode}")
    _parity(eng, PLANAR, pc, ref["U"], top, bot)


@pytest.mark.parametrize("pc,mode", [(GAMG, PROP), (ICC, DEAD)])
def test_parity_with_element_props(eng, pc, mode):
    xyz, e2n, top, bot = mesh_of(PLANAR)
    n = len(e2n)
    A, I, _ = recipe(n)  # noqa: E741
    f = loads_of(PLANAR, "S", mode)
    start(eng, PLANAR, f, mode, props=dict(A=A, I=I))
    K = het_K(xyz, e2n, np.ones(n, bool), fo.E_MOD, A, I).tocsr()
    ref = check(PLANAR, f, mode, AMP, -AMP, K=K)
    print(f"props, S, pc {pc} {mode}")
    _parity(eng, PLANAR, pc, ref["U"], top, bot)
    eng.set_element_props()


# ---------------------------------------------------------------------------
# 2. the zero-load identity: an all-zero array takes the load kernels and
#    gives the bits of a handle that never set loads
# ---------------------------------------------------------------------------
def _three_steps(e, pc, f):
    start(e, PLANAR, f)
    rows = []
    for d in (0.012, 0.024, -0.03):  # (the last: a negative top amplitude)
        force, n, st = e.step(d, -d, opts(pc, 1e-12), MAX_STRAIN)
        assert st.status == 0
        rows.append((force, n, st.iters, e.displacement(), e.stress(), e.active()))
    return rows


@pytest.mark.parametrize("mode", [DEAD, PROP])
@pytest.mark.parametrize("pc,graphs", [(GAMG, GRAPHS_ON), (GAMG, GRAPHS_OFF), (JACOBI, {}), (ICC, {})],
                         ids=["gamg_on", "gamg_off", "jacobi", "icc"])
def test_zero_load_identity(eng, pc, graphs, mode):
    n = len(mesh_of(PLANAR)[1])
    with eng.options(**graphs):
        plain = _three_steps(eng, pc, None)
        assert not eng.node_loads()[2]
        start(eng, PLANAR, loads_of(PLANAR, "0"), mode)
        zero = []
        for d in (0.012, 0.024, -0.03):
            force, na, st = eng.step(d, -d, opts(pc, 1e-12), MAX_STRAIN)
            assert st.status == 0
            zero.append((force, na, st.iters, eng.displacement(), eng.stress(), eng.active()))
        assert eng.node_loads()[2]  # an all-zero array counts as set
    assert plain[-1][1] < n  # elements failed on the way
    for k, (a, b) in enumerate(zip(zero, plain)):
        assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], k
        assert same_bits(a[3], b[3]) and same_bits(a[4], b[4]) and np.array_equal(a[5], b[5]), k


# ---------------------------------------------------------------------------
# 3. a dead load at zero amplitudes is a real solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI, SOR])
def test_dead_load_at_zero_amplitudes(eng, pc):
    f = loads_of(PLANAR, "S")
    start(eng, PLANAR, f)
    ref = check(PLANAR, f, DEAD, 0.0, 0.0, cache=(PLANAR, "S", "zero"))
    for k in range(2):  # (the second: a kept step)
        force, _, st = eng.step(0.0, 0.0, opts(pc), 1.0)
        assert st.status == 0 and st.iters > 0
        U = eng.displacement()
        bref = float(np.sqrt(np.sum(ref["rhs"].astype(np.longdouble) ** 2)))
        print(f"pc {pc} step {k}: iters {st.iters} rel {rel(U, ref['U']):.3e} bnorm {st.bnorm!r} ref {bref!r}")
        assert rel(U, ref["U"]) <= 1e-10
        assert np.array_equal(ref["rhs"], ref["q"].ravel()[ref["free"]])  # b is q_f: nothing else
        assert abs(st.bnorm - bref) <= gamma(len(ref["rhs"]) + 2) * bref
    # the proportional load at dy_top = 0 is no load: nothing to solve
    eng.set_node_loads(f, PROP)
    _, _, st = eng.step(0.0, 0.0, opts(pc), 1.0)
    assert st.status == 0 and st.iters == 0 and not eng.displacement().any()


# ---------------------------------------------------------------------------
# 4. floating pieces: the load is dropped, the piece stays at exactly zero
# ---------------------------------------------------------------------------
def chain_cut(name):
    """A free chain hanging off the network and the element that holds it: from
    a free node with one element, inwards over nodes with two, at most four
    nodes; cutting the element at the chain's inner end leaves the chain — its
    nodes still joined to each other — without a grip.  Returns (chain nodes,
    the element to cut)."""
    xyz, e2n, top, bot = mesh_of(name)
    n = len(xyz)
    grip = np.zeros(n, bool)
    grip[top] = grip[bot] = True
    inc = [[] for _ in range(n)]
    for e, (a, b) in enumerate(e2n):
        inc[a].append(e)
        inc[b].append(e)
    for leaf in np.flatnonzero(~grip):
        if len(inc[leaf]) != 1:
            continue
        chain, prev_e, cur = [int(leaf)], -1, int(leaf)
        while True:
            nxt_e = [e for e in inc[cur] if e != prev_e]
            if len(nxt_e) != 1:
                break
            e = nxt_e[0]
            other = int(e2n[e, 0] if e2n[e, 1] == cur else e2n[e, 1])
            if grip[other] or len(inc[other]) != 2 or len(chain) == 4:
                if len(chain) >= 3 and not grip[other]:
                    return np.array(chain), e
                break
            chain.append(other)
            prev_e, cur = e, other
    raise AssertionError("no free chain of three nodes on this mesh")


@pytest.mark.parametrize("mode", [DEAD, PROP])
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_floating_piece(eng, pc, mode):
    from mfea import loads
    xyz, e2n, top, bot = mesh_of(PLANAR)
    chain, cut = chain_cut(PLANAR)
    active = np.ones(len(e2n), np.uint8)
    active[cut] = 0
    fl = floating_nodes(PLANAR, active)
    assert fl[chain].all() and fl.sum() == len(chain)  # the checker finds the piece floating, and nothing else
    assert not floating_nodes(PLANAR).any()
    # the piece carries a load, and so does the rest
    f = loads_of(PLANAR, "P", mode) + loads.point(len(xyz), chain, np.array(PT_VEC) / (AMP if mode == PROP else 1))
    start(eng, PLANAR, f, mode)
    eng.set_active(active)
    assert np.array_equal(eng.floating(), fl)
    ref = check(PLANAR, f, mode, AMP, -AMP, active=active, cache=(PLANAR, "cut", mode))
    assert not ref["U"].reshape(-1, 3)[chain].any()
    eng.assemble()
    for k, go in enumerate((lambda: eng.solve(AMP, -AMP, opts(pc)), lambda: eng.step(AMP, -AMP, opts(pc), 1.0)[2],
                            lambda: eng.step(AMP, -AMP, opts(pc), 1.0)[2])):
        st = go()
        assert st.status == 0
        U = eng.displacement()
        piece = U.reshape(-1, 3)[chain]
        print(f"pc {pc} {mode} call {k}: iters {st.iters} rel {rel(U, ref['U']):.3e} max |U| on the piece "
              f"{np.abs(piece).max():.3e}")
        assert not piece.any() and not np.signbit(piece).any()
        assert rel(U, ref["U"]) <= 1e-10
    # joined again: the load is back
    eng.set_active(None)
    _, _, st = eng.step(AMP, -AMP, opts(pc), 1.0)
    assert st.status == 0
    whole = check(PLANAR, f, mode, AMP, -AMP, cache=(PLANAR, "cut-whole", mode))
    assert rel(eng.displacement(), whole["U"]) <= 1e-10
    assert eng.displacement().reshape(-1, 3)[chain].any()


@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_failures_detach_a_loaded_piece_mid_run(eng, pc):
    """The element that holds a loaded chain is given a failure strain of 1e-12
    (every other element one of 1): it fails in the post of the first step, so
    from the second step on the chain floats.  mfea_run must equal the step
    loop bit for bit, every step must match the checker on the activity its K
    was assembled from, and the chain must be at exactly zero afterwards."""
    from mfea import loads
    xyz, e2n, top, bot = mesh_of(PLANAR)
    chain, cut = chain_cut(PLANAR)
    strength = np.ones(len(e2n))
    strength[cut] = 1e-12
    f = loads_of(PLANAR, "S") + loads.point(len(xyz), chain, PT_VEC)
    dys = np.array([0.01, 0.02, 0.03])
    start(eng, PLANAR, f, props=dict(max_strain=strength))
    loop = []
    for d in dys:
        force, na, st = eng.step(d, -d, opts(pc), 1.0)
        assert st.status == 0
        loop.append((force, na, st.iters, eng.displacement(), eng.stress(), eng.active()))
    cut_mask = np.ones(len(e2n), bool)
    cut_mask[cut] = False
    for k, row in enumerate(loop):
        assert np.array_equal(row[5], cut_mask), k  # that element failed in step 0, and nothing else
        ref = check(PLANAR, f, DEAD, dys[k], -dys[k], active=None if k == 0 else cut_mask)
        piece = row[3].reshape(-1, 3)[chain]
        print(f"pc {pc} step {k}: iters {row[2]} rel {rel(row[3], ref['U']):.3e} max |U| on the chain "
              f"{np.abs(piece).max():.3e}")
        assert rel(row[3], ref["U"]) <= 1e-10, k
        assert piece.any() if k == 0 else not piece.any(), k
    start(eng, PLANAR, f, props=dict(max_strain=strength))
    run = eng.run(dys, -dys, opts(pc), 1.0)
    assert run["n_done"] == len(dys)
    for k, row in enumerate(loop):
        assert same_bits(run["force"][k], row[0]) and run["n_active"][k] == row[1], k
        assert run["stats"][k]["iters"] == row[2], k
        assert same_bits(run["U"][k], row[3]) and same_bits(run["stress"][k], row[4]), k
        assert np.array_equal(run["active"][k], row[5]), k
    eng.set_element_props()


# ---------------------------------------------------------------------------
# 5. proportional mode: U scales with the amplitudes, events stand; dead mode
#    refuses events
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_proportional_scaling(eng, pc):
    """Both solves lie within 1e-10 of their exact solutions, which are exactly
    a factor 2 apart, so they lie within 2e-10 of each other."""
    f = loads_of(PLANAR, "S", PROP)
    start(eng, PLANAR, f, PROP)
    a, b = 0.02, -0.015
    _, _, st = eng.step(a, b, opts(pc), 1.0)
    assert st.status == 0
    U1 = eng.displacement()
    _, _, st = eng.step(2 * a, 2 * b, opts(pc), 1.0)
    assert st.status == 0
    U2 = eng.displacement()
    assert rel(U1, check(PLANAR, f, PROP, a, b)["U"]) <= 1e-10
    print(f"pc {pc}: |U(2a,2b) - 2 U(a,b)| / |2 U| = {rel(U2, 2 * U1):.3e}")
    assert rel(U2, 2.0 * U1) <= 2e-10


@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_events_proportional(eng, pc):
    from mfea import EVENTS_COMPLETE
    dref, tie, lam_max, n_events = 0.02, 1e-9, np.inf, 3
    xyz, e2n, _, _ = mesh_of(PLANAR)
    f = loads_of(PLANAR, "S", PROP) * (AMP / dref)  # (the load of S at the reference amplitude)
    eps0 = np.abs(fo.element_strain(xyz, e2n, check(PLANAR, f, PROP, dref, -dref, cache=(PLANAR, "ev"))["U"]))
    max_strain = 0.5 * float(np.nanmax(eps0))
    start(eng, PLANAR, f, PROP)
    rec = {k: [] for k in ("lam", "force1", "U1", "stress", "active", "n_failed")}
    for k in range(n_events):
        act0 = eng.active()
        lam, f1, nf, na, st = eng.event(dref, -dref, opts(pc), max_strain, tie, lam_max)
        assert st.status == 0
        U1, stress, act1 = eng.displacement(), eng.stress(), eng.active()
        if k == 0:
            assert rel(U1, _ref[PLANAR, "ev"]["U"]) <= 1e-10
        _, lam_np, group, stress_np = rule(fo.element_strain(xyz, e2n, U1), act0, max_strain, tie, lam_max)
        assert same_bits(lam, lam_np), (k, lam, lam_np)
        assert nf == int(group.sum()) > 0 and na == int(act1.sum()), k
        assert np.array_equal(act1, act0 & ~group), k
        assert same_bits(stress, stress_np), k
        assert same_bits(f1, eng.post(np.inf)[0]), k
        for key, v in zip(rec, (lam, f1, U1, stress, act1, nf)):
            rec[key].append(v)
    assert 0.4 < rec["lam"][0] < 0.6
    start(eng, PLANAR, f, PROP)
    run = eng.run_events(dref, -dref, opts(pc), max_strain, tie, lam_max, n_events=n_events)
    assert run["n_done"] == n_events and run["stop_reason"] == EVENTS_COMPLETE
    assert same_bits(run["lam"], rec["lam"]) and same_bits(run["force1"], rec["force1"])
    assert same_bits(run["stress"], rec["stress"]) and np.array_equal(run["active"], rec["active"])
    assert same_bits(run["U"], np.asarray(rec["lam"])[:, None] * np.asarray(rec["U1"]))
    assert np.array_equal(run["n_failed"], rec["n_failed"])


def test_dead_mode_refuses_events(eng):
    from mfea import MfeaError
    from mfea._capi import ESTATE
    f = loads_of(PLANAR, "P")
    start(eng, PLANAR, f)
    for call in (lambda: eng.event(0.02, -0.02, opts(GAMG), MAX_STRAIN, 1e-9, np.inf),
                 lambda: eng.run_events(0.02, -0.02, opts(GAMG), MAX_STRAIN, 1e-9, np.inf, n_events=2)):
        with pytest.raises(MfeaError) as err:
            call()
        assert err.value.code == ESTATE and "affine" in str(err.value)
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)  # the handle still steps
    assert st.status == 0
    assert rel(eng.displacement(), check(PLANAR, f, DEAD, AMP, -AMP, cache=(PLANAR, "P", DEAD))["U"]) <= 1e-10
    eng.set_node_loads(None)  # cleared: events run again
    lam, _, nf, _, st = eng.event(0.02, -0.02, opts(GAMG), MAX_STRAIN, 1e-9, np.inf)
    assert st.status == 0 and nf > 0 and lam > 0


# ---------------------------------------------------------------------------
# 6. the work of the loads, and the work identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,tag,mode,cut", [(PLANAR, "S", DEAD, False), (PLANAR, "P", PROP, True),
                                              (SIM3D, "P", DEAD, False), (SIM3D, "S", PROP, False),
                                              (X, "P", DEAD, False)])
def test_load_work(eng, mesh, tag, mode, cut):
    from mfea import loads
    xyz, e2n, top, bot = mesh_of(mesh)
    f = loads_of(mesh, tag, mode)
    active = None
    if cut:  # a loaded floating piece: its rows do not count
        chain, ce = chain_cut(mesh)
        active = np.ones(len(e2n), np.uint8)
        active[ce] = 0
        f = f + loads.point(len(xyz), chain, np.array(PT_VEC) / AMP)
    start(eng, mesh, f, mode)
    if cut:
        eng.set_active(active)
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    U = eng.displacement()
    L = eng.load_work()
    ref = check(mesh, f, mode, AMP, -AMP, active=active)
    q, free = ref["q"].ravel(), ref["free"]
    # the dot-product bound of the checker's extended-precision sum
    Lref = float(np.sum(q[free].astype(np.longdouble) * U[free].astype(np.longdouble)))
    bound = gamma(len(free) + 1) * float(np.abs(q[free]) @ np.abs(U[free]))
    print(f"{mesh} {tag} {mode}: L {L!r} ref {Lref!r} err {abs(L - Lref):.3e} bound {bound:.3e}")
    assert L != 0.0 and abs(L - Lref) <= bound
    assert same_bits(L, eng.load_work())  # reproducible
    # the work identity: gap = u_fᵀ(KU)_f from the oracle's K and the device's U
    K, A = ref["K"], ref["A"]
    uf = U[free]
    KU = K @ U
    gap = float(uf @ KU[free])
    reg_term = fo.REG * float(uf @ uf)
    resid = float(np.linalg.norm(ref["rhs"] - A @ uf))
    nrow = int(np.diff(K.indptr).max())
    rounding = gamma(len(free) + nrow + 4) * (float(np.abs(uf) @ (abs(K) @ np.abs(U))[free]) +
                                              float(np.abs(q[free]) @ np.abs(uf)) + reg_term)
    lhs, rhs_ = abs(gap - L + reg_term), float(np.linalg.norm(uf)) * resid + rounding
    print(f"  gap {gap!r}, |gap - L + reg|u|^2| {lhs:.3e} <= |u||r| {float(np.linalg.norm(uf)) * resid:.3e} "
          f"+ rounding {rounding:.3e}")
    assert lhs <= rhs_
    # 2W = dy_top·G_top + dy_bot·G_bot + L up to those terms (on the activity of K)
    en = eng.energy(elements=False, active=active)
    g_top, g_bot = eng.grip_work()
    W2 = 2.0 * (en["axial"] + en["bending"])
    scale = float(np.abs(U) @ (abs(K) @ np.abs(U)))
    print(f"  2W {W2!r}, 2W - (grips + L) {W2 - (AMP * g_top - AMP * g_bot + L):.3e}")
    assert abs(W2 - (AMP * g_top - AMP * g_bot + L)) <= rhs_ + reg_term + 1e-12 * scale
    eng.set_node_loads(None)
    assert eng.load_work() == 0.0


# ---------------------------------------------------------------------------
# 7. changes between steps, every graph option on: nothing stale, everything kept
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("phase_times", [0, 1])
def test_change_between_steps(eng, phase_times):
    from mfea import Engine
    d = 0.01
    P, S = loads_of(PLANAR, "P"), loads_of(PLANAR, "S")
    seq = [(P, DEAD), (S, DEAD), (S / d, PROP), (None, DEAD)]
    with eng.options(**GRAPHS_ON, phase_times=phase_times):
        start(eng, PLANAR)
        for _ in range(2):  # (the second replays what the first captured / kept)
            _, _, st = eng.step(d, -d, opts(GAMG), 1.0)
            assert st.status == 0
        for f, mode in seq:
            kept = eng.get_option("op_kept_steps"), eng.get_option("amg_setup_kept")
            eng.set_node_loads(f, mode)
            want = check(PLANAR, np.zeros_like(P) if f is None else f, mode, d, -d)["U"]
            for k in range(2):
                force, _, st = eng.step(d, -d, opts(GAMG), 1.0)
                assert st.status == 0 and st.amg_rebuilt == 0
                U = eng.displacement()
                assert rel(U, want) <= 1e-10, (mode, k, rel(U, want))
                # a kept step: no assembly, no numeric setup
                assert eng.get_option("op_kept_steps") == kept[0] + k + 1
                assert eng.get_option("amg_setup_kept") == kept[1] + k + 1
                if phase_times:
                    assert st.t_setup_ms == 0
            # the same bytes and mode again drop nothing: a kept step with the same bits
            eng.set_node_loads(None if f is None else f.copy(), mode)
            force2, _, st2 = eng.step(d, -d, opts(GAMG), 1.0)
            assert st2.status == 0 and st2.amg_rebuilt == 0 and st2.iters == st.iters
            assert same_bits(eng.displacement(), U) and same_bits(force2, force)
            assert eng.get_option("op_kept_steps") == kept[0] + 3
        # the last step after clearing: the bits of a fresh handle
        with Engine(0) as fresh:
            fresh.set_option("amg_rebuild_rent", 0)
            with fresh.options(**GRAPHS_ON, phase_times=phase_times):
                start(fresh, PLANAR)
                for _ in range(2):
                    f0, _, st0 = fresh.step(d, -d, opts(GAMG), 1.0)
                assert st0.status == 0 and st0.iters == st2.iters
                assert same_bits(eng.displacement(), fresh.displacement()) and same_bits(force2, f0)


# ---------------------------------------------------------------------------
# 8. z loads on a planar mesh: 3 DOFs per node, and back
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [GAMG, JACOBI])
def test_planar_z(eng, pc):
    from mfea import Engine
    f = loads_of(PLANAR, "P")
    start(eng, PLANAR, f)
    assert eng.info()["planar"] == 1
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2  # every z entry zero: the 2-DOF lanes
    fz = loads_of(PLANAR, "Z")
    eng.set_node_loads(fz)
    eng.assemble()
    st = eng.solve(AMP, -AMP, opts(pc))
    assert st.status == 0
    U = eng.displacement()
    want = check(PLANAR, fz, DEAD, AMP, -AMP)["U"]
    print(f"planar z pc {pc}: iters {st.iters} rel {rel(U, want):.3e}")
    assert rel(U, want) <= 1e-10
    assert np.any(U.reshape(-1, 3)[:, 2] != 0.0)
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 3
    # every z entry zero again: back to 2; then cleared: the bits of a fresh handle
    eng.set_node_loads(f)
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2
    eng.set_node_loads(fz)
    eng.set_node_loads(None)
    eng.assemble()
    assert eng.solve(AMP, -AMP, opts(pc)).status == 0
    if pc == GAMG:
        assert eng.amg_info()["nd"] == 2
    U2 = eng.displacement()
    with Engine(0) as fresh:
        fresh.set_option("amg_rebuild_rent", 0)
        start(fresh, PLANAR)
        fresh.assemble()
        assert fresh.solve(AMP, -AMP, opts(pc)).status == 0
        assert same_bits(U2, fresh.displacement())
    assert not np.any(U2.reshape(-1, 3)[:, 2])


# ---------------------------------------------------------------------------
# 9. lifetime and errors
# ---------------------------------------------------------------------------
def test_lifetime(eng):
    xyz, e2n, top, bot = mesh_of(SIM3D)
    f = loads_of(SIM3D, "S")
    start(eng, SIM3D, f)
    # other bands: the stored loads are gathered again for the new free rows
    top2, bot2 = fo.grip_nodes(xyz, np.arange(len(xyz)), 1.4 * GRIP[SIM3D])
    assert len(top2) > len(top) and len(bot2) > len(bot) and not set(top2) & set(bot2)
    eng.set_bc(top2, bot2)
    eng.set_active(None)
    got, mode, is_set = eng.node_loads()
    assert is_set and mode == DEAD and same_bits(got, f + 0.0)
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    known, vals = fo.known_dof_map(top2, bot2, AMP, -AMP)
    A, b, free = fo.free_system(K_of(SIM3D), known, vals)
    q = f.copy()
    q[top2] = 0.0
    q[bot2] = 0.0
    want = np.zeros(3 * len(xyz))
    want[free] = spsolve(A.tocsc(), b + q.ravel()[free])
    want[known] = vals
    assert rel(eng.displacement(), want) <= 1e-10
    # the other setters keep them
    eng.set_bc(top, bot)
    eng.set_active(np.ones(len(e2n), dtype=np.uint8))
    eng.set_material(fo.E_MOD, fo.AREA, fo.INERTIA)
    eng.set_element_props(A=np.full(len(e2n), fo.AREA))
    eng.set_element_props()
    eng.set_grip_motion((1.0, 0.0, 0.0), EY)
    eng.set_grip_motion(EY, EY)
    eng.set_grip_field(field_of(SIM3D, "A"))
    eng.set_grip_field(None)
    got, mode, is_set = eng.node_loads()
    assert is_set and mode == DEAD and same_bits(got, f + 0.0)
    _, _, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
    assert st.status == 0
    assert rel(eng.displacement(), check(SIM3D, f, DEAD, AMP, -AMP)["U"]) <= 1e-10
    # -0 is stored as 0
    z = f.copy()
    z[free_nodes(SIM3D)[0]] = (-0.0, 0.0, -0.0)
    eng.set_node_loads(z, PROP)
    got, mode, is_set = eng.node_loads()
    assert is_set and mode == PROP and not np.signbit(got[free_nodes(SIM3D)[0]]).any()
    # mfea_set_mesh clears them
    eng.set_mesh(xyz, e2n)
    eng.set_bc(top, bot)
    got, mode, is_set = eng.node_loads()
    assert not is_set and mode == DEAD and not got.any()


def test_errors():
    from mfea import Engine, MfeaError
    from mfea._capi import EINVAL, ESTATE, _lib, _ptr
    xyz, e2n, top, bot = mesh_of(X)
    f = loads_of(X, "P")
    with Engine(0) as e:
        with pytest.raises(MfeaError) as err:  # before a mesh
            e.set_node_loads(f)
        assert err.value.code == ESTATE
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_node_loads(f, PROP)
        for bad in (np.nan, np.inf, -np.inf):
            g = f.copy()
            g[top[0], 1] = bad  # (a grip node's row is checked too)
            with pytest.raises(MfeaError) as err:
                e.set_node_loads(g)
            assert err.value.code == EINVAL
            got, mode, is_set = e.node_loads()  # the handle is unchanged
            assert is_set and mode == PROP and same_bits(got, f + 0.0)
        for bad_mode in (2, -1):
            assert _lib.mfea_set_node_loads(e._h, _ptr(np.ascontiguousarray(f)), bad_mode) == EINVAL
            got, mode, is_set = e.node_loads()
            assert is_set and mode == PROP and same_bits(got, f + 0.0)
        with pytest.raises(ValueError):
            e.set_node_loads(f, "follower")
        with pytest.raises(ValueError):
            e.set_node_loads(f[:-1])
        # the getter accepts NULL for every argument
        assert _lib.mfea_get_node_loads(e._h, None, None, None) == 0
        assert _lib.mfea_get_load_work(e._h, None) == EINVAL
        with pytest.raises(MfeaError) as err:  # no assembly yet: as mfea_get_reaction
            e.load_work()
        assert err.value.code == ESTATE
        _, _, st = e.step(0.01, -0.01, opts(JACOBI), 1.0)
        assert st.status == 0 and e.load_work() != 0.0
        # loads, then partitions: MFEA_ESTATE at the next build
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.assemble()
        assert err.value.code == ESTATE
    with Engine(0) as e:  # partitions first: the setter refuses
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_parts(2)
        with pytest.raises(MfeaError) as err:
            e.set_node_loads(f)
        assert err.value.code == ESTATE
        assert not e.node_loads()[2]
        e.set_active(None)
        e.assemble()  # no loads: the partitioned handle builds and runs
        assert e.solve(0.01, -0.01, opts(JACOBI)).status == 0


# ---------------------------------------------------------------------------
# 10. the drop-in solver
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
    lmode = PROP if mode == "events" else DEAD
    dmax, steps = 0.004, 3
    f = loads_of(X, "P") * (0.1 / dmax if lmode == PROP else 0.1)
    csv = str(tmp_path / "loads.csv")
    with open(csv, "w") as fh:  # the loaded nodes alone
        fh.write("node_id,fx,fy,fz\n")
        for n in np.flatnonzero(f.any(axis=1)):
            fh.write(f"{n},{float(f[n, 0])!r},{float(f[n, 1])!r},{float(f[n, 2])!r}\n")
    try:
        fs.main([dirn, "--node-loads", csv, "--load-mode", lmode, "--grip-length", str(GRIP[X]), "--n-steps",
                 str(steps), "--disp-max", str(dmax)] +
                {"loop": [], "device_run": ["--device-run"], "events": ["--events"]}[mode])
    finally:  # (main sets the module's constants)
        fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG = 40, 0.02, 0.018, 1e-12
    out = os.path.join(dirn, "fea_results")
    for name in ("stress_record.csv", "active_elements.csv", "node_displacements.csv", "force_displacement.csv"):
        assert os.path.exists(os.path.join(out, name)), name
    last = pd.read_csv(os.path.join(out, "node_displacements.csv"),
                       float_precision="round_trip").values[-1, :-1].astype(np.float64)  # (the step column is last)
    got, m, is_set = fs.get_engine().node_loads()
    assert is_set and m == lmode and same_bits(got, f + 0.0)
    with Engine(0) as e:
        e.set_mesh(xyz, e2n)
        e.set_bc(top, bot)
        e.set_active(None)
        e.set_node_loads(f, lmode)
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
    if mode == "loop":  # ... and the checker's solve of the last step
        assert rel(last, check(X, f, DEAD, dmax, -dmax)["U"]) <= 1e-10
    fs.get_engine().set_node_loads(None)
