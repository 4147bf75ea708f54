"""Level 0's sorting window (AmgLayout::l0_window) and the block halo plan
(AmgFusePlan) of csrc/amg_symbolic.cpp, no GPU: the window only permutes rows
inside its windows, the halo plan covers every A_0 column of every block, and
its per-block restatement — u over own + halo rows, then w from the local u
through the local columns — is the global up sweep followed by A_0 u
(amg.hip k_amg_up_w)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import amg_ref
import fea_oracle as fo
from conftest import PKG, REPO, load_mesh
from test_amg_cpu import _golden22k, setup_case

P = C.c_void_p
B = 1408  # capi.hip kAmgFuseWindow


def _build_fuse_shim():
    d = os.path.join(REPO, "tests", "native")
    out = os.path.join(d, "libfuseshim.so")
    srcs = [os.path.join(d, "fuse_shim.cpp")] + [os.path.join(PKG, "csrc", f) for f in (
        "symbolic.cpp", "partition.cpp", "amg_symbolic.cpp", "amg_dist.cpp", "amg_collapse.cpp")]
    deps = srcs + glob.glob(os.path.join(PKG, "csrc", "*.hpp")) + [os.path.join(d, "host_shim.cpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(PKG, "csrc"),
                               "-I" + d, *srcs, "-o", out])
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_build_fuse_shim())
    lib.shim_build.restype = C.c_int
    lib.shim_build.argtypes = [C.c_int64, P, C.c_int64, P, C.c_int, C.c_int64, P, C.c_int64, P,
                               C.c_int, P, C.c_char_p, C.c_int]
    lib.shim_arrays.argtypes = [P] * 6
    lib.shim_sell_values.argtypes = [P, C.c_double, C.c_double, P, P]
    lib.shim_amg.restype = C.c_int
    lib.shim_amg.argtypes = [P, C.c_int, C.c_char_p, C.c_int]
    lib.shim_amg_array.restype = C.c_int64
    lib.shim_amg_array.argtypes = [C.c_int, C.c_char_p, P]
    lib.shim_amg_array_more.restype = C.c_int64
    lib.shim_amg_array_more.argtypes = [C.c_int, C.c_char_p, P]
    lib.shim_amg_l0_window.argtypes = [C.c_int64]
    lib.shim_amg_l0_window_used.restype = C.c_int64
    lib.shim_fuse.restype = C.c_int
    lib.shim_fuse.argtypes = [C.c_int64, P, C.c_char_p, C.c_int]
    lib.shim_fuse_array.restype = C.c_int64
    lib.shim_fuse_array.argtypes = [C.c_char_p, P]
    lib.shim_amg_layout_by_a(1)  # the compact cycle's labels, as the engine builds them
    yield lib
    lib.shim_amg_l0_window(4096)


def _ptr(a):
    return a.ctypes.data_as(P)


def _mesh3d():
    nodes, elems = load_mesh("sim_20251115_135507")
    xyz = nodes[["x", "y", "z"]].values
    top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, 0.5)
    return xyz, elems[["n1", "n2"]].values, top, bot


def _tiles_1x5():
    from mfea import synth
    xyz, e2n = synth.tiled_mesh(1, 5)
    top, bot = synth.grips(xyz)
    return xyz, e2n, top, bot


_MORE = ("nat", "A.rlen", "P.rlen", "R.rlen", "AP.rlen", "PT.rlen", "RT.rlen")


def _plan(shim, mesh, nd, window=None):
    """pattern + plan at the window (None: the layout's default, untouched);
    the per-level arrays of amg_ref.fetch_plan plus the row lengths and nat."""
    xyz, e2n, top, bot = (np.ascontiguousarray(a, t) for a, t in zip(mesh, (np.float64,) + (np.int64,) * 3))
    sizes = np.zeros(5, np.int64)
    err = C.create_string_buffer(256)
    assert shim.shim_build(len(xyz), _ptr(xyz), len(e2n), _ptr(e2n), 0, len(top), _ptr(top), len(bot), _ptr(bot),
                           -1, _ptr(sizes), err, 256) == 0, err.value
    if window is not None:
        shim.shim_amg_l0_window(window)
    levels = amg_ref.fetch_plan(shim, np.ones(len(e2n), np.uint8), nd)
    for l, L in enumerate(levels):
        for name in _MORE:
            n = shim.shim_amg_array_more(l, name.encode(), None)
            L[name] = np.zeros(max(n, 0), np.int32)
            if n > 0:
                shim.shim_amg_array_more(l, name.encode(), _ptr(L[name]))
    return levels


def _fuse(shim, cap=1 << 20):
    info = np.zeros(5, np.int64)
    why = C.create_string_buffer(256)
    on = shim.shim_fuse(cap, _ptr(info), why, 256)
    assert on >= 0, why.value
    out = {"on": on, "why": why.value.decode(), "B": int(info[0]), "n_blocks": int(info[1]),
           "max_halo": int(info[2]), "cut": int(info[3]), "offdiag": int(info[4])}
    for name in ("hptr", "hrow", "hpt", "lcol"):
        n = shim.shim_fuse_array(name.encode(), None)
        out[name] = np.zeros(max(n, 0), np.int32)
        if n > 0:
            shim.shim_fuse_array(name.encode(), _ptr(out[name]))
    return out


def _same_plan(a, b):
    assert len(a) == len(b)
    for l, (La, Lb) in enumerate(zip(a, b)):
        assert La.keys() == Lb.keys()
        for k in La:
            assert np.array_equal(La[k], Lb[k]), (l, k)


@pytest.mark.parametrize("mesh,nd", [(_golden22k, 2), (_mesh3d, 3)], ids=["golden22k", "mesh3d"])
def test_window_4096_is_the_default_plan(shim, mesh, nd):
    m = mesh()
    shim.shim_amg_l0_window(4096)
    default = _plan(shim, m, nd)              # AmgLayout's own default
    assert shim.shim_amg_l0_window_used() == 4096
    _same_plan(default, _plan(shim, m, nd, 4096))
    other = _plan(shim, m, nd, 1408)          # (the option does reach the labels)
    assert shim.shim_amg_l0_window_used() == 1408
    if default[0]["n"] > 1408:
        assert not np.array_equal(default[0]["nat"], other[0]["nat"])
    # the coarse levels keep their 4096-row windows: same rows, same lengths
    for La, Lb in zip(default[1:], other[1:]):
        assert np.array_equal(La["nat"], Lb["nat"]) and np.array_equal(La["A.rlen"], Lb["A.rlen"])


@pytest.mark.parametrize("window", [1408, 704])
def test_window_permutes_inside_windows_only(shim, window):
    levels = _plan(shim, _golden22k(), 2, window)
    L, L1 = levels[0], levels[1]
    n, nc = L["n"], L["nc"]
    assert n > 2 * window
    # each labelling as row → natural (aggregation-order) index: A_0's rows,
    # P̃_0's rows (pt_row names the level-0 row), R̂_0's rows (rt_row names the
    # level-1 row, whose own labels keep their 4096-row windows)
    for name, rows, length, nat in (("nat", n, "A.rlen", L["nat"]), ("pt_row", n, "PT.rlen", L["nat"][L["pt_row"]]),
                                    ("rt_row", nc, "RT.rlen", L1["nat"][L["rt_row"]])):
        assert len(nat) == rows
        for w0 in range(0, rows, window):
            w1 = min(rows, w0 + window)
            # a permutation inside the window: across windows the natural order is kept
            assert np.array_equal(np.sort(nat[w0:w1]), np.arange(w0, w1)), (name, w0)
            # … by descending length, ties in natural order
            ln = L[length][w0:w1]
            assert np.all(np.diff(ln) <= 0), (name, w0)
            for v in np.unique(ln):
                assert np.all(np.diff(nat[w0:w1][ln == v]) > 0), (name, w0, v)
            # P̃_0's windows hold the level-0 rows of A_0's windows: a block's rows stay its own
            if name == "pt_row":
                assert np.array_equal(np.sort(L["pt_row"][w0:w1]), np.arange(w0, w1)), w0
    # pt_row and rt_row are still the inverses of their labellings: bijections
    for lab, rows in ((L["pt_row"], n), (L["rt_row"], nc)):
        assert np.array_equal(np.sort(lab), np.arange(rows))


def _check_halo_plan(L, F):
    n, Bk = L["n"], F["B"]
    row, k = amg_ref.pos_rows(L["A.sptr"], n)
    col, lcol = L["A.col"], F["lcol"]
    valid = (col >= 0) & (row >= 0)
    assert len(lcol) == len(col)
    assert np.all(lcol[~valid] == 0xFFFF)
    assert F["n_blocks"] == -(-n // Bk) and len(F["hptr"]) == F["n_blocks"] + 1
    inv_pt = np.empty(n, np.int64)
    inv_pt[L["pt_row"]] = np.arange(n)
    worst = 0
    for b in range(F["n_blocks"]):
        lo, hi = b * Bk, min(n, (b + 1) * Bk)
        halo = F["hrow"][F["hptr"][b]:F["hptr"][b + 1]]
        worst = max(worst, len(halo))
        # sorted, unique, disjoint from the own range
        assert np.all(np.diff(halo) > 0)
        assert np.all((halo < lo) | (halo >= hi))
        # each halo row's P̃_0 row maps back to it
        hpt = F["hpt"][F["hptr"][b]:F["hptr"][b + 1]]
        assert np.array_equal(L["pt_row"][hpt], halo)
        assert np.array_equal(hpt, inv_pt[halo])
        # every column of the block's rows is an own row or a halo row, and
        # decoding the local column gives it back
        m = valid & (row >= lo) & (row < hi)
        lc = lcol[m].astype(np.int64)
        assert np.all(lc < Bk + len(halo))
        local = np.concatenate([np.arange(lo, lo + Bk), halo])
        assert np.array_equal(local[lc], col[m])
        own = (col[m] >= lo) & (col[m] < hi)
        assert np.all(lc[own] < Bk) and np.all(lc[~own] >= Bk)
        # nothing in the list that no row references
        assert np.array_equal(np.unique(col[m][~own]), halo)
    assert worst == F["max_halo"]


@pytest.mark.parametrize("mesh", [_golden22k, _tiles_1x5], ids=["golden22k", "tiles1x5"])
def test_halo_plan_covers_every_column(shim, mesh):
    L = _plan(shim, mesh(), 2, B)[0]
    F = _fuse(shim)
    assert F["on"] == 1, F["why"]
    assert F["B"] == B
    _check_halo_plan(L, F)


def test_halo_over_capacity_turns_the_fusion_off(shim):
    _plan(shim, _golden22k(), 2, B)
    F = _fuse(shim, cap=1)
    assert F["on"] == 0 and "capacity" in F["why"]
    assert F["max_halo"] > 1
    assert len(F["lcol"]) == 0 and len(F["hrow"]) == 0  # nothing a kernel could run on
    assert _fuse(shim)["on"] == 1
    # a window the P̃_0 labelling does not share is no block plan either
    _plan(shim, _golden22k(), 2, 4096)
    assert _fuse(shim)["B"] == 4096


def test_block_restatement_equals_up_then_spmv(shim):
    xyz, e2n, top, bot = _golden22k()
    shim.shim_amg_l0_window(B)
    levels, _, _, _ = setup_case(shim, xyz, e2n, top, bot, np.ones(len(e2n)), 2)
    assert shim.shim_amg_l0_window_used() == B
    F = _fuse(shim)
    assert F["on"] == 1
    amg_ref.compact_transfers(levels)
    L, nd = levels[0], 2
    n = L["n"]
    rng = np.random.default_rng(11)
    c = rng.standard_normal(n * nd)
    e1 = rng.standard_normal(L["nc"] * nd)
    u = c + L["Pt"] @ e1                       # the global up sweep
    w = L["A"] @ u                             # … followed by A_0 u
    row, _ = amg_ref.pos_rows(L["A.sptr"], n)
    Pt = L["Pt"].tocsr()
    wb = np.zeros_like(w)
    for b in range(F["n_blocks"]):
        lo, hi = b * B, min(n, (b + 1) * B)
        halo = F["hrow"][F["hptr"][b]:F["hptr"][b + 1]].astype(np.int64)
        ul = np.zeros((B + len(halo), nd))     # the block's LDS: own rows, then the halo
        for rows, at in ((np.arange(lo, hi), 0), (halo, B)):
            dofs = (rows[:, None] * nd + np.arange(nd)).ravel()
            ul[at:at + len(rows)] = (c[dofs] + Pt[dofs] @ e1).reshape(-1, nd)
        q = np.flatnonzero((row >= lo) & (row < hi) & (L["A.col"] >= 0))
        contrib = np.einsum("pab,pb->pa", L["Ab"][q], ul[F["lcol"][q]])
        acc = np.zeros((n, nd))
        np.add.at(acc, row[q], contrib)
        wb[lo * nd:hi * nd] = acc[lo:hi].ravel()
    assert np.linalg.norm(wb - w) <= 1e-12 * np.linalg.norm(w)


def test_depth_first_order_keeps_couplings_inside_blocks(shim):
    """The 1×5-tile network (C2) in 1408-row blocks: couplings that leave their
    block, and halo rows per own row.  Measured when this test was written:
    cut 0.0182 of the off-diagonal couplings, halo / own 0.0254 (largest halo
    79 rows); twice that would be a regression of the level-0 order."""
    L = _plan(shim, _tiles_1x5(), 2, B)[0]
    F = _fuse(shim)
    assert F["on"] == 1
    cut = F["cut"] / F["offdiag"]
    halo = len(F["hrow"]) / L["n"]
    print(f"C2 at B={B}: rows {L['n']}, cut {cut:.4f}, halo/own {halo:.4f}, max halo {F['max_halo']}")
    assert cut <= 2 * 0.0182
    assert halo <= 2 * 0.0254
