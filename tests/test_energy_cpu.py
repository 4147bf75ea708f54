"""Strain energy per element (mfea_get_energy), the parts that need no GPU.

csrc/energy.hpp is run on the host through tests/native/energy_main.cpp, a
program of its own under the address and undefined-behaviour sanitizers, and
held against the NumPy restatement of include/mfea.h's operation table
(tests/energy_ref.py).  The restatement itself is held against ½ UᵀKU on the
oracle's heterogeneous K and direct solve, the work identity and central
differences of the equilibrium energy."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import energy_ref as er
from conftest import REPO

import fea_oracle as fo  # noqa: E402  (checker only)
from test_gpu_props import het_K  # noqa: E402

SYMBOL = "mfea_get_energy"
ULP = 2.0 ** -52


def test_symbol_methods_and_abi():
    import mfea
    from mfea import _capi
    assert mfea.abi_version() == 8
    assert SYMBOL in _capi.EXPORTED and hasattr(_capi._lib, SYMBOL)
    for method in ("energy", "energy_gradient"):
        assert callable(getattr(mfea.Engine, method))
    assert [f for f, _ in _capi.ElementEnergy._fields_] == ["w_axial", "w_bending", "g_axial", "g_bending"]


def test_header_declares_it():
    text = open(os.path.join(REPO, "include", "mfea.h")).read()
    assert f"int {SYMBOL}(mfea_handle* h, const double* U, const uint8_t* active, double total[2]," in text
    assert "} mfea_element_energy;" in text
    assert "#define MFEA_ABI_VERSION 8" in text
    # the operation order, the gradients and the work identity are part of the contract
    for line in ("d    = (n0*δ0 + n1*δ1) + n2*δ2", "t_c  = δ_c − d*n_c", "g_axial   = ((0.5*d)*d) / Ls",
                 "g_bending = (0.5*q) / cube(Ls)", "∂W/∂E_e = A_e·g_axial + (12·I_e)·g_bending",
                 "∂W/∂A_e = E_e·g_axial", "∂W/∂I_e = (12·E_e)·g_bending",
                 "2W = dy_top·(top·S_top) + dy_bot·(bot·S_bot) + u_fᵀ(KU)_f"):
        assert line in text, line


# ---------------------------------------------------------------------------
# energy.hpp on the host against the restatement
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return er.build_energy_main(tmp_path_factory.mktemp("energy_main"), sanitize=True)


def _case(name):
    """The mesh with the 4x recipe, a tenth of the elements off and the
    oracle's direct-solve U of the tensile test."""
    xyz, e2n, _, _ = er.mesh_of(name)
    props = er.props4(len(e2n))
    active = er.tenth_off(name)
    _, U, _, _ = er.direct(name, "tensile", props, active)
    return xyz, e2n, props, active, U


@pytest.mark.parametrize("name", er.MESHES)
def test_header_equals_restatement(program, tmp_path, name):
    xyz, e2n, props, active, U = _case(name)
    EA, EI12 = er.sections(props)
    assert not active.all() and active.any()
    # two elements more than the mesh has: a zero-length one between two
    # coincident nodes that moved apart, counting, and the same one switched off
    p = np.array([[0.25, -0.5, 0.125]])
    xyz2 = np.concatenate([xyz, p, p])
    U2 = np.concatenate([U, [1e-3, -2e-3, 5e-4], [-1e-3, 1e-3, 2e-3]])
    n0 = len(xyz)
    e2n2 = np.concatenate([e2n, [[n0, n0 + 1], [n0, n0 + 1]]])
    EA2, EI2 = np.append(EA, [EA[0], EA[0]]), np.append(EI12, [EI12[0], EI12[0]])
    act2 = np.append(active, [True, False])
    got = er.run_energy_main(program, er.records(xyz2, e2n2, U2, EA2, EI2, act2), tmp_path)
    want = er.restate(xyz2, e2n2, U2, EA2, EI2, act2)
    # axial rows: no cube involved — the same IEEE operations, the same bits
    assert er.same_bits(got[0], want[0]) and er.same_bits(got[2], want[2])
    # bending rows: NumPy's Ls³ is two rounded products, the header's a
    # half-ulp double-double
    for k in (1, 3):
        assert np.all(np.abs(got[k] - want[k]) <= 4 * ULP * np.abs(want[k])), k
    # w = section · g, exact in bits
    assert er.same_bits(got[0], EA2 * got[2]) and er.same_bits(got[1], EI2 * got[3])
    for k in range(4):
        assert np.all(got[k][~act2] == 0.0) and np.all(np.isfinite(got[k]))
    # the zero-length element: n = 0, d = 0, t = δ, w_b = ½ k_b |δ|²
    z = len(e2n)
    dl = U2.reshape(-1, 3)[n0 + 1] - U2.reshape(-1, 3)[n0]
    assert got[0][z] == 0.0 and got[2][z] == 0.0
    q = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]
    assert abs(got[3][z] - 0.5 * q / 1e-36) <= 4 * ULP * got[3][z] and got[1][z] > 0.0


# ---------------------------------------------------------------------------
# the restatement against ½ UᵀKU, the work identity and central differences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("motion", list(er.MOTIONS))
@pytest.mark.parametrize("name", er.MESHES)
def test_restatement_is_half_UKU_and_the_work_identity(name, motion):
    """Both to 1e-12 of W.  Measured: 0 to 1.6e-16 on test_X, 1.7e-14 to
    2.2e-13 on the two samples — the reference's own error: K's entries are
    rounded, and UᵀKU on a U that is mostly rigid motion amplifies that by
    (|u| / |δ|)²; an extended-precision sum of the same K gives the same level."""
    xyz, e2n, top, bot = er.mesh_of(name)
    props = er.props4(len(e2n))
    active = er.tenth_off(name)
    K, U, known, _ = er.direct(name, motion, props, active)
    EA, EI12 = er.sections(props)
    w_ax, w_b, _, _ = er.restate(xyz, e2n, U, EA, EI12, active)
    W = math.fsum(w_ax) + math.fsum(w_b)
    R = K @ U
    W_K = 0.5 * float(U @ R)
    print(f"{name} {motion}: W {W:.6e}, |W - UKU/2|/W {abs(W - W_K) / W:.2e}, axial share {math.fsum(w_ax) / W:.3f}")
    assert W > er.LOADED and abs(W - W_K) <= 1e-12 * W
    t, b = (np.asarray(v) for v in er.MOTIONS[motion])
    R3 = R.reshape(-1, 3)
    only_top = np.setdiff1d(top, bot)  # (a node in both bands counts in the bottom one)
    S_top, S_bot = R3[only_top].sum(axis=0), R3[bot].sum(axis=0)
    free = np.setdiff1d(np.arange(len(U)), known)
    work = er.AMP * float(t @ S_top) + (-er.AMP) * float(b @ S_bot) + float(U[free] @ R[free])
    print(f"  |2W - work|/2W {abs(2 * W - work) / (2 * W):.2e}")
    assert abs(2.0 * W - work) <= 1e-12 * 2.0 * W


def test_gradients_equal_central_differences():
    """dW/dE_e, dW/dA_e, dW/dI_e from the g rows against central differences of
    ½ UᵀKU (relative step 1e-4) on the four test_X elements with the largest
    energy, to 1e-6.  Measured: worst 7.4e-08."""
    xyz, e2n, top, bot = er.mesh_of(er.X)
    n = len(e2n)
    props = er.props4(n)
    active = np.ones(n, dtype=bool)
    known, vals = er.known_map(top, bot, er.AMP, -er.AMP, er.EY, er.EY)

    # reg = 0: the equilibrium of K itself.  The oracle's default 1e-12 on the
    # diagonal is 1e-5 of this mesh's bending stiffness; its U minimises
    # W + ½ reg |u_f|², and the derivative of W alone along that path differs
    # from the explicit term by 4e-7 of dW/dI_e (measured, whatever the step).
    def energy(p):
        K = het_K(xyz, e2n, active, p["E"], p["A"], p["I"]).tocsr()
        U = fo.solve_system(K, known, vals, reg=0.0)
        return 0.5 * float(U @ (K @ U)), U

    _, U = energy(props)
    EA, EI12 = er.sections(props)
    w_ax, w_b, g_ax, g_b = er.restate(xyz, e2n, U, EA, EI12, active)
    grad = {"E": props["A"] * g_ax + (12.0 * props["I"]) * g_b, "A": props["E"] * g_ax,
            "I": (12.0 * props["E"]) * g_b}
    worst = 0.0
    for e in np.argsort(w_ax + w_b)[-4:]:
        for k in ("E", "A", "I"):
            h = 1e-4 * props[k][e]
            hi, lo = ({**props, k: props[k].copy()} for _ in range(2))
            hi[k][e] += h
            lo[k][e] -= h
            fd = (energy(hi)[0] - energy(lo)[0]) / (hi[k][e] - lo[k][e])
            err = abs(fd - grad[k][e]) / abs(grad[k][e])
            worst = max(worst, err)
            assert err <= 1e-6, (int(e), k, fd, grad[k][e])
    print(f"worst relative error of the gradients against central differences: {worst:.2e}")


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------
def _three_node_mesh(tmp_path):
    d = tmp_path / "mesh"
    d.mkdir()
    pd.DataFrame({"node_id": [0, 1, 2], "x": [0.0, 0, 0], "y": [0.0, 1, 2], "z": [0.0, 0, 0]}) \
        .to_csv(d / "nodes.csv", index=False)
    pd.DataFrame({"elem_id": [0, 1], "n1": [0, 1], "n2": [1, 2]}).to_csv(d / "elements.csv", index=False)
    return str(d)


def test_cli_hands_energy_on(tmp_path, monkeypatch):
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)
    seen = []
    monkeypatch.setattr(fs, "fea_solver", lambda *a, **k: seen.append(k))
    fs.main([d, "--energy"])
    fs.main([d, "--energy", "--device-run"])
    fs.main([d, "--events", "--energy"])
    fs.main([d])
    assert [k["energy"] for k in seen] == [True, True, True, False]
    assert not seen[0]["device_run"] and not seen[0]["events"]
    assert seen[1]["device_run"] and seen[2]["events"]


def test_cli_refuses_energy_on_a_partitioned_run(tmp_path, capsys, monkeypatch):
    """A message and a non-zero status before the device is touched."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)

    def never(*a, **k):
        raise AssertionError("the solver ran")
    monkeypatch.setattr(fs, "fea_solver", never)
    monkeypatch.setattr(fs, "get_engine", never)
    with pytest.raises(SystemExit) as e:
        fs.main([d, "--energy", "--parts", "2"])
    assert e.value.code not in (0, None)
    assert "--energy" in capsys.readouterr().err
    # ... and the function itself, called directly
    monkeypatch.undo()
    monkeypatch.setattr(fs, "get_engine", never)
    with pytest.raises(ValueError, match="energy"):
        fs.fea_solver(d, energy=True, nparts=2, verbose=False)


@pytest.mark.parametrize("fmt", ["python", "petsc"])
def test_energy_files_have_the_stress_records_layout(tmp_path, fmt):
    import fea_solver as fs
    rng = np.random.default_rng(1)
    w_ax, w_b = rng.random((3, 5)), rng.random((3, 5))
    totals = [[float(a.sum()), float(b.sum())] for a, b in zip(w_ax, w_b)]
    curve = [[0.0, 0.0], [0.01, 1.5], [0.02, 3.25]]
    fs.write_energy(str(tmp_path), 5, curve, totals, list(w_ax), list(w_b), fmt, npy=True)
    fs.write_records(str(tmp_path), 2, 5, list(w_ax), [], [], curve, fmt)
    stress = open(tmp_path / "stress_record.csv").read()
    assert open(tmp_path / "element_energy_axial.csv").read() == stress
    assert open(tmp_path / "element_energy_bending.csv").read() != stress
    assert np.array_equal(np.load(tmp_path / "element_energy_bending.npy"), w_b)
    en = pd.read_csv(tmp_path / "energy.csv", float_precision="round_trip")
    assert list(en.columns) == ["step", "total_displacement", "axial_energy", "bending_energy"]
    assert en["step"].tolist() == [1, 2, 3] and en["total_displacement"].tolist() == [0.0, 0.01, 0.02]
    assert np.array_equal(en[["axial_energy", "bending_energy"]].values, np.asarray(totals))
