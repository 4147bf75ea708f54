"""Per-element properties, the parts that need no GPU: the exported symbols and
the ctypes struct, the --element-props file parser, the synth helpers."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest


def test_symbols_and_struct():
    import mfea
    from mfea import _capi
    assert mfea.abi_version() == 8
    for name in ("mfea_set_element_props", "mfea_get_element_props"):
        assert name in _capi.EXPORTED
        assert hasattr(_capi._lib, name)
    fields = mfea.ElementProps._fields_
    assert [f for f, _ in fields] == ["E", "A", "I", "max_strain"]
    assert all(t is C.c_void_p for _, t in fields)
    assert C.sizeof(mfea.ElementProps) == 4 * C.sizeof(C.c_void_p)
    assert callable(mfea.Engine.set_element_props) and callable(mfea.Engine.element_props)


def _write(path, **cols):
    pd.DataFrame(cols).to_csv(path, index=False)
    return str(path)


def test_props_file_parser(tmp_path):
    import fea_solver as fs
    n = 7
    rng = np.random.default_rng(0)
    order = rng.permutation(n)
    A, s = rng.random(n), rng.random(n) + 0.5
    # a column subset, ids in any order, columns in any order
    got = fs.read_element_props(_write(tmp_path / "a.csv", max_strain=s[order], elem_id=order, A=A[order]), n)
    assert sorted(got) == ["A", "max_strain"]
    assert np.array_equal(got["A"], A) and np.array_equal(got["max_strain"], s)
    assert got["A"].dtype == np.float64 and got["A"].flags.c_contiguous
    # all four columns; inf is a strength
    s2 = s.copy()
    s2[3] = np.inf
    got = fs.read_element_props(_write(tmp_path / "b.csv", elem_id=np.arange(n), E=A, A=A, I=A, max_strain=s2), n)
    assert sorted(got) == ["A", "E", "I", "max_strain"] and np.isinf(got["max_strain"][3])
    # elem_id alone: nothing set
    assert fs.read_element_props(_write(tmp_path / "c.csv", elem_id=np.arange(n)), n) == {}
    # a missing id, a duplicate id, an id out of range, no elem_id, an unknown column
    ids = np.arange(n)
    with pytest.raises(ValueError, match="missing element id 6"):
        fs.read_element_props(_write(tmp_path / "d.csv", elem_id=ids[:-1], A=A[:-1]), n)
    dup = ids.copy()
    dup[2] = 4
    with pytest.raises(ValueError, match="duplicate element id 4"):
        fs.read_element_props(_write(tmp_path / "e.csv", elem_id=dup, A=A), n)
    with pytest.raises(ValueError, match="outside"):
        fs.read_element_props(_write(tmp_path / "f.csv", elem_id=ids + 1, A=A), n)
    with pytest.raises(ValueError, match="elem_id"):
        fs.read_element_props(_write(tmp_path / "g.csv", A=A), n)
    with pytest.raises(ValueError, match="unknown column"):
        fs.read_element_props(_write(tmp_path / "h.csv", elem_id=ids, diameter=A), n)


def test_cli_refuses_a_bad_props_file(tmp_path, capsys):
    """A missing or duplicate id: a clear message and a non-zero status, before
    anything touches the device."""
    import fea_solver as fs
    d = tmp_path / "mesh"
    d.mkdir()
    pd.DataFrame({"node_id": [0, 1, 2], "x": [0.0, 0, 0], "y": [0.0, 1, 2], "z": [0.0, 0, 0]}) \
        .to_csv(d / "nodes.csv", index=False)
    pd.DataFrame({"elem_id": [0, 1], "n1": [0, 1], "n2": [1, 2]}).to_csv(d / "elements.csv", index=False)
    for name, ids, what in (("missing.csv", [0], "missing element id 1"), ("dup.csv", [0, 0], "duplicate element id 0")):
        f = _write(tmp_path / name, elem_id=ids, A=[1.0] * len(ids))
        with pytest.raises(SystemExit) as e:
            fs.main([str(d), "--element-props", f])
        assert e.value.code not in (0, None)
        assert what in capsys.readouterr().err


def test_synth_helpers():
    from mfea import synth
    import fea_oracle as fo
    # the reference's own section at its constants
    A, I = synth.section_from_diameter(fo.D_FIL, fo.T_WALL)  # noqa: E741
    assert A == fo.AREA and I == fo.INERTIA
    d = np.array([1e-4, 2e-4, 5e-4])
    t = np.array([1e-6, 1e-6, 2e-6])
    A, I = synth.section_from_diameter(d, t)  # noqa: E741
    assert np.array_equal(A, 3.14 * ((d / 2) ** 2 - (d / 2 - t) ** 2)) and np.array_equal(I, A * 0.001)
    assert synth.section_from_diameter(d, 1e-6)[0].shape == (3,)
    s = synth.weibull_strength(1000, 6.0, 0.018, seed=7)
    assert np.array_equal(s, 0.018 * np.random.default_rng(7).weibull(6.0, 1000))
    assert np.array_equal(s, synth.weibull_strength(1000, 6.0, 0.018, 7)) and s.min() > 0
    f = synth.weibull_strength(1000, 6.0, 0.018, 7, floor=0.012)
    assert np.array_equal(f, np.maximum(s, 0.012)) and (f == 0.012).any() and (f > 0.012).any()
