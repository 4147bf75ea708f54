"""Nodal loads (mfea_set_node_loads), the parts that need no GPU: the exported
symbols, the Engine methods, the builders of mfea.loads, the CSV reader, and
the CLI's handling of --node-loads / --load-mode before anything touches the
device."""
import numpy as np
import pandas as pd
import pytest

SYMBOLS = ("mfea_set_node_loads", "mfea_get_node_loads", "mfea_get_load_work")


def test_symbols_and_methods():
    import mfea
    from mfea import _capi
    assert mfea.abi_version() == 8
    for name in SYMBOLS:
        assert name in _capi.EXPORTED
        assert hasattr(_capi._lib, name)
    for method in ("set_node_loads", "node_loads", "load_work"):
        assert callable(getattr(mfea.Engine, method))
    assert (mfea.LOAD_DEAD, mfea.LOAD_PROPORTIONAL) == (0, 1)


def test_header_declares_them():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "mfea.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(mfea_handle* h" in text
    assert "#define MFEA_ABI_VERSION 8" in text
    assert "#define MFEA_LOAD_DEAD 0" in text and "#define MFEA_LOAD_PROPORTIONAL 1" in text
    # the work identity with loads is part of the contract
    assert "u_fᵀ(KU)_f = L − reg·‖u_f‖² − u_f·r" in text
    assert "2W = dy_top·G_top + dy_bot·G_bot + L" in text


# ---------------------------------------------------------------------------
# mfea.loads
# ---------------------------------------------------------------------------
def _network(n=19, m=31):
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-2.0, 3.0, (n, 3))
    e2n = np.array([(a, b) for a, b in rng.integers(0, n, (3 * m, 2)) if a != b][:m])
    return xyz, e2n


def test_point():
    from mfea import loads
    nodes = np.array([2, 7, 11])
    f = loads.point(13, nodes, (0.5, -1.0, 0.25))
    assert f.dtype == np.float64 and f.shape == (13, 3)
    assert np.array_equal(f[nodes], np.broadcast_to([0.5, -1.0, 0.25], (3, 3)))
    rest = np.setdiff1d(np.arange(13), nodes)
    assert not f[rest].any() and not np.signbit(f[rest]).any()
    # one row per node; a node listed twice takes the sum
    g = loads.point(5, [1, 3, 1], [[1, 0, 0], [0, 2, 0], [0.5, 0, 3]])
    assert g[1].tolist() == [1.5, 0.0, 3.0] and g[3].tolist() == [0.0, 2.0, 0.0]
    assert not loads.point(4, [], (1, 2, 3)).any()
    with pytest.raises(ValueError, match="out of range"):
        loads.point(4, [4], (1, 0, 0))
    with pytest.raises(ValueError, match="out of range"):
        loads.point(4, [-1], (1, 0, 0))
    with pytest.raises(ValueError, match="one row per node"):
        loads.point(4, [0, 1], [[1, 0, 0]] * 3)


def test_self_weight_sums_to_the_total_weight():
    from mfea import loads
    xyz, e2n = _network()
    L = np.linalg.norm(xyz[e2n[:, 1]] - xyz[e2n[:, 0]], axis=1)
    d = np.array([0.0, -1.0, 0.0])
    # a scalar weight per length
    f = loads.self_weight(xyz, e2n, 0.3, d)
    assert f.dtype == np.float64 and f.shape == (len(xyz), 3)
    assert np.allclose(f.sum(axis=0), (L * 0.3).sum() * d, rtol=1e-13, atol=0)
    assert not f[:, 0].any() and not f[:, 2].any()
    # one value per element, any direction: Σ L_e · w_e · direction
    w = np.random.default_rng(9).uniform(0.1, 2.0, len(e2n))
    d = np.array([0.48, 0.6, -0.64])
    f = loads.self_weight(xyz, e2n, w, d)
    assert np.allclose(f.sum(axis=0), (L * w).sum() * d, rtol=1e-13, atol=0)
    # each element puts half on each end
    one = loads.self_weight(xyz, e2n[:1], w[:1], d)
    assert np.array_equal(one[e2n[0, 0]], 0.5 * L[0] * w[0] * d) and np.array_equal(one[e2n[0, 0]], one[e2n[0, 1]])
    assert np.count_nonzero(one.any(axis=1)) == 2


def test_self_weight_skips_inactive_elements():
    from mfea import loads
    xyz, e2n = _network()
    w = np.random.default_rng(9).uniform(0.1, 2.0, len(e2n))
    d = np.array([0.0, -1.0, 0.0])
    active = np.random.default_rng(2).random(len(e2n)) < 0.6
    assert 0 < active.sum() < len(e2n)
    f = loads.self_weight(xyz, e2n, w, d, active=active)
    assert np.array_equal(f, loads.self_weight(xyz, e2n[active], w[active], d))
    L = np.linalg.norm(xyz[e2n[:, 1]] - xyz[e2n[:, 0]], axis=1)
    assert np.allclose(f.sum(axis=0), (L * w)[active].sum() * d, rtol=1e-13, atol=0)
    # a node whose elements are all inactive carries nothing
    touched = np.zeros(len(xyz), bool)
    touched[e2n[active].ravel()] = True
    assert not f[~touched].any()
    assert not loads.self_weight(xyz, e2n, w, d, active=np.zeros(len(e2n), np.uint8)).any()
    with pytest.raises(ValueError, match="one entry per element"):
        loads.self_weight(xyz, e2n, w, d, active=active[:-1])
    with pytest.raises(ValueError, match="one value per element"):
        loads.self_weight(xyz, e2n, w[:-1], d)
    with pytest.raises(ValueError, match="out of range"):
        loads.self_weight(xyz, [[0, len(xyz)]], 1.0, d)


def test_read_csv_round_trip(tmp_path):
    from mfea import loads
    nodes = np.array([1, 4, 5, 11])
    want = loads.point(17, nodes, np.random.default_rng(1).normal(size=(4, 3)))
    p = tmp_path / "loads.csv"
    with open(p, "w") as f:
        f.write("node_id,fx,fy,fz\n")
        for n in nodes[::-1]:  # any order
            f.write(f"{n},{float(want[n, 0])!r},{float(want[n, 1])!r},{float(want[n, 2])!r}\n")
    got = loads.read_csv(str(p), 17)
    assert got.dtype == np.float64 and got.shape == (17, 3) and np.array_equal(got, want)
    q = tmp_path / "loads2.csv"  # the columns in another order, with one more
    q.write_text("fz,note,fy,fx,node_id\n0.5,a,0.25,-1,3\n")
    assert loads.read_csv(str(q), 5)[3].tolist() == [-1.0, 0.25, 0.5]


BAD_FILES = [("node_id,fx,fy,fz\n1,0,1,0\n1,0,2,0\n", "duplicate"),
             ("node_id,fx,fy,fz\n3,0,1,0\n", "out of range"),
             ("node_id,fx,fy,fz\n-1,0,1,0\n", "out of range"),
             ("node_id,fx,fy\n1,0,1\n", "missing column"),
             ("fx,fy,fz\n0,1,0\n", "missing column"),
             ("node_id,dx,dy,dz\n1,0,1,0\n", "missing column"),
             ("node_id,fx,fy,fz\n1,0,nan,0\n", "non-finite"),
             ("node_id,fx,fy,fz\n1,inf,0,0\n", "non-finite"),
             ("node_id,fx,fy,fz\n1,0,x,0\n", "not a number"),
             ("node_id,fx,fy,fz\n1.5,0,1,0\n", "not an integer")]


@pytest.mark.parametrize("text,what", BAD_FILES)
def test_read_csv_malformed(tmp_path, text, what):
    """The ValueErrors of mfea.fields.read_csv, naming the file."""
    from mfea import fields, loads
    p = tmp_path / "bad.csv"
    p.write_text(text)
    with pytest.raises(ValueError, match=what) as e:
        loads.read_csv(str(p), 3)
    assert str(p) in str(e.value)
    if "dx" not in text:  # the same file under the field's column names: the same error
        p.write_text(text.replace("fx", "dx").replace("fy", "dy").replace("fz", "dz"))
        with pytest.raises(ValueError, match=what):
            fields.read_csv(str(p), 3)


# ---------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------
def _three_node_mesh(tmp_path):
    d = tmp_path / "mesh"
    d.mkdir()
    pd.DataFrame({"node_id": [0, 1, 2], "x": [0.0, 0, 0], "y": [0.0, 1, 2], "z": [0.0, 0, 0]}) \
        .to_csv(d / "nodes.csv", index=False)
    pd.DataFrame({"elem_id": [0, 1], "n1": [0, 1], "n2": [1, 2]}).to_csv(d / "elements.csv", index=False)
    return str(d)


def _never(*a, **k):
    raise AssertionError("the solver ran")


def test_cli_refuses_before_the_device(tmp_path, capsys, monkeypatch):
    """A message naming --node-loads and a non-zero status before the device is
    touched: neither the engine nor the step loop is reached."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)
    monkeypatch.setattr(fs, "fea_solver", _never)
    monkeypatch.setattr(fs, "get_engine", _never)
    p = tmp_path / "bad.csv"
    for text, what in BAD_FILES:
        p.write_text(text)
        with pytest.raises(SystemExit) as e:
            fs.main([d, "--node-loads", str(p)])
        assert e.value.code not in (0, None), text
        err = capsys.readouterr().err
        assert "--node-loads" in err and what in err, (text, err)
    with pytest.raises(SystemExit) as e:  # no such file
        fs.main([d, "--node-loads", str(tmp_path / "absent.csv")])
    assert e.value.code not in (0, None)
    assert "--node-loads" in capsys.readouterr().err
    p.write_text("node_id,fx,fy,fz\n1,1,0,0\n")
    with pytest.raises(SystemExit) as e:  # one partition only
        fs.main([d, "--node-loads", str(p), "--parts", "2"])
    assert e.value.code not in (0, None)
    assert "--node-loads" in capsys.readouterr().err
    for extra in ([], ["--load-mode", "dead"]):  # events: proportional loads only
        with pytest.raises(SystemExit) as e:
            fs.main([d, "--node-loads", str(p), "--events"] + extra)
        assert e.value.code not in (0, None)
        err = capsys.readouterr().err
        assert "--events" in err and "proportional" in err
    with pytest.raises(SystemExit) as e:  # an unknown mode: argparse's own refusal
        fs.main([d, "--node-loads", str(p), "--load-mode", "follower"])
    assert e.value.code not in (0, None)


def test_fea_solver_refuses_before_the_device(tmp_path, monkeypatch):
    """The function's own checks come before the mesh is read or the engine made."""
    import fea_solver as fs
    monkeypatch.setattr(fs, "get_engine", _never)
    d = _three_node_mesh(tmp_path)
    f = np.zeros((3, 3))
    with pytest.raises(ValueError, match="one partition"):
        fs.fea_solver(d, node_loads=f, nparts=2, verbose=False)
    with pytest.raises(ValueError, match="proportional"):
        fs.fea_solver(d, node_loads=f, events=True, verbose=False)
    with pytest.raises(ValueError, match="load_mode"):
        fs.fea_solver(d, node_loads=f, load_mode="follower", verbose=False)


def test_cli_hands_the_loads_on(tmp_path, monkeypatch):
    """The parsed loads and the mode reach fea_solver in every run mode and next
    to the other flags; no flag: None, and the default mode is dead."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)
    p = tmp_path / "loads.csv"
    p.write_text("node_id,fx,fy,fz\n1,0.5,0.25,0\n")
    g = tmp_path / "field.csv"
    g.write_text("node_id,dx,dy,dz\n0,0,0,0\n")
    seen = []
    monkeypatch.setattr(fs, "fea_solver", lambda *a, **k: seen.append(k))
    fs.main([d, "--node-loads", str(p)])
    fs.main([d, f"--node-loads={p}", "--device-run", "--energy", "--grip-field", str(g)])
    fs.main([d, "--node-loads", str(p), "--events", "--load-mode", "proportional", "--shear"])
    fs.main([d])
    for k in seen[:3]:
        assert k["node_loads"].tolist() == [[0, 0, 0], [0.5, 0.25, 0], [0, 0, 0]]
    assert [k["load_mode"] for k in seen] == ["dead", "dead", "proportional", "dead"]
    assert seen[1]["device_run"] and seen[1]["energy"] and seen[1]["grip_field"] is not None
    assert seen[2]["events"] and seen[2]["grip_direction"][0].tolist() == [1.0, 0.0, 0.0]
    assert seen[3]["node_loads"] is None
