"""Grip displacement fields (mfea_set_grip_field), the parts that need no GPU:
the exported symbols, the Engine methods, the builders of mfea.fields, the CSV
reader, and the CLI's handling of --grip-field before anything touches the
device."""
import numpy as np
import pandas as pd
import pytest

SYMBOLS = ("mfea_set_grip_field", "mfea_get_grip_field", "mfea_get_grip_work")


def test_symbols_and_methods():
    import mfea
    from mfea import _capi
    assert mfea.abi_version() == 8
    for name in SYMBOLS:
        assert name in _capi.EXPORTED
        assert hasattr(_capi._lib, name)
    for method in ("set_grip_field", "grip_field", "grip_work"):
        assert callable(getattr(mfea.Engine, method))


def test_header_declares_them():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "mfea.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(mfea_handle* h" in text
    assert "#define MFEA_ABI_VERSION 8" in text
    # the row expression and the general work identity are part of the contract
    assert "w_r = (d_r[0]·f_r[0] + d_r[1]·f_r[1]) + d_r[2]·f_r[2]" in text
    assert "2W = dy_top·G_top + dy_bot·G_bot + u_fᵀ(KU)_f" in text


# ---------------------------------------------------------------------------
# mfea.fields
# ---------------------------------------------------------------------------
def _cloud(n=23):
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-2.0, 3.0, (n, 3))
    nodes = np.array([1, 4, 5, 11, 20, 22])
    return xyz, nodes


def _rest_is_zero(f, nodes):
    rest = np.setdiff1d(np.arange(len(f)), nodes)
    return not f[rest].any() and not np.signbit(f[rest]).any()


def test_rigid_rotation():
    from mfea import fields
    xyz, nodes = _cloud()
    axis, c = np.array([0.48, 0.6, 0.64]), np.array([0.5, -1.0, 2.0])
    f = fields.rigid_rotation(xyz, nodes, axis, centre=c)
    assert f.dtype == np.float64 and f.shape == (len(xyz), 3)
    for n in nodes:
        assert np.array_equal(f[n], np.cross(axis, xyz[n] - c))
    assert _rest_is_zero(f, nodes)
    # the default centre: the mean of the listed nodes
    g = fields.rigid_rotation(xyz, nodes, (0, 0, 1))
    m = xyz[nodes].mean(axis=0)
    for n in nodes:
        assert np.array_equal(g[n], np.cross(np.array([0.0, 0.0, 1.0]), xyz[n] - m))
    assert _rest_is_zero(g, nodes)
    # planar points about z stay in the plane
    flat = xyz.copy()
    flat[:, 2] = 0.0
    assert not fields.rigid_rotation(flat, nodes, (0, 0, 1))[:, 2].any()
    with pytest.raises(ValueError, match="out of range"):
        fields.rigid_rotation(xyz, [len(xyz)], (0, 0, 1))


def test_affine():
    from mfea import fields
    xyz, nodes = _cloud()
    H = np.array([[0.1, 0.3, 0.0], [-0.2, 0.05, 0.4], [0.0, 0.7, -0.1]])
    o = np.array([1.0, 2.0, -0.5])
    f = fields.affine(xyz, nodes, H, origin=o)
    assert f.dtype == np.float64 and f.shape == (len(xyz), 3)
    assert np.array_equal(f[nodes], (H @ (xyz[nodes] - o).T).T)
    assert _rest_is_zero(f, nodes)
    assert np.array_equal(fields.affine(xyz, nodes, H)[nodes], (H @ xyz[nodes].T).T)


def test_uniform():
    from mfea import fields
    f = fields.uniform(9, [2, 3, 8], (0.6, 0.8, 0))
    assert f.dtype == np.float64 and f.shape == (9, 3)
    assert np.array_equal(f[[2, 3, 8]], np.broadcast_to([0.6, 0.8, 0.0], (3, 3)))
    assert _rest_is_zero(f, [2, 3, 8])
    assert not fields.uniform(4, [], (1, 0, 0)).any()


# ---------------------------------------------------------------------------
# read_csv
# ---------------------------------------------------------------------------
def test_read_csv_round_trip(tmp_path):
    from mfea import fields
    xyz, nodes = _cloud()
    want = fields.rigid_rotation(xyz, nodes, (0.1, -0.2, 0.3))
    p = tmp_path / "field.csv"
    with open(p, "w") as f:
        f.write("node_id,dx,dy,dz\n")
        for n in nodes[::-1]:  # any order
            f.write(f"{n},{float(want[n, 0])!r},{float(want[n, 1])!r},{float(want[n, 2])!r}\n")
    got, listed = fields.read_csv(str(p), len(xyz))
    assert got.dtype == np.float64 and got.shape == (len(xyz), 3)
    assert np.array_equal(got, want)
    assert listed.dtype == bool and np.array_equal(np.flatnonzero(listed), nodes)
    # the columns in another order, with one more
    q = tmp_path / "field2.csv"
    with open(q, "w") as f:
        f.write("dz,note,dy,dx,node_id\n0.5,a,0.25,-1,3\n")
    got, listed = fields.read_csv(str(q), 5)
    assert got[3].tolist() == [-1.0, 0.25, 0.5] and listed.tolist() == [False, False, False, True, False]


BAD_FILES = [("node_id,dx,dy,dz\n1,0,1,0\n1,0,2,0\n", "duplicate"),
             ("node_id,dx,dy,dz\n3,0,1,0\n", "out of range"),
             ("node_id,dx,dy,dz\n-1,0,1,0\n", "out of range"),
             ("node_id,dx,dy\n1,0,1\n", "missing column"),
             ("dx,dy,dz\n0,1,0\n", "missing column"),
             ("node_id,dx,dy,dz\n1,0,nan,0\n", "non-finite"),
             ("node_id,dx,dy,dz\n1,inf,0,0\n", "non-finite")]


@pytest.mark.parametrize("text,what", BAD_FILES)
def test_read_csv_malformed(tmp_path, text, what):
    from mfea import fields
    p = tmp_path / "bad.csv"
    p.write_text(text)
    with pytest.raises(ValueError, match=what) as e:
        fields.read_csv(str(p), 3)
    assert str(p) in str(e.value)


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


def test_cli_refuses_a_malformed_file(tmp_path, capsys, monkeypatch):
    """A message naming --grip-field and a non-zero status before the device is
    touched: neither the engine nor the step loop is reached."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)

    def never(*a, **k):
        raise AssertionError("the solver ran")
    monkeypatch.setattr(fs, "fea_solver", never)
    monkeypatch.setattr(fs, "get_engine", never)
    p = tmp_path / "bad.csv"
    for text, what in BAD_FILES:
        p.write_text(text)
        with pytest.raises(SystemExit) as e:
            fs.main([d, "--grip-field", str(p)])
        assert e.value.code not in (0, None), text
        err = capsys.readouterr().err
        assert "--grip-field" in err and what in err, (text, err)
    with pytest.raises(SystemExit) as e:  # no such file
        fs.main([d, "--grip-field", str(tmp_path / "absent.csv")])
    assert e.value.code not in (0, None)
    assert "--grip-field" in capsys.readouterr().err
    p.write_text("node_id,dx,dy,dz\n2,1,0,0\n")
    with pytest.raises(SystemExit) as e:  # one partition only
        fs.main([d, "--grip-field", str(p), "--parts", "2"])
    assert e.value.code not in (0, None)
    assert "--grip-field" in capsys.readouterr().err


def test_cli_hands_the_field_on(tmp_path, monkeypatch):
    """The parsed field and its listed-node mask reach fea_solver in every run
    mode and next to the other flags; no flag: None."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)
    p = tmp_path / "field.csv"
    p.write_text("node_id,dx,dy,dz\n2,0.5,0.25,0\n1,9,9,9\n")
    seen = []
    monkeypatch.setattr(fs, "fea_solver", lambda *a, **k: seen.append(k))
    fs.main([d, "--grip-field", str(p)])
    fs.main([d, f"--grip-field={p}", "--device-run", "--energy"])
    fs.main([d, "--grip-field", str(p), "--events", "--shear"])
    fs.main([d])
    for k in seen[:3]:
        field, listed = k["grip_field"]
        assert field.tolist() == [[0, 0, 0], [9, 9, 9], [0.5, 0.25, 0]] and listed.tolist() == [False, True, True]
    assert seen[1]["device_run"] and seen[1]["energy"] and seen[2]["events"]
    assert seen[2]["grip_direction"][0].tolist() == [1.0, 0.0, 0.0]
    assert seen[3]["grip_field"] is None


def test_unlisted_grip_nodes_take_the_band_vector(tmp_path):
    import fea_solver as fs
    top, bot = np.array([4, 5, 2]), np.array([0, 1, 2])  # (node 2 in both bands: a bottom node)
    field = np.zeros((6, 3))
    field[5] = (0.0, 0.0, 0.0)  # a listed zero row: a held node, kept
    field[3] = (7.0, 7.0, 7.0)  # a listed free node: handed on, the engine ignores it
    field[0] = (0.1, 0.2, 0.3)
    listed = np.array([True, False, False, True, False, True])
    out = fs.complete_grip_field((field, listed), 6, top, bot)
    assert out.dtype == np.float64
    assert out.tolist() == [[0.1, 0.2, 0.3], [0, 1, 0], [0, 1, 0], [7, 7, 7], [0, 1, 0], [0, 0, 0]]
    out = fs.complete_grip_field((field, listed), 6, top, bot, fs.parse_grip_direction("1,0,0/0,0,1"))
    assert out.tolist() == [[0.1, 0.2, 0.3], [0, 0, 1], [0, 0, 1], [7, 7, 7], [1, 0, 0], [0, 0, 0]]
    assert not field[1].any()  # the caller's array is not written
    # a path, and a plain array (every node listed)
    p = tmp_path / "f.csv"
    p.write_text("node_id,dx,dy,dz\n4,1,2,3\n")
    out = fs.complete_grip_field(str(p), 6, top, bot)
    assert out[4].tolist() == [1, 2, 3] and out[5].tolist() == [0, 1, 0] and not out[3].any()
    assert np.array_equal(fs.complete_grip_field(field, 6, top, bot), field)
    with pytest.raises(ValueError, match="one row per node"):
        fs.complete_grip_field(np.zeros((5, 3)), 6, top, bot)
