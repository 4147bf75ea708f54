"""Grip motion vectors (mfea_set_grip_motion), the parts that need no GPU: the
exported symbols, the Engine methods, the --grip-direction parser and the CLI's
refusal of a malformed value before anything touches the device."""
import numpy as np
import pandas as pd
import pytest

SYMBOLS = ("mfea_set_grip_motion", "mfea_get_grip_motion", "mfea_get_reaction")


def test_symbols_and_methods():
    import mfea
    from mfea import _capi
    assert mfea.abi_version() == 8
    for name in SYMBOLS:
        assert name in _capi.EXPORTED
        assert hasattr(_capi._lib, name)
    for method in ("set_grip_motion", "grip_motion", "reaction"):
        assert callable(getattr(mfea.Engine, method))


def test_header_declares_them():
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "mfea.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(mfea_handle* h" in text
    assert "#define MFEA_ABI_VERSION 8" in text
    # the force expression is part of the contract
    assert "F = (top[0]·S[0] + top[1]·S[1]) + top[2]·S[2]" in text


def test_parser_good_forms():
    import fea_solver as fs
    top, bot = fs.parse_grip_direction("1,0,0")
    assert top.tolist() == [1.0, 0.0, 0.0] and bot.tolist() == [1.0, 0.0, 0.0]
    assert top.dtype == np.float64 and top is not bot
    top, bot = fs.parse_grip_direction("0.6,0.8,0/0,0,1")
    assert top.tolist() == [0.6, 0.8, 0.0] and bot.tolist() == [0.0, 0.0, 1.0]
    top, bot = fs.parse_grip_direction(" 4.8e-1, 0.6 ,0.64 / -1,0,0 ")
    assert top.tolist() == [0.48, 0.6, 0.64] and bot.tolist() == [-1.0, 0.0, 0.0]
    # not normalised
    assert fs.parse_grip_direction("0,2,0")[0].tolist() == [0.0, 2.0, 0.0]


BAD = [("1,0", "three components"), ("1,0,0,0", "three components"), ("1,0,0/0,1", "three components"),
       ("1,0,0/0,1,0/0,0,1", "at most one"), ("1,a,0", "not a number"), ("1,,0", "not a number"),
       ("", "three components"), ("0,0,0", "all zero"), ("1,0,0/0,0,-0", "all zero"), ("nan,0,0", "finite"),
       ("1,0,0/0,inf,0", "finite")]


@pytest.mark.parametrize("text,what", BAD)
def test_parser_malformed(text, what):
    import fea_solver as fs
    with pytest.raises(ValueError, match=what):
        fs.parse_grip_direction(text)


def _three_node_mesh(tmp_path):
    d = tmp_path / "mesh"
    d.mkdir()
    pd.DataFrame({"node_id": [0, 1, 2], "x": [0.0, 0, 0], "y": [0.0, 1, 2], "z": [0.0, 0, 0]}) \
        .to_csv(d / "nodes.csv", index=False)
    pd.DataFrame({"elem_id": [0, 1], "n1": [0, 1], "n2": [1, 2]}).to_csv(d / "elements.csv", index=False)
    return str(d)


def test_cli_refuses_a_malformed_direction(tmp_path, capsys, monkeypatch):
    """A clear message and a non-zero status before the device is touched: the
    step loop is never entered."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)

    def never(*a, **k):
        raise AssertionError("the solver ran")
    monkeypatch.setattr(fs, "fea_solver", never)
    monkeypatch.setattr(fs, "get_engine", never)
    for text, what in BAD:
        with pytest.raises(SystemExit) as e:
            fs.main([d, f"--grip-direction={text}"])
        assert e.value.code not in (0, None), text
        err = capsys.readouterr().err
        assert "--grip-direction" in err and what in err, (text, err)
    with pytest.raises(SystemExit) as e:
        fs.main([d, "--shear", "--grip-direction", "0,1,0"])
    assert e.value.code not in (0, None)


def test_cli_hands_the_direction_on(tmp_path, monkeypatch):
    """--shear is 1,0,0 for both grips; --grip-direction reaches fea_solver
    parsed, with every run mode; no flag: None (the tensile test)."""
    import fea_solver as fs
    d = _three_node_mesh(tmp_path)
    seen = []
    monkeypatch.setattr(fs, "fea_solver", lambda *a, **k: seen.append(k))
    fs.main([d, "--shear"])
    fs.main([d, "--grip-direction", "0.6,0.8,0/0,1,0", "--device-run"])
    fs.main([d, "--grip-direction=-1,0,0", "--events"])
    fs.main([d])
    g = [k["grip_direction"] for k in seen]
    assert g[0][0].tolist() == [1.0, 0.0, 0.0] and g[0][1].tolist() == [1.0, 0.0, 0.0]
    assert g[1][0].tolist() == [0.6, 0.8, 0.0] and g[1][1].tolist() == [0.0, 1.0, 0.0] and seen[1]["device_run"]
    assert g[2][0].tolist() == [-1.0, 0.0, 0.0] and seen[2]["events"]
    assert g[3] is None
