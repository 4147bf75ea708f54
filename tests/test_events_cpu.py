"""The host side of the event-driven failure runs (mfea_event / mfea_run_events)
that needs no device: the ABI, the ctypes layout against the header, the
envelope helper, the argument checks and the drop-in's refusal of partitions."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def test_event_symbols_are_exported_and_the_abi_version_stays():
    import mfea
    from mfea import _capi
    for name in ("mfea_event", "mfea_run_events"):
        assert name in _capi.EXPORTED and hasattr(_capi._lib, name)
    assert _capi.abi_version() == 8
    for name in ("EventOpts", "EventOut", "EventRecords", "event_opts", "event_envelope", "EVENTS_COMPLETE",
                 "EVENTS_LAMBDA_MAX", "EVENTS_UNLOADED"):
        assert hasattr(mfea, name), name
    assert (mfea.EVENTS_COMPLETE, mfea.EVENTS_LAMBDA_MAX, mfea.EVENTS_UNLOADED) == (0, 1, 2)
    assert callable(mfea.Engine.event) and callable(mfea.Engine.run_events)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mfea.h"
#define S(T) printf(#T " size %zu\n", sizeof(T))
#define O(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main(void) {
  S(mfea_event_opts); O(mfea_event_opts, max_strain); O(mfea_event_opts, tie_rtol); O(mfea_event_opts, lam_max);
  S(mfea_event_out); O(mfea_event_out, lam); O(mfea_event_out, force1); O(mfea_event_out, n_failed);
  O(mfea_event_out, n_active);
  S(mfea_event_records); O(mfea_event_records, U); O(mfea_event_records, stress); O(mfea_event_records, active);
  O(mfea_event_records, lam); O(mfea_event_records, force1); O(mfea_event_records, n_failed);
  O(mfea_event_records, n_active); O(mfea_event_records, event_of); O(mfea_event_records, stats);
  O(mfea_event_records, wall_s);
  printf("codes %d %d %d\n", MFEA_EVENTS_COMPLETE, MFEA_EVENTS_LAMBDA_MAX, MFEA_EVENTS_UNLOADED);
  return 0;
}
"""


def test_ctypes_layout_matches_the_header(tmp_path):
    from mfea import _capi
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    py = {"mfea_event_opts": _capi.EventOpts, "mfea_event_out": _capi.EventOut,
          "mfea_event_records": _capi.EventRecords}
    seen = {k: [] for k in py}
    for ln in lines:
        w = ln.split()
        if not w:
            continue
        if w[0] == "codes":
            assert [int(x) for x in w[1:]] == [_capi.EVENTS_COMPLETE, _capi.EVENTS_LAMBDA_MAX,
                                               _capi.EVENTS_UNLOADED]
        elif w[1] == "size":
            assert C.sizeof(py[w[0]]) == int(w[2]), ln
        else:
            assert getattr(py[w[0]], w[1]).offset == int(w[2]), ln
            seen[w[0]].append(w[1])
    for k, cls in py.items():  # every field, in the header's order
        assert seen[k] == [n for n, _ in cls._fields_], k


def test_envelope_monotone():
    from mfea import event_envelope
    disp, force = event_envelope([0.25, 0.5, 0.75], [8.0, 4.0, 2.0], 0.5)
    assert disp.tolist() == [0.125, 0.125, 0.25, 0.25, 0.375, 0.375]
    assert force.tolist() == [2.0, 1.0, 2.0, 1.0, 1.5, 1.5]


def test_envelope_avalanche_holds_the_displacement():
    from mfea import event_envelope
    # event 1 needs less load than event 0 reached: it breaks at held displacement
    disp, force = event_envelope([0.5, 0.25, 0.75], [8.0, 4.0, 2.0], 2.0)
    assert disp.tolist() == [1.0, 1.0, 1.0, 1.0, 1.5, 1.5]
    assert force.tolist() == [4.0, 2.0, 2.0, 1.0, 1.5, 1.5]


def test_envelope_terminal_inf_stays_at_the_last_displacement():
    from mfea import event_envelope
    disp, force = event_envelope([0.5, np.inf], [8.0, 0.0], 2.0)
    assert disp.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert force.tolist() == [4.0, 0.0, 0.0, 0.0]
    d0, f0 = event_envelope([], [], 1.0)
    assert d0.size == 0 and f0.size == 0
    with pytest.raises(ValueError, match="one entry per event"):
        event_envelope([1.0], [1.0, 2.0], 1.0)


@pytest.mark.parametrize("kw,msg", [
    (dict(max_strain=0.0), "max_strain must be > 0"),
    (dict(max_strain=-1.0), "max_strain must be > 0"),
    (dict(max_strain=float("nan")), "max_strain must be > 0"),
    (dict(max_strain=0.018, tie_rtol=-1e-9), r"tie_rtol must be in \[0, 1\)"),
    (dict(max_strain=0.018, tie_rtol=1.0), r"tie_rtol must be in \[0, 1\)"),
    (dict(max_strain=0.018, lam_max=0.0), "lam_max must be > 0"),
    (dict(max_strain=0.018, lam_max=float("nan")), "lam_max must be > 0"),
])
def test_argument_checks_python_and_library(kw, msg):
    """The binding and the library refuse the same values with the same words
    (the library checks the options before anything else, so no device is needed)."""
    import re
    from mfea import _capi
    with pytest.raises(ValueError, match=msg):
        _capi.event_opts(**kw)
    ev = _capi.EventOpts(kw["max_strain"], kw.get("tie_rtol", 1e-9), kw.get("lam_max", float("inf")))
    out = _capi.EventOut()
    assert _capi._lib.mfea_event(None, 0.02, -0.02, None, C.byref(ev), C.byref(out), None) == _capi.EINVAL
    assert re.search(msg, _capi.last_error())
    n_done, stop = C.c_int32(), C.c_int32()
    rec = _capi.EventRecords()
    assert _capi._lib.mfea_run_events(None, 1, 0.02, -0.02, None, C.byref(ev), C.byref(rec), C.byref(n_done),
                                      C.byref(stop)) == _capi.EINVAL
    assert re.search(msg, _capi.last_error())


def test_good_options_pass_and_null_arguments_are_refused():
    from mfea import _capi
    ev = _capi.event_opts(0.018, 0.0, float("inf"))
    assert (ev.max_strain, ev.tie_rtol, ev.lam_max) == (0.018, 0.0, float("inf"))
    out = _capi.EventOut()
    assert _capi._lib.mfea_event(None, 0.02, -0.02, None, C.byref(ev), C.byref(out), None) == _capi.EINVAL
    assert "NULL argument" in _capi.last_error()
    assert _capi._lib.mfea_event(None, 0.02, -0.02, None, None, C.byref(out), None) == _capi.EINVAL


def test_cli_rejects_events_with_partitions(tmp_path):
    import fea_solver as fs
    d = tmp_path / "test_X"
    shutil.copytree(os.path.join(GOLDEN, "meshes", "test_X"), d)
    before = fs._engine
    saved = (fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG)
    try:
        with pytest.raises(ValueError, match="events needs one process and one partition"):
            fs.main([str(d), "--events", "--parts", "2"])
    finally:
        fs.N_STEPS, fs.DISPLACEMENT_MAX, fs.MAX_STRAIN, fs.REG = saved
    assert fs._engine is before  # no handle was created
    assert not (d / "fea_results").exists()
