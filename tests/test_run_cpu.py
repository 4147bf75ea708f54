"""The host side of mfea_run that needs no device: the ABI, the ctypes layout
and the drop-in's argument check."""
import ctypes as C
import os
import shutil

import pytest

from conftest import GOLDEN


def test_capi_exposes_run_and_its_record_layout():
    from mfea import _capi
    assert callable(_capi.Engine.run)
    assert C.sizeof(_capi.RunRecords) == 7 * C.sizeof(C.c_void_p)
    assert [n for n, _ in _capi.RunRecords._fields_] == ["U", "stress", "active", "force", "n_active",
                                                         "stats", "wall_s"]
    assert (_capi.RUN_COMPLETE, _capi.RUN_NO_ACTIVE) == (0, 1)


def test_run_is_exported_and_the_abi_version_stays():
    from mfea import _capi
    assert "mfea_run" in _capi.EXPORTED
    assert hasattr(_capi._lib, "mfea_run")
    assert _capi.abi_version() == 8


def test_run_rejects_null_arguments_without_a_device():
    from mfea import _capi
    n_done, stop = C.c_int32(), C.c_int32()
    rec = _capi.RunRecords()
    assert _capi._lib.mfea_run(None, 1, None, None, None, 0.018, C.byref(rec), C.byref(n_done),
                               C.byref(stop)) == _capi.EINVAL


def test_dropin_device_run_refuses_partitions_before_touching_the_device(tmp_path):
    import fea_solver as fs
    d = tmp_path / "test_X"
    shutil.copytree(os.path.join(GOLDEN, "meshes", "test_X"), d)
    before = fs._engine
    with pytest.raises(ValueError):
        fs.fea_solver(str(d), tol=0.5, verbose=False, device_run=True, nparts=2)
    assert fs._engine is before  # no handle was created
    assert not (d / "fea_results").exists()
