"""The option table behind mfea_set_option / mfea_get_option (csrc/options.cpp)
through its two handle-free entries, mfea_debug_option_info and
mfea_debug_option_check: no device needed.

tests/golden/option_domains.json holds what the library of the commit before
the table (its hash is in the file) answered on a GPU, on a fresh handle, for
every writable option and probe value — "EINVAL" or the mfea_get_option
read-back — and every default (tools/option_domains.py)."""
import json
import os
import re

import pytest

from conftest import GOLDEN, PKG, REPO

FIXTURE = json.load(open(os.path.join(GOLDEN, "option_domains.json")))

# the 45 pinned before the table (mfea._capi.DEFAULT_OPTIONS, then written by hand) ...
DEFAULTS = {"graph": 1, "phase_times": 0, "dist_graph": 1, "order": -1, "lane_dof": 0, "cg_kernel": 0,
            "ell_block": 256, "ell_maxg": 0, "ell_compact": 1, "amg_tail_rows": 2048,
            "amg_max_levels": 32, "amg_restrict_lanes": 0, "amg_op_lanes": 0,
            "amg_tail_lds": 1, "dist_timeout_ms": 60000, "part_slack_pct": 35, "amg_dist": -1,
            "amg_rep_rows": 32768, "amg_dist_cycle": 1, "dist_sums": 1, "amg_cycle": 1, "amg_fuse_setup": 1,
            "amg_up_lanes": 0, "amg_spatial": -1, "amg_collapse": -1, "amg_collapse_mb": 32,
            "amg_collapse_pairs": 8000000, "amg_theta_ppm": 0, "amg_reuse": 1, "amg_rebuild_pct": 800,
            "amg_rebuild_rent": 100, "amg_coarse_rho_ppm": 1750000, "sweep_piece": 64, "cc_tile": 1024,
            "asm_kernel": 0, "spec_post": 1, "setup_entry": 1,
            "batch_graph": 1, "step_graph": 0,
            "graph_start": 1, "combo_graph": 1, "amg_a0_slot": 1, "run_register": 1,
            "keep_operator": 1, "event_scratch": 1,
            # ... and the ten it had not listed
            "amg_v_lanes": 0, "amg_small_lanes": 65536, "amg_merge": -1, "amg_down_split": 0, "amg_fuse_l0": -1,
            "amg_l0_window": 0, "amg_close": 1, "amg_start": 1, "amg_lazy_px": 1, "amg_big_chunk": 8}
REBUILDS_LAYOUT = {"order", "lane_dof", "ell_compact", "amg_tail_rows", "amg_max_levels", "amg_merge", "amg_collapse",
                   "amg_collapse_mb", "amg_collapse_pairs", "amg_spatial", "amg_fuse_l0", "amg_l0_window",
                   "amg_coarse_rho_ppm", "amg_a0_slot", "sweep_piece", "amg_theta_ppm", "part_slack_pct"}
KEEPS_KEPT = {"phase_times", "run_register", "amg_close", "amg_start", "amg_lazy_px", "amg_big_chunk"}
READ_ONLY = {"element_props", "run_direct", "amg_merged", "amg_merge_dq_blocks", "amg_merge_u_blocks", "sweep_colors",
             "sweep_pieces", "amg_fused_l0", "amg_l0_window_used", "amg_fuse_max_halo", "amg_fuse_halo_cap",
             "amg_safe_omega", "amg_collapse_level", "amg_collapse_blocks", "amg_spatial_chosen", "amg_reused",
             "amg_build_iters", "amg_dist_chosen", "op_kept_steps", "amg_setup_kept", "amg_px_replays", "amg_px_slots",
             "amg_start_fused", "amg_close_hits", "amg_last_cycles", "asm_colours"}


def test_the_fixture_is_whole():
    assert re.fullmatch(r"[0-9a-f]{40}", FIXTURE["commit"])
    assert len(DEFAULTS) == 55 and len(READ_ONLY) == 26
    assert set(FIXTURE["answers"]) == set(FIXTURE["defaults"]) == set(DEFAULTS)
    assert all(len(row) == len(FIXTURE["probes"]) for row in FIXTURE["answers"].values())


def test_enumeration_lists_the_writable_options_then_the_read_only_names():
    from mfea import _capi
    info = _capi.option_info()
    names = [n for n, _, _ in info]
    assert len(names) == len(set(names)) == 55 + 26
    assert set(names[:55]) == set(FIXTURE["defaults"])
    assert all(f & _capi.OPT_WRITABLE for _, _, f in info[:55])
    assert set(names[55:]) == READ_ONLY
    assert all((d, f) == (0, 0) for _, d, f in info[55:])
    # past the end, and before the start
    n, d, f = _capi.C.c_char_p(), _capi.C.c_int64(), _capi.C.c_int()
    for index in (81, -1):
        assert _capi._lib.mfea_debug_option_info(index, _capi.C.byref(n), _capi.C.byref(d),
                                                 _capi.C.byref(f)) == _capi.EINVAL


def test_defaults():
    from mfea import _capi
    got = {n: d for n, d, f in _capi.option_info() if f & _capi.OPT_WRITABLE}
    assert got == DEFAULTS
    assert got == FIXTURE["defaults"]
    assert _capi.DEFAULT_OPTIONS == DEFAULTS
    assert list(_capi.DEFAULT_OPTIONS) == [n for n, _, _ in _capi.option_info()[:55]]  # table order


def test_layout_and_keeps_kept_flags():
    from mfea import _capi
    info = _capi.option_info()
    assert {n for n, _, f in info if f & _capi.OPT_REBUILDS_LAYOUT} == REBUILDS_LAYOUT
    assert {n for n, _, f in info if f & _capi.OPT_KEEPS_KEPT} == KEEPS_KEPT


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_accepted_values_and_read_backs_are_the_parent_commits(name):
    from mfea import _capi
    for probe, want in zip(FIXTURE["probes"], FIXTURE["answers"][name]):
        try:
            got = _capi.option_check(name, probe)
        except _capi.MfeaError as e:
            assert e.code == _capi.EINVAL
            assert name in str(e)  # the message names the option (and its legal values)
            got = "EINVAL"
        assert got == want, (name, probe)


@pytest.mark.parametrize("name", sorted(READ_ONLY) + ["no_such_option"])
def test_read_only_and_unknown_names_cannot_be_set(name):
    from mfea import _capi
    with pytest.raises(_capi.MfeaError, match="unknown option " + name) as ei:
        _capi.option_check(name, 0)
    assert ei.value.code == _capi.EINVAL


def test_abi_version_and_header():
    from mfea import _capi
    assert _capi.abi_version() == 8
    header = open(os.path.join(REPO, "include", "mfea_debug.h")).read()
    assert "#define MFEA_ABI_VERSION 8" in open(os.path.join(REPO, "include", "mfea.h")).read()
    for name in DEFAULTS:
        assert f'"{name}"' in header, name
    for name in ("mfea_debug_option_info", "mfea_debug_option_check"):
        assert name in _capi.EXPORTED and hasattr(_capi._lib, name)


def test_table_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/options.cpp with tests/native/options_main.cpp as a program of its
    own (plain host C++), every fixture probe through its check and store."""
    import subprocess
    exe = str(tmp_path / "options_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(PKG, "csrc", "options.cpp"),
                    os.path.join(REPO, "tests", "native", "options_main.cpp"), "-o", exe], check=True)
    lines = [f"{name} {probe} {want}\n" for name, row in FIXTURE["answers"].items()
             for probe, want in zip(FIXTURE["probes"], row)]
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr)
    assert r.stdout.split() == ["ok", "55", str(len(lines))]
