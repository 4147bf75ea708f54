"""csrc/solve_plan.hpp — the captured chunk graphs' key and the chunk lengths
of a planned batch — through tests/native/solve_plan_main.cpp, a program of
its own (plain host C++, under the address and undefined-behaviour
sanitizers): no device needed.

The chunk lengths are held against the formulas of the solve drivers in
csrc/capi.hip, restated here: drive_sized's, and, for chunks of one size,
drive_planned's.  (capi.hip does not call the header yet.)"""
import os
import subprocess

import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solve_plan") / "solve_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "native", "solve_plan_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, cases):
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr)
    lines = r.stdout.splitlines()
    keys = [tuple(ln.split()[1:]) for ln in lines if ln.startswith("key ")]
    lists = [[int(x) for x in ln.split()] for ln in lines if not ln.startswith("key ")]
    assert len(lists) == len(cases)
    return keys, lists


def sized_in_capi(big, small, need, exact_rem, zero_ok):
    """drive_sized's queueing, need = expected + 1 before its clamp."""
    need = max(0 if zero_ok else 1, need)
    out = [0] if need == 0 else []
    nbig = need // big if big > small else 0
    rem = need - nbig * big
    nsmall = (rem + small - 1) // small
    out += [big] * nbig
    if exact_rem and rem > 0:
        out.append(rem)
    else:
        out += [small] * nsmall
    return out


def planned_in_capi(chunk, need):
    """drive_planned's first batch, need = expected + 1 (below its bound of
    max_it / chunk + 3 chunks, which the driver applies itself)."""
    return [chunk] * max(1, (need + chunk - 1) // chunk)


CASES = [(big, small, need, er, zo) for big in range(2, 17) for small in (2, 4) for need in range(0, 71)
         for er in (0, 1) for zo in (0, 1)]


def test_chunk_lengths_are_drive_sized_formulas(program):
    _, got = _run(program, CASES)
    for case, lens in zip(CASES, got):
        assert lens == sized_in_capi(*case), case
    # what the formulas promise, stated on the lists themselves
    for (big, small, need, er, zo), lens in zip(CASES, got):
        need = max(0 if zo else 1, need)
        assert need <= sum(lens) < need + small, (big, small, need, er, zo)
        assert lens == [0] or all(n > 0 for n in lens)
        if er:
            assert sum(lens) == need


def test_one_size_is_drive_planned(program):
    cases = [(c, c, need, 0, 0) for c in (2, 4, 6, 8, 32) for need in range(0, 71)]
    _, got = _run(program, cases)
    for (c, _, need, _, _), lens in zip(cases, got):
        assert lens == planned_in_capi(c, need), (c, need)


def test_chunk_keys_differ_when_any_one_field_does(program):
    keys, _ = _run(program, [])
    names = [k for k, _ in keys]
    assert names == ["same"] + ["path"] * 5 + ["chunk", "precond", "lanes", "gen", "gen_folded", "gen_high", "close",
                                               "lazy", "default"]
    for name, equal in keys:
        assert equal == ("1" if name == "same" else "0"), name
