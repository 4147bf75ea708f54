"""csrc/bc_form.hpp — the boundary forms' dispatch (with_grip / with_bc) and the
staging of a per-node vector array (mfea_set_grip_field, mfea_set_node_loads) —
through tests/native/bc_form_main.cpp, a program of its own (plain host C++,
under the address and undefined-behaviour sanitizers): no device needed."""
import itertools
import os
import struct
import subprocess

import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bc_form") / "bc_form_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "native", "bc_form_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr)
    return r.stdout.splitlines()


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def vec(xs):
    return " ".join(["%d" % len(xs)] + [bits(x) for x in xs])


def stage(exe, cur_set, cur, src):
    """→ (verdict, staged bit patterns); src None: a NULL source."""
    line = "stage %d %s %d %s" % (cur_set, vec(cur), src is not None, vec(src or []))
    out = _run(exe, [line])[0].split()
    assert out[0] == "stage"
    return out[1], out[2:]


def test_every_pointer_combination_calls_once_with_its_pair(program):
    combos = list(itertools.product((0, 1), repeat=3))
    out = _run(program, ["form %d %d %d" % c for c in combos])
    assert len(out) == 2 * len(combos) == 16
    for k, (g, f, l) in enumerate(combos):
        gm = "GripField same" if f else ("GripVec same" if g else "GripY -")  # field wins over grip
        ld = "NodeLoad same" if l else "LoadNone -"
        assert out[2 * k] == "bc 1 %s %s" % (gm, ld), (g, f, l)
        assert out[2 * k + 1] == "grip 1 %s" % gm, (g, f, l)


@pytest.mark.parametrize("nodes", [1, 3])
def test_non_finite_entries_are_rejected_at_every_position(program, nodes):
    n = 3 * nodes
    good = [0.5 * (k + 1) for k in range(n)]
    for at in sorted({0, n // 2, n - 1}):
        for bad in (float("nan"), float("inf"), float("-inf")):
            src = list(good)
            src[at] = bad
            assert stage(program, 0, [], src)[0] == "notfinite", (at, bad)
            assert stage(program, 1, good, src)[0] == "notfinite", (at, bad)
    assert stage(program, 0, [], good) == ("new", [bits(x) for x in good])


def test_negative_zero_is_stored_as_zero(program):
    src = [-0.0, 1.0, -0.0, -2.0, 0.0, -0.0, 3.0, -0.0, -0.0]
    verdict, staged = stage(program, 0, [], src)
    assert verdict == "new"
    assert staged == [bits(0.0) if x == 0.0 else bits(x) for x in src]
    assert bits(-0.0) != bits(0.0) and bits(-0.0) not in staged
    # ... and a −0 source equals a stored 0: the state is the normalised one
    assert stage(program, 1, [0.0 if x == 0.0 else x for x in src], src)[0] == "same"


@pytest.mark.parametrize("nodes", [1, 3])
def test_same_exactly_when_every_byte_is_equal(program, nodes):
    n = 3 * nodes
    cur = [1.0 + 0.25 * k for k in range(n)]
    assert stage(program, 1, cur, list(cur))[0] == "same"
    for at in range(n):  # one bit anywhere is another state
        src = list(cur)
        src[at] = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", cur[at]))[0] ^ 1))[0]
        assert src[at] != cur[at]
        assert stage(program, 1, cur, src)[0] == "new", at
    assert stage(program, 1, cur, None) == ("new", [])  # set → unset
    assert stage(program, 0, [], list(cur))[0] == "new"  # unset → set, whatever the values
    assert stage(program, 0, [], None) == ("same", [])  # unset stays unset


def test_no_nodes(program):
    assert stage(program, 0, [], None) == ("same", [])
    assert stage(program, 0, [], []) == ("new", [])  # an empty array given: set, with nothing in it
    assert stage(program, 1, [], []) == ("same", [])
    assert stage(program, 1, [], None) == ("new", [])
    assert _run(program, ["z 0"]) == ["z 0"]


def test_z_detection_reads_the_third_components_only(program):
    for nodes in (1, 3):
        n = 3 * nodes
        for at in range(n):
            v = [0.0] * n
            v[at] = -1e-300
            assert _run(program, ["z " + vec(v)]) == ["z %d" % (at % 3 == 2)], (nodes, at)
        assert _run(program, ["z " + vec([1.0, 2.0, 0.0] * nodes)]) == ["z 0"]
        assert _run(program, ["z " + vec([1.0, 2.0, -0.0] * nodes)]) == ["z 0"]
