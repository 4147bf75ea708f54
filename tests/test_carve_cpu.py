"""csrc/carve.hpp — IndexStage, which carves the index arrays of capi.hip's
plan uploads out of one allocation and lists their copies — through
tests/native/carve_main.cpp, a program of its own (plain host C++, under the
address and undefined-behaviour sanitizers): no device needed.

The offsets are held against the pointer arithmetic the uploads had before
they moved onto the stage, restated here: upload_amg advanced by
amg_al(size), upload_xplans by size + 1, upload_sweep and upload_amg_halo by
size."""
import os
import subprocess

import pytest

from conftest import PKG, REPO

AMG_ALIGN = 64


def amg_al(n):
    return (n + AMG_ALIGN - 1) // AMG_ALIGN * AMG_ALIGN


# (align, gap) of the stage and the old code's step past an array of n elements
SETTINGS = {
    "hierarchy": (AMG_ALIGN, 0, amg_al),
    "xplans": (1, 1, lambda n: n + 1),
    "sweep_halo": (1, 0, lambda n: n),
}

LENGTHS = [
    [0, 1, 63, 64, 65, 1000],
    [1000, 0, 65, 0, 0, 64, 1, 63, 0],
    [65, 64, 63, 1, 0, 1000, 0],
    [0],
    [0, 0, 0],
    [],
    [64, 64, 1, 1, 0, 63, 1000, 65, 0, 1],
    [65, "r1"],              # upload_sweep / upload_amg_halo: one element past the lists
    [0, "r1"],
    ["r63", 1, "r0", "r65", 64],
]


def _n(item):
    return int(str(item).lstrip("r"))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("carve") / "carve_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                    os.path.join(REPO, "tests", "native", "carve_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def results(program):
    cases = [(name, items) for name in SETTINGS for items in LENGTHS]
    text = "".join("%d %d %s\n" % (SETTINGS[name][0], SETTINGS[name][1], " ".join(map(str, items)))
                   for name, items in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr)
    lines = r.stdout.split("\n")
    assert len(lines) == 3 * len(cases) + 2
    # a fill that places more than was counted shows: offset() 4 against size() 3
    assert lines[0] == "overrun 4 3"
    out = []
    for k, case in enumerate(cases):
        sized, end, size = (int(x) for x in lines[3 * k + 1].split())
        out.append((case, sized, end, size, [int(x) for x in lines[3 * k + 2].split()],
                    [int(x) for x in lines[3 * k + 3].split()]))
    return out


def test_sizing_pass_total_is_the_fills_end(results):
    for case, sized, end, size, _, mem in results:
        assert sized == end == size == len(mem), case


def test_offsets_are_the_old_pointer_arithmetic(results):
    for (name, items), _, end, _, offs, _ in results:
        step = SETTINGS[name][2]
        want, at = [], 0
        for item in items:
            want.append(at)
            at += step(_n(item))
        assert offs == want and end == at, (name, items)


def test_copy_list_puts_each_vector_at_its_offset_and_nothing_else(results):
    """(the memory held -1 before the copies: pads, gaps and reserved elements
    are not written, as the uploads never wrote them.  The stage keeps no host
    mirror — DESIGN.md §3.1 — so this stands where a mirror's "zeros in every
    pad" would have been checked.)"""
    for (name, items), _, _, _, offs, mem in results:
        want = [-1] * len(mem)
        for k, (item, at) in enumerate(zip(items, offs)):
            if not str(item).startswith("r"):
                want[at:at + _n(item)] = [(k + 1) * 100000 + i + 1 for i in range(_n(item))]
        assert mem == want, (name, items)


def test_empty_vectors_keep_the_old_offsets(results):
    """An empty list's pointer was the running pointer: with the exchange
    plans' gap of 1 every list, empty or not, has an element of its own
    (distinct offsets, all inside the allocation); without a gap an empty
    list shares the next list's offset and, when last, points one past the
    arrays — inside the allocation, which upload_sweep and upload_amg_halo
    make one element longer (reserve(1)) and upload_amg at least one long."""
    for (name, items), _, _, size, offs, _ in results:
        if name == "xplans":
            assert len(set(offs)) == len(offs) and all(o < size for o in offs), items
        else:
            assert all(o <= size for o in offs), (name, items)
            for k in range(len(items) - 1):
                assert (offs[k + 1] == offs[k]) == (_n(items[k]) == 0), (name, items)
            if items and str(items[-1]) == "r1":
                assert all(o < size for o in offs), (name, items)
