"""What the strain-energy tests share (tests/test_energy_cpu.py,
tests/test_gpu_energy.py): the NumPy restatement of include/mfea.h's operation
table, the input file of tests/native/energy_main.cpp, the 4x property recipe
and the oracle's heterogeneous direct solve.  Checker code only."""
import os
import subprocess

import numpy as np

from conftest import PKG, REPO, load_mesh

import fea_oracle as fo  # noqa: E402  (checker only)
from test_gpu_grip_motion import known_map  # noqa: E402
from test_gpu_props import het_K  # noqa: E402

X, SIM3D, PLANAR = "test_X", "sim_20251115_135507", "sim_20251117_175809"
MESHES = (X, SIM3D, PLANAR)
GRIP = {X: 0.5, PLANAR: 1.5, SIM3D: 0.5}
EX, EY = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
MIX2 = (0.6, 0.8, 0.0)
# (top direction, bottom direction): tensile, shear, unequal grip vectors
MOTIONS = {"tensile": (EY, EY), "shear": (EX, EX), "unequal": (MIX2, EY)}
AMP = 0.01

_meshes, _solved = {}, {}


def mesh_of(name):
    if name not in _meshes:
        nodes, elems = load_mesh(name)
        xyz = np.ascontiguousarray(nodes[["x", "y", "z"]].values, dtype=np.float64)
        e2n = elems[["n1", "n2"]].values.astype(np.int64)
        top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, GRIP[name])
        _meshes[name] = (xyz, e2n, top, bot)
    return _meshes[name]


def props4(n, seed=5):
    """E, A and I each spread over 4x (0.5 ... 2 times the scalar), independently."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (3, n)))
    return {"E": fo.E_MOD * s[0], "A": fo.AREA * s[1], "I": fo.INERTIA * s[2]}


# These networks are sparse: a random tenth of the elements off separates the
# two larger samples more often than not (W falls from ~1e-10 to the ~1e-18 the
# regularisation leaves, and a relative comparison means nothing).  The seeds
# below leave every sample carrying load under all three grip motions.
MASK_SEED = {X: 3, SIM3D: 3, PLANAR: 5}
LOADED = 1e-12  # a strain energy above this is a sample that carries load at AMP


def tenth_off(name):
    """The mesh's activity mask with a tenth of the elements off."""
    n = len(mesh_of(name)[1])
    act = np.ones(n, dtype=bool)
    act[np.random.default_rng(MASK_SEED[name]).choice(n, size=max(1, n // 10), replace=False)] = False
    return act


def sections(props):
    """(EA_e, EI12_e) with mfea_set_material's expressions and rounding."""
    return props["E"] * props["A"], (12.0 * props["E"]) * props["I"]


def restate(xyz, e2n, U, EA, EI12, active, cube=None):
    """include/mfea.h's table in NumPy, one ufunc call per operation: returns
    (w_axial, w_bending, g_axial, g_bending).  NumPy has no fma: Ls^3 is
    (Ls*Ls)*Ls here unless `cube` supplies it."""
    xyz = np.asarray(xyz, dtype=np.float64)
    U3 = np.asarray(U, dtype=np.float64).reshape(-1, 3)
    a, b = e2n[:, 0], e2n[:, 1]
    v = xyz[b] - xyz[a]
    L = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    Ls = np.where(L < 1e-12, 1e-12, L)
    n = v / Ls[:, None]
    dl = U3[b] - U3[a]
    d = (n[:, 0] * dl[:, 0] + n[:, 1] * dl[:, 1]) + n[:, 2] * dl[:, 2]
    t = dl - d[:, None] * n
    q = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    g_ax = ((0.5 * d) * d) / Ls
    g_b = (0.5 * q) / ((Ls * Ls) * Ls if cube is None else cube(Ls))
    off = ~np.asarray(active, dtype=bool)
    w_ax, w_b = EA * g_ax, EI12 * g_b
    for r in (w_ax, w_b, g_ax, g_b):
        r[off] = 0.0
    return w_ax, w_b, g_ax, g_b


def direct(name, motion, props, active, dy_top=AMP, dy_bot=-AMP):
    """(K, U, known, vals): the oracle's heterogeneous K of the active elements
    and its direct solve under the named grip motion, once per case."""
    key = (name, motion, dy_top, dy_bot, tuple(props[k].tobytes() for k in ("E", "A", "I")), active.tobytes())
    if key not in _solved:
        xyz, e2n, top, bot = mesh_of(name)
        t, b = MOTIONS[motion]
        K = het_K(xyz, e2n, active, props["E"], props["A"], props["I"]).tocsr()
        known, vals = known_map(top, bot, dy_top, dy_bot, t, b)
        _solved[key] = (K, fo.solve_system(K, known, vals), known, vals)
    return _solved[key]


def build_energy_main(out_dir, sanitize):
    """tests/native/energy_main.cpp with g++, at the library's contraction
    setting; sanitize: under the address and undefined-behaviour sanitizers."""
    exe = os.path.join(str(out_dir), "energy_main_san" if sanitize else "energy_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *san, "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tests", "native", "energy_main.cpp"),
                    "-o", exe], check=True)
    return exe


def records(xyz, e2n, U, EA, EI12, active):
    """energy_main's input records, one row of 15 doubles per element."""
    xyz = np.asarray(xyz, dtype=np.float64)
    U3 = np.asarray(U, dtype=np.float64).reshape(-1, 3)
    a, b = e2n[:, 0], e2n[:, 1]
    n = len(e2n)
    return np.concatenate([xyz[a], xyz[b], U3[a], U3[b], np.broadcast_to(EA, (n,))[:, None],
                           np.broadcast_to(EI12, (n,))[:, None],
                           np.asarray(active, dtype=np.float64)[:, None]], axis=1)


def run_energy_main(exe, rec, work_dir):
    """The four rows energy_main computes for the records."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    src, dst = os.path.join(str(work_dir), "energy.in"), os.path.join(str(work_dir), "energy.out")
    with open(src, "wb") as f:
        f.write(np.int64(len(rec)).tobytes())
        f.write(rec.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    out = np.fromfile(dst, dtype=np.float64).reshape(4, len(rec))
    return out[0], out[1], out[2], out[3]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
