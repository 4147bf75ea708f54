"""Drop-in replacement for the reference's ``src/fea_solver.py`` on MI355X.

Same module constants, same functions, same CLI and the same ``fea_results/``
CSV outputs; the hot path (element stiffness, global assembly, Dirichlet
elimination, the linear solve, reactions and the stress/failure update) runs in
libmfea.so's HIP kernels.  Run it exactly like the reference:

    python mycelium-fea-project_amd/fea_solver.py <results_dir> [options]

Differences by design: the direct SuperLU solve
(src/fea_solver.py:128) is replaced by device PCG preconditioned with a
smoothed-aggregation AMG V-cycle (the reference sweep's `-pc_type gamg`; Jacobi
and block Jacobi on request) run to a tight relative residual (default 1e-13 →
displacement within ~1e-10 relative L2 of the direct solution); PNG plotting
(plot_network, py:137-181) is out of scope.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import pandas as pd
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mfea import _capi  # noqa: E402  (fails loudly when libmfea.so is missing)

# ----------------------------------------------------------------------------
# Material & Simulation Parameters — src/fea_solver.py:14-28 (π = 3.14 as there)
# ----------------------------------------------------------------------------
E_mod = 2500
d = 0.0002
t = 0.000001
A = 3.14 * ((d / 2) ** 2 - (d / 2 - t) ** 2)
I = A * 0.001  # noqa: E741  (reference name)
N_STEPS = 40
DISPLACEMENT_MAX = 0.02
MAX_STRAIN = 0.018
MAX_STRESS = E_mod * MAX_STRAIN
GRIP_LENGTH = 1.5

# solver settings of the device PCG (no counterpart in the direct-solve reference)
RTOL = 1e-13
MAX_IT = 200000
PRECOND = _capi.PC_GAMG  # partitioned runs: the distributed V-cycle of one global hierarchy
REG = 1e-12  # src/fea_solver.py:125

_engine = None
_world_joined = False


def get_engine(device: int | None = None) -> _capi.Engine:
    """Process-wide device handle (device = LOCAL_RANK or 0)."""
    global _engine
    if _engine is None:
        dev = int(os.environ.get("LOCAL_RANK", "0")) if device is None else device
        _engine = _capi.Engine(dev)
    return _engine


def dist_env():
    """(rank, world) of a multi-process launch — ``python -m torch.distributed.run
    --nproc-per-node N fea_solver.py <dir>``, one process per GPU, as the
    reference's ``mpirun -np N fea_petsc_parallel.exe <dir>`` (README.md:18;
    rank/size src/fea_petsc_parallel.cpp:169-171) — else (0, 1)."""
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def _join_world(eng, rank, world):
    """Joins this process's handle to the RCCL world: rank 0 makes the
    communicator id, torch.distributed (gloo, launcher plumbing only) carries
    it to the other ranks.  Once per process."""
    global _world_joined
    if _world_joined:
        return
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("gloo")
    obj = [_capi.dist_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    eng.dist_init(rank, world, obj[0])
    _world_joined = True


def gather_records(node_owned, elem_owned, U, stress, active, rank, world):
    """One step's records of the whole mesh on rank 0: every node's U from the
    rank owning the node, every element's stress / activity from the rank
    owning it (its first node's).  The values travel as they are (a -0.0
    displacement stays -0.0 in the CSV, which a sum-reduction would not keep).
    Replaces the reference's VecScatterCreateToZero + MPI_Bcast of U
    (src/fea_petsc_parallel.cpp:373-391); returns None on the other ranks."""
    import torch.distributed as dist
    U3 = np.asarray(U).reshape(-1, 3)
    payload = (np.flatnonzero(node_owned), U3[node_owned], np.flatnonzero(elem_owned),
               np.asarray(stress)[elem_owned], np.asarray(active)[elem_owned])
    out = [None] * world if rank == 0 else None
    dist.gather_object(payload, out, dst=0)
    if rank != 0:
        return None
    Ug, Sg, Ag = np.zeros_like(U3), np.zeros(len(stress)), np.ones(len(active), dtype=bool)
    seen_n, seen_e = np.zeros(len(U3), bool), np.zeros(len(stress), bool)
    for ni, uv, ei, sv, av in out:
        Ug[ni], Sg[ei], Ag[ei] = uv, sv, av
        seen_n[ni] = True
        seen_e[ei] = True
    if not (seen_n.all() and seen_e.all()):
        raise RuntimeError("record gather: a node or element is owned by no rank")
    return Ug.reshape(-1), Sg, Ag


def _opts(rtol=None, max_it=None, precond=None):
    return _capi.make_opts(rtol=RTOL if rtol is None else rtol,
                           max_it=MAX_IT if max_it is None else max_it,
                           precond=PRECOND if precond is None else precond, reg=REG)


def bar_stiffness_bulk(p1s, p2s, E=E_mod, A=A, I=I):  # noqa: E741
    """Element stiffness (N,6,6) and length (N,), src/fea_solver.py:30-68, on device."""
    return get_engine().element_stiffness(p1s, p2s, E, A, I)


def _elem_array(elems):
    if isinstance(elems, pd.DataFrame):
        return elems[["n1", "n2"]].values.astype(np.int64)
    return np.asarray(elems, dtype=np.int64).reshape(-1, 2)


def assemble_global_stiffness(coords, elems, active):
    """Global K as scipy CSR (3N×3N), src/fea_solver.py:74-106, assembled on device.

    Same sparsity pattern as the reference's csr_matrix (explicit zeros kept,
    duplicates summed in element order)."""
    coords = np.asarray(coords, dtype=np.float64)
    e2n = _elem_array(elems)
    eng = _capi.Engine(get_engine_device())
    try:
        eng.set_material(E_mod, A, I)
        eng.set_mesh(coords, e2n)
        eng.set_bc(np.zeros(0, np.int64), np.zeros(0, np.int64))
        eng.set_active(np.asarray(active, dtype=bool))
        eng.assemble()
        indptr, indices, data = eng.export_csr()
    finally:
        eng.close()
    n = 3 * coords.shape[0]
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def get_engine_device():
    return int(os.environ.get("LOCAL_RANK", "0"))


def solve_system(K, known_dofs, known_vals):
    """Dirichlet elimination + solve of an arbitrary K, src/fea_solver.py:112-135.

    K_ff + 1e-12·I solved by device Jacobi-PCG (rtol RTOL); raises
    np.linalg.LinAlgError (a SolverFailure) if it does not converge."""
    K = sp.csr_matrix(K)
    U, _ = get_engine().solve_csr(K.indptr, K.indices, K.data, known_dofs, known_vals,
                                  _opts(precond=_capi.PC_JACOBI))
    return U


def _grips(nodes, coords, tol):
    """src/fea_solver.py:207-210."""
    y_min, y_max = coords[:, 1].min(), coords[:, 1].max()
    top = nodes.loc[np.abs(nodes["y"] - y_max) < tol, "node_id"].values.astype(int)
    bot = nodes.loc[np.abs(nodes["y"] - y_min) < tol, "node_id"].values.astype(int)
    return top, bot


PROP_COLUMNS = ("E", "A", "I", "max_strain")


def read_element_props(path, n_elems):
    """A per-element property file: CSV with a header, ``elem_id`` plus any
    subset of E, A, I, max_strain; every element id 0 … n_elems − 1 exactly
    once, in any order.  Returns {column: float64 array in element order}
    (Engine.set_element_props's arguments); ValueError names what is wrong."""
    df = pd.read_csv(path, float_precision="round_trip")  # (the values the file's digits stand for)
    if "elem_id" not in df.columns:
        raise ValueError(f"{path}: no elem_id column")
    unknown = [c for c in df.columns if c != "elem_id" and c not in PROP_COLUMNS]
    if unknown:
        raise ValueError(f"{path}: unknown column(s) {unknown}; expected elem_id and any of {list(PROP_COLUMNS)}")
    ids_f = df["elem_id"].values.astype(np.float64)
    if not (np.isfinite(ids_f).all() and (ids_f == np.floor(ids_f)).all()):
        raise ValueError(f"{path}: elem_id must hold integers")
    ids = ids_f.astype(np.int64)
    bad = ids[(ids < 0) | (ids >= n_elems)]
    if bad.size:
        raise ValueError(f"{path}: element id {int(bad[0])} outside 0..{n_elems - 1}")
    count = np.bincount(ids, minlength=n_elems)
    if (count > 1).any():
        raise ValueError(f"{path}: duplicate element id {int(np.flatnonzero(count > 1)[0])}")
    if (count == 0).any():
        raise ValueError(f"{path}: missing element id {int(np.flatnonzero(count == 0)[0])} "
                         f"({int((count == 0).sum())} of {n_elems} missing)")
    out = {}
    for c in PROP_COLUMNS:
        if c in df.columns:
            col = np.empty(n_elems, dtype=np.float64)
            col[ids] = df[c].values.astype(np.float64)
            out[c] = col
    return out


def parse_grip_direction(text):
    """``TX,TY,TZ[/BX,BY,BZ]``: the direction of the top grip's motion and, after
    the slash, of the bottom grip's (without it: the same as the top's, so that
    the opposite amplitudes of the ramp shear the network along one axis).
    Returns (top, bot), two float64 arrays of three components
    (Engine.set_grip_motion's arguments); ValueError names what is wrong."""
    parts = str(text).split("/")
    if len(parts) > 2:
        raise ValueError(f"{text!r}: at most one '/' (TX,TY,TZ[/BX,BY,BZ])")
    vecs = []
    for name, part in zip(("top", "bottom"), parts):
        fields = part.split(",")
        if len(fields) != 3:
            raise ValueError(f"{text!r}: the {name} direction needs three components, got {len(fields)}")
        try:
            v = np.array([float(f) for f in fields], dtype=np.float64)
        except ValueError:
            raise ValueError(f"{text!r}: the {name} direction holds something that is not a number") from None
        if not np.isfinite(v).all():
            raise ValueError(f"{text!r}: the {name} direction must be finite")
        if not v.any():
            raise ValueError(f"{text!r}: the {name} direction must not be all zero")
        vecs.append(v)
    return vecs[0], (vecs[1] if len(vecs) == 2 else vecs[0].copy())


TENSILE = (0.0, 1.0, 0.0)


def complete_grip_field(grip_field, n_nodes, top, bot, grip_direction=None):
    """The n_nodes x 3 field Engine.set_grip_field takes, from fea_solver's
    grip_field argument: a CSV path (mfea.fields.read_csv), a (field, listed)
    pair, or an n_nodes x 3 array (every node listed).  A grip node that is not
    listed takes its band's direction vector — grip_direction's, or the tensile
    default; a node in both bands the bottom one's."""
    from mfea import fields
    if isinstance(grip_field, (str, os.PathLike)):
        grip_field = fields.read_csv(grip_field, n_nodes)
    if isinstance(grip_field, tuple):
        field, listed = grip_field
    else:
        field, listed = grip_field, np.ones(n_nodes, dtype=bool)
    field = np.array(field, dtype=np.float64).reshape(-1, 3)
    listed = np.asarray(listed, dtype=bool).ravel()
    if field.shape[0] != n_nodes or listed.size != n_nodes:
        raise ValueError(f"grip_field must have one row per node ({n_nodes})")
    vt, vb = grip_direction if grip_direction is not None else (TENSILE, TENSILE)
    for nodes, vec in ((top, vt), (bot, vb)):  # (bottom last: it wins)
        nodes = np.asarray(nodes, dtype=np.int64)
        rest = nodes[~listed[nodes]]
        field[rest] = np.asarray(vec, dtype=np.float64)
    return field


def fea_solver(results_dir, tol=GRIP_LENGTH, *, rtol=None, max_it=None, precond=None,
               out_format="python", verbose=True, nparts=1, npy=False, device_run=False,
               events=False, tie_rtol=1e-9, max_events=None, element_props=None, grip_direction=None,
               energy=False, grip_field=None, node_loads=None, load_mode="dead"):
    """The reference step loop (src/fea_solver.py:186-335) with the hot path on device.

    Reads <results_dir>/nodes.csv + elements.csv, runs N_STEPS load steps and
    writes <results_dir>/fea_results/{stress_record,active_elements,
    node_displacements,force_displacement}.csv, runtime.txt and
    solve_runtime.txt.  Module constants are read at call time, as in the
    reference.  out_format='petsc' writes the fea_petsc.cpp formatting instead
    (src/fea_petsc.cpp:433-516).  npy=True also writes every record as a .npy
    sidecar next to its CSV (the raw per-step array, no step column).

    Multi-GPU: launched as N processes (``torch.distributed.run``, dist_env),
    every rank solves its partition of the mesh (RCCL between the GPUs) and
    rank 0 alone gathers the records and writes the files — the reference's
    MPI variant has every rank write the same files (src/fea_petsc_parallel.cpp:
    491-574).  nparts > 1 in ONE process runs that partitioned solve with its
    partitions all on this device (mfea_debug_set_parts).

    device_run=True (one process, one partition) runs the step loop as ONE
    library call (Engine.run / mfea_run): every step's records are gathered on
    the device and copied out while the next step computes.  Same files, same
    returned dict; the per-step progress lines are printed after the run.

    events=True (one process, one partition) replaces the fixed ramp by the
    event-driven run (Engine.run_events / mfea_run_events): one solve at the
    reference load ±DISPLACEMENT_MAX per failure event, each break at its exact
    load factor lam (lam_max = 1: the test's full travel), elements within
    tie_rtol of the largest strain breaking together, at most max_events
    events (default n_elems + 1).  The four records hold one row per event —
    the state at the failure load; force_displacement.csv holds (lam·span,
    lam·F₁) — and failure_events.csv lists event, lam, total_displacement,
    total_force, n_failed, n_active.  npy=True also writes event_of.npy (the
    event that failed each element, -1 = none).

    element_props (one process, one partition): a property file
    (read_element_props) or a dict of per-element arrays E, A, I, max_strain —
    a heterogeneous network (Engine.set_element_props); the columns not given
    stay the module's constants.  Works with the ramp, device_run and events;
    the record files and their formats do not change.

    grip_direction (one process, one partition): a ``TX,TY,TZ[/BX,BY,BZ]`` string
    (parse_grip_direction) or a (top, bot) pair of 3-vectors — the grips move
    along them (Engine.set_grip_motion), dy_top / dy_bot being the amplitudes:
    a shear or mixed-mode test.  None: the tensile test along y.  Works with the
    ramp, device_run, events and element_props; force_displacement.csv keeps its
    two columns, the amplitude span and the work-conjugate force.

    grip_field (one process, one partition): a CSV file with the columns
    node_id,dx,dy,dz (mfea.fields.read_csv), a (field, listed) pair or an
    n_nodes x 3 array — a prescribed vector per grip node
    (Engine.set_grip_field): grip node n moves by amplitude · d_n, the amplitude
    being dy_top, or dy_bot for a bottom node.  A grip rotation, an affine
    boundary displacement, an indentation.  Grip nodes the file does not list
    take their band's direction vector (grip_direction's, or the tensile
    default); free nodes it lists are ignored.  Works with the ramp, device_run,
    events, element_props, energy and grip_direction.  force_displacement.csv
    keeps total_displacement = dy_top − dy_bot; total_force is the generalised
    force of the top band, Σ d_n·(K U)_n over its nodes.

    node_loads (one process, one partition): a CSV file with the columns
    node_id,fx,fy,fz (mfea.loads.read_csv) or an n_nodes x 3 array — a force on
    every free node listed (Engine.set_node_loads); grip nodes listed are
    ignored, and the load on a piece cut off from both grips is dropped.
    load_mode "dead": the load as given at every step; "proportional": dy_top
    times it.  Works with the ramp, device_run, element_props, grip_direction,
    grip_field and energy; with events only in proportional mode (a dead load
    makes the response affine in the load factor).  The records keep their
    meaning: total_force is the reaction of the top band.

    energy=True (one process, one partition): the strain energy of every record
    row, split into its axial and bending parts (Engine.energy /
    mfea_get_energy), each row on the activity its K was assembled from — the
    one BEFORE the step's or event's failures.  The per-step path asks after
    every step; device_run and events ask once per recorded row afterwards,
    with U row k and activity row k − 1 (an event's U row is lam_k·U₁, so its
    energy is that at the failure load).  Writes energy.csv (step,
    total_displacement, axial_energy, bending_energy) and
    element_energy_axial.csv / element_energy_bending.csv in the stress
    record's layout and out_format (.npy sidecars with npy); the returned dict
    gains "energy" (rows × 2), "w_axial" and "w_bending"."""
    start_time = time.time()
    rank, world = dist_env()
    if energy and (world > 1 or nparts > 1):
        raise ValueError("energy needs one process and one partition (world == 1, nparts == 1)")
    if grip_direction is not None and (world > 1 or nparts > 1):
        raise ValueError("grip_direction needs one process and one partition (world == 1, nparts == 1)")
    if isinstance(grip_direction, str):
        grip_direction = parse_grip_direction(grip_direction)
    if grip_field is not None and (world > 1 or nparts > 1):
        raise ValueError("grip_field needs one process and one partition (world == 1, nparts == 1)")
    if node_loads is not None:
        if world > 1 or nparts > 1:
            raise ValueError("node_loads needs one process and one partition (world == 1, nparts == 1)")
        if load_mode not in ("dead", "proportional"):
            raise ValueError(f"load_mode must be 'dead' or 'proportional', not {load_mode!r}")
        if events and load_mode != "proportional":
            raise ValueError("events with node_loads needs load_mode 'proportional' (a dead load makes the "
                             "response affine in the load factor)")
    if element_props is not None and (world > 1 or nparts > 1):
        raise ValueError("element_props needs one process and one partition (world == 1, nparts == 1)")
    if events and (world > 1 or nparts > 1):
        raise ValueError("events needs one process and one partition (world == 1, nparts == 1)")
    if device_run and (world > 1 or nparts > 1):
        raise ValueError("device_run needs one process and one partition (world == 1, nparts == 1)")
    say = print if verbose and rank == 0 else (lambda *a, **k: None)
    say(f"🔧 Running FEA on geometry from {results_dir}")
    fea_dir = os.path.join(results_dir, "fea_results")
    if rank == 0:
        os.makedirs(fea_dir, exist_ok=True)
    nodes = pd.read_csv(os.path.join(results_dir, "nodes.csv"))
    elems = pd.read_csv(os.path.join(results_dir, "elements.csv"))
    coords = nodes[["x", "y", "z"]].values
    n_nodes = len(nodes)
    n_elems = len(elems)
    e2n = _elem_array(elems)
    if n_elems and (e2n.min() < 0 or e2n.max() >= n_nodes):
        # the reference fails here with an IndexError from coords[...] (py:82-83)
        raise IndexError("elements.csv references a node id outside nodes.csv")

    top, bot = _grips(nodes, coords, tol)
    say(f"Top nodes: {len(top)}, Bottom nodes: {len(bot)}")

    eng = get_engine()
    if world > 1:
        _join_world(eng, rank, world)
    else:
        eng.set_parts(nparts)
    if world == 1 and nparts == 1:  # (the process-wide handle keeps its directions: always set)
        eng.set_grip_motion(*(grip_direction if grip_direction is not None else (TENSILE, TENSILE)))
    eng.set_material(E_mod, A, I)
    eng.set_mesh(coords, e2n)
    eng.set_bc(top, bot)
    eng.set_active(None)
    if grip_field is not None:  # (set_mesh cleared the one the process-wide handle may have held)
        eng.set_grip_field(complete_grip_field(grip_field, n_nodes, top, bot, grip_direction))
    if node_loads is not None:  # (set_mesh cleared the ones the process-wide handle may have held)
        from mfea import loads as _loads
        if isinstance(node_loads, (str, os.PathLike)):
            node_loads = _loads.read_csv(node_loads, n_nodes)
        node_loads = np.asarray(node_loads, dtype=np.float64)
        if node_loads.size != 3 * n_nodes:
            raise ValueError(f"node_loads must have one row per node ({n_nodes})")
        eng.set_node_loads(node_loads.reshape(n_nodes, 3), load_mode)
    if element_props is not None:
        props = (element_props if isinstance(element_props, dict)
                 else read_element_props(element_props, n_elems))
        eng.set_element_props(**{k: np.ascontiguousarray(v, dtype=np.float64) for k, v in props.items()})
    opts = _opts(rtol, max_it, precond)
    node_owned, elem_owned = eng.ownership() if world > 1 else (None, None)

    stress_record, active_record, disp_record, force_disp_curve, solve_times = [], [], [], [], []
    energy_record, wax_record, wb_record = [], [], []
    act_before = eng.active() if energy else None  # the activity the next K is assembled from
    if rank == 0:
        with open(os.path.join(fea_dir, "solve_runtime.txt"), "w") as f:
            f.write("step, runtime_s\n")
    if events:
        stress_record, active_record, disp_record, force_disp_curve = _event_run(
            eng, opts, fea_dir, say, tie_rtol, max_events, npy)
    elif device_run:
        stress_record, active_record, disp_record, force_disp_curve = _device_run(eng, opts, fea_dir, say)
    if energy and (events or device_run):
        for k in range(len(disp_record)):
            _energy_row(eng, disp_record[k], act_before if k == 0 else active_record[k - 1],
                        energy_record, wax_record, wb_record)
    for step in range(0 if device_run or events else N_STEPS):  # the per-step path
        disp_factor = step / (N_STEPS - 1)
        dy_top = +DISPLACEMENT_MAX * disp_factor
        dy_bot = -DISPLACEMENT_MAX * disp_factor
        say(f"➡️  Step {step+1}/{N_STEPS} | dy_top={dy_top:.3f}, dy_bot={dy_bot:.3f}")
        t0 = time.time()
        try:
            total_force, n_active, st = eng.step(dy_top, dy_bot, opts, MAX_STRAIN)
        except np.linalg.LinAlgError:
            say(f"❌ Singular matrix at step {step+1}. Saving partial results and stopping.")
            break
        t1 = time.time()
        solve_times.append(t1 - t0)
        if world > 1:
            rec = gather_records(node_owned, elem_owned, eng.displacement(), eng.stress(), eng.active(),
                                 rank, world)
        else:
            rec = (eng.displacement(), eng.stress(), eng.active())
        if rank == 0:
            with open(os.path.join(fea_dir, "solve_runtime.txt"), "a") as f:
                f.write(f"{step+1}, {t1 - t0:.6f}\n")
            force_disp_curve.append([dy_top - dy_bot, total_force])
            disp_record.append(rec[0])
            stress_record.append(rec[1])
            active_record.append(rec[2])
        if energy:  # the handle's U, the activity before this step's failures
            _energy_row(eng, None, act_before, energy_record, wax_record, wb_record)
            act_before = rec[2]
        if n_active == 0:
            say(f"⚠️  Simulation stopped early at step {step+1}.")
            break

    if rank == 0:
        write_records(fea_dir, n_nodes, n_elems, stress_record, active_record, disp_record,
                      force_disp_curve, out_format, npy=npy)
        if energy:
            write_energy(fea_dir, n_elems, force_disp_curve, energy_record, wax_record, wb_record, out_format,
                         npy=npy)
        say(f"✅ FEA completed. Results saved to {fea_dir}")
        total_time = time.time() - start_time
        with open(os.path.join(fea_dir, "runtime.txt"), "w") as f:
            f.write(f"Total FEA runtime: {total_time:.6f} seconds\n")
        say(f"⏱️ Total runtime: {total_time:.3f} seconds")
    res = {"force": np.asarray(force_disp_curve), "stress": np.asarray(stress_record),
           "active": np.asarray(active_record), "U": np.asarray(disp_record)}
    if energy:
        res.update(energy=np.asarray(energy_record, dtype=np.float64).reshape(-1, 2),
                   w_axial=np.asarray(wax_record), w_bending=np.asarray(wb_record))
    return res


def _energy_row(eng, U, active, energy_record, wax_record, wb_record):
    """One record row of fea_solver(energy=True): the two totals and the two
    element rows of Engine.energy(U, active), appended to the three lists."""
    en = eng.energy(U=U, active=active)
    energy_record.append([en["axial"], en["bending"]])
    wax_record.append(en["w_axial"])
    wb_record.append(en["w_bending"])


def _device_run(eng, opts, fea_dir, say):
    """The step loop of fea_solver as one library call (Engine.run / mfea_run):
    the same dy schedule, the same progress lines (printed after the run),
    solve_runtime.txt from the call's per-step wall times.  Returns the four
    records as the loop would have collected them."""
    dys = [(+DISPLACEMENT_MAX * (step / (N_STEPS - 1)), -DISPLACEMENT_MAX * (step / (N_STEPS - 1)))
           for step in range(N_STEPS)]
    run = eng.run([d[0] for d in dys], [d[1] for d in dys], opts, MAX_STRAIN)
    n_done = run["n_done"]
    with open(os.path.join(fea_dir, "solve_runtime.txt"), "a") as f:
        for step in range(n_done):
            say(f"➡️  Step {step+1}/{N_STEPS} | dy_top={dys[step][0]:.3f}, dy_bot={dys[step][1]:.3f}")
            f.write(f"{step+1}, {run['wall_s'][step]:.6f}\n")
    if run["stop_reason"] in (_capi.EMAXIT, _capi.EBREAKDOWN):
        say(f"➡️  Step {n_done+1}/{N_STEPS} | dy_top={dys[n_done][0]:.3f}, dy_bot={dys[n_done][1]:.3f}")
        say(f"❌ Singular matrix at step {n_done+1}. Saving partial results and stopping.")
    elif run["stop_reason"] == _capi.RUN_NO_ACTIVE:
        say(f"⚠️  Simulation stopped early at step {n_done}.")
    if not n_done:  # empty lists, as the loop leaves them
        return [], [], [], []
    force_disp_curve = [[dys[k][0] - dys[k][1], float(run["force"][k])] for k in range(n_done)]
    return run["stress"], run["active"], run["U"], force_disp_curve


def _event_run(eng, opts, fea_dir, say, tie_rtol, max_events, npy):
    """The event-driven failure run of fea_solver(events=True): one library
    call (Engine.run_events / mfea_run_events) at the reference load
    ±DISPLACEMENT_MAX with lam_max = 1.  Writes failure_events.csv (and
    event_of.npy with npy) and solve_runtime.txt; returns the four records, one
    row per event."""
    span = DISPLACEMENT_MAX - (-DISPLACEMENT_MAX)
    run = eng.run_events(+DISPLACEMENT_MAX, -DISPLACEMENT_MAX, opts, MAX_STRAIN, tie_rtol=tie_rtol, lam_max=1.0,
                         n_events=max_events)
    n_done = run["n_done"]
    with open(os.path.join(fea_dir, "solve_runtime.txt"), "a") as f:
        for k in range(n_done):
            say(f"➡️  Event {k+1} | lam={run['lam'][k]:.6g}, failed={run['n_failed'][k]}, "
                f"active={run['n_active'][k]}")
            f.write(f"{k+1}, {run['wall_s'][k]:.6f}\n")
    stop = run["stop_reason"]
    if stop in (_capi.EMAXIT, _capi.EBREAKDOWN):
        say(f"❌ Singular matrix at event {n_done+1}. Saving partial results and stopping.")
    elif stop == _capi.EVENTS_LAMBDA_MAX:
        say(f"✅ No further failure within the test's travel (event {n_done}).")
    elif stop == _capi.EVENTS_UNLOADED:
        say(f"⚠️  The network carries no load at event {n_done}.")
    curve = [[float(run["lam"][k] * span), float(run["lam"][k] * run["force1"][k])] for k in range(n_done)]
    with open(os.path.join(fea_dir, "failure_events.csv"), "w") as f:
        f.write("event,lam,total_displacement,total_force,n_failed,n_active\n")
        for k in range(n_done):
            f.write(f"{k+1},{float(run['lam'][k])!r},{curve[k][0]!r},{curve[k][1]!r},"
                    f"{int(run['n_failed'][k])},{int(run['n_active'][k])}\n")
    if npy:
        np.save(os.path.join(fea_dir, "event_of.npy"), run["event_of"])
    if not n_done:
        return [], [], [], []
    return run["stress"], run["active"], run["U"], curve


def write_records(fea_dir, n_nodes, n_elems, stress_record, active_record, disp_record,
                  force_disp_curve, out_format="python", npy=False):
    """CSV writers, src/fea_solver.py:297-316 (pandas) / src/fea_petsc.cpp:433-516,
    through the native multi-threaded writer (mfea_write_record_csv), which
    reproduces both byte for byte.  The C++ driver writes a record file only
    when it holds at least one step (src/fea_petsc.cpp:435, 457, 477, 508)."""
    petsc = out_format == "petsc"
    style = _capi.CSV_PETSC if petsc else _capi.CSV_PANDAS
    files = (("stress_record.csv", _capi.REC_STRESS, stress_record, n_elems),
             ("active_elements.csv", _capi.REC_ACTIVE, active_record, n_elems),
             ("node_displacements.csv", _capi.REC_DISP, disp_record, 3 * n_nodes),
             ("force_displacement.csv", _capi.REC_FORCE, force_disp_curve, 2))
    for name, kind, rec, ncol in files:
        if petsc and not len(rec):
            continue
        _capi.write_record_csv(os.path.join(fea_dir, name), style, kind, rec, n_cols=ncol)
        if npy:
            _capi.write_record_npy(os.path.join(fea_dir, name[:-4] + ".npy"), kind, rec, n_cols=ncol)


def write_energy(fea_dir, n_elems, force_disp_curve, energy_record, wax_record, wb_record,
                 out_format="python", npy=False):
    """The files of fea_solver(energy=True): energy.csv — one line per record
    row, floats as Python's repr writes them — and the two element records
    through the native writer, in the stress record's layout (petsc: written
    only when they hold a row, as write_records)."""
    with open(os.path.join(fea_dir, "energy.csv"), "w") as f:
        f.write("step,total_displacement,axial_energy,bending_energy\n")
        for k, (w_ax, w_b) in enumerate(energy_record):
            f.write(f"{k+1},{float(force_disp_curve[k][0])!r},{float(w_ax)!r},{float(w_b)!r}\n")
    petsc = out_format == "petsc"
    style = _capi.CSV_PETSC if petsc else _capi.CSV_PANDAS
    for name, rec in (("element_energy_axial.csv", wax_record), ("element_energy_bending.csv", wb_record)):
        if petsc and not len(rec):
            continue
        _capi.write_record_csv(os.path.join(fea_dir, name), style, _capi.REC_STRESS, rec, n_cols=n_elems)
        if npy:
            _capi.write_record_npy(os.path.join(fea_dir, name[:-4] + ".npy"), _capi.REC_STRESS, rec, n_cols=n_elems)


def main(argv=None):
    global N_STEPS, DISPLACEMENT_MAX, MAX_STRAIN, REG
    ap = argparse.ArgumentParser(description="MI355X FEA (drop-in for src/fea_solver.py)")
    ap.add_argument("results_dir")
    ap.add_argument("--grip-length", type=float, default=GRIP_LENGTH)
    ap.add_argument("--disp-max", type=float, default=DISPLACEMENT_MAX)
    ap.add_argument("--n-steps", type=int, default=N_STEPS)
    ap.add_argument("--max-strain", type=float, default=MAX_STRAIN)
    ap.add_argument("--rtol", type=float, default=RTOL)
    ap.add_argument("--max-it", type=int, default=MAX_IT)
    ap.add_argument("--reg", type=float, default=REG)
    ap.add_argument("--pc", choices=["gamg", "jacobi", "bjacobi", "sor", "icc"], default="gamg")
    ap.add_argument("--format", choices=["python", "petsc"], default="python")
    ap.add_argument("--npy", action="store_true", help="also write each record as a .npy sidecar")
    ap.add_argument("--device-run", action="store_true",
                    help="run the step loop as one library call, the records gathered on the device "
                         "(one process, one partition)")
    ap.add_argument("--events", action="store_true",
                    help="event-driven failure run: one solve per failure, each break at its exact "
                         "load (one process, one partition)")
    ap.add_argument("--tie-rtol", type=float, default=1e-9,
                    help="--events: elements within this relative distance of the largest strain break together")
    ap.add_argument("--max-events", type=int, default=None, help="--events: at most this many events")
    ap.add_argument("--parts", type=int, default=1,
                    help="partitions of the multi-GPU solve, all on this device (one process); "
                         "for one GPU per process launch with torch.distributed.run instead")
    ap.add_argument("--element-props", metavar="FILE", default=None,
                    help="per-element properties: CSV with a header, elem_id plus any of E,A,I,max_strain, "
                         "every element exactly once (one process, one partition)")
    ap.add_argument("--grip-direction", metavar="TX,TY,TZ[/BX,BY,BZ]", default=None,
                    help="direction of the grips' motion, the ramp's displacements being the amplitudes "
                         "(bottom: the same as the top's unless given; one process, one partition); "
                         "default 0,1,0: the tensile test")
    ap.add_argument("--shear", action="store_true", help="shorthand for --grip-direction 1,0,0")
    ap.add_argument("--energy", action="store_true",
                    help="also write the strain energy of every record row, axial and bending parts: energy.csv, "
                         "element_energy_axial.csv, element_energy_bending.csv (one process, one partition)")
    ap.add_argument("--grip-field", metavar="FILE.csv", default=None,
                    help="a prescribed vector per grip node: CSV with the header node_id,dx,dy,dz; node n moves "
                         "by amplitude x (dx,dy,dz), the ramp's displacements being the amplitudes.  Grip nodes "
                         "not listed take their band's direction (--grip-direction or the tensile default), "
                         "free nodes listed are ignored.  force_displacement.csv keeps total_displacement = "
                         "dy_top - dy_bot, total_force is the generalised force of the top band "
                         "(one process, one partition)")
    ap.add_argument("--node-loads", metavar="FILE.csv", default=None,
                    help="a force per free node: CSV with the header node_id,fx,fy,fz; nodes not listed carry "
                         "none, grip nodes listed are ignored, the load on a piece cut off from both grips is "
                         "dropped (one process, one partition)")
    ap.add_argument("--load-mode", choices=["dead", "proportional"], default="dead",
                    help="--node-loads: dead, the load as given at every step, or proportional, dy_top times "
                         "it (--events takes proportional loads only)")
    a = ap.parse_args(argv)
    if a.energy and a.parts > 1:
        print("fea_solver: --energy needs one partition (--parts 1)", file=sys.stderr)
        sys.exit(2)
    grip = None
    if a.shear and a.grip_direction is not None:
        print("fea_solver: --shear and --grip-direction exclude each other", file=sys.stderr)
        sys.exit(2)
    if a.shear or a.grip_direction is not None:
        try:
            grip = parse_grip_direction("1,0,0" if a.shear else a.grip_direction)
        except ValueError as e:
            print(f"fea_solver: --grip-direction: {e}", file=sys.stderr)
            sys.exit(2)
    field = None
    if a.grip_field is not None:
        if a.parts > 1:
            print("fea_solver: --grip-field needs one partition (--parts 1)", file=sys.stderr)
            sys.exit(2)
        try:
            from mfea import fields
            n_nodes = len(pd.read_csv(os.path.join(a.results_dir, "nodes.csv")))
            field = fields.read_csv(a.grip_field, n_nodes)
        except (ValueError, OSError) as e:
            print(f"fea_solver: --grip-field: {e}", file=sys.stderr)
            sys.exit(2)
    node_loads = None
    if a.node_loads is not None:
        if a.parts > 1:
            print("fea_solver: --node-loads needs one partition (--parts 1)", file=sys.stderr)
            sys.exit(2)
        if a.events and a.load_mode != "proportional":
            print("fea_solver: --events with --node-loads needs --load-mode proportional", file=sys.stderr)
            sys.exit(2)
        try:
            from mfea import loads
            n_nodes = len(pd.read_csv(os.path.join(a.results_dir, "nodes.csv")))
            node_loads = loads.read_csv(a.node_loads, n_nodes)
        except (ValueError, OSError) as e:
            print(f"fea_solver: --node-loads: {e}", file=sys.stderr)
            sys.exit(2)
    props = None
    if a.element_props is not None:
        try:
            n_elems = len(pd.read_csv(os.path.join(a.results_dir, "elements.csv")))
            props = read_element_props(a.element_props, n_elems)
        except (ValueError, OSError) as e:
            print(f"fea_solver: --element-props: {e}", file=sys.stderr)
            sys.exit(2)
    N_STEPS, DISPLACEMENT_MAX, MAX_STRAIN, REG = a.n_steps, a.disp_max, a.max_strain, a.reg
    fea_solver(a.results_dir, tol=a.grip_length, rtol=a.rtol, max_it=a.max_it,
               precond={"gamg": _capi.PC_GAMG, "jacobi": _capi.PC_JACOBI,
                        "bjacobi": _capi.PC_BLOCK_JACOBI, "sor": _capi.PC_SOR, "icc": _capi.PC_ICC}[a.pc],
               out_format=a.format, nparts=a.parts, npy=a.npy, device_run=a.device_run,
               events=a.events, tie_rtol=a.tie_rtol, max_events=a.max_events, element_props=props,
               grip_direction=grip, energy=a.energy, grip_field=field, node_loads=node_loads,
               load_mode=a.load_mode)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        print("Usage: python fea_solver.py <results_dir>")
        sys.exit(0)
    main()
