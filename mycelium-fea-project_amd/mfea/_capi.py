"""ctypes binding of libmfea.so (include/mfea.h).

The HIP library is the product path: if it is missing this module raises
ImportError at import time — there is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CG_KERNEL = {"auto": 0, "lanes": 1, "sell": 2}

LIB_PATH = os.environ.get("MFEA_LIB", os.path.join(os.path.dirname(_HERE), "libmfea.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"mfea: HIP library not found at {LIB_PATH}; build it with "
        f"`make -C mycelium-fea-project_amd` (or __graft_entry__.build())")
_lib = C.CDLL(LIB_PATH)

# error codes (mfea.h)
OK, EINVAL, EDEVICE, ESTATE, EMAXIT, EBREAKDOWN, ENOMEM, ECOMM = 0, -1, -2, -3, -4, -5, -6, -7
PC_JACOBI, PC_BLOCK_JACOBI, PC_GAMG, PC_SOR, PC_ICC = 0, 1, 2, 3, 4
NORM_UNPRECONDITIONED, NORM_PRECONDITIONED = 0, 1
MESH_SKIP_INVALID = 1
RUN_COMPLETE, RUN_NO_ACTIVE = 0, 1  # mfea_run's stop_reason (or EMAXIT / EBREAKDOWN)
# mfea_run_events' stop_reason (or EMAXIT / EBREAKDOWN)
EVENTS_COMPLETE, EVENTS_LAMBDA_MAX, EVENTS_UNLOADED = 0, 1, 2
LOAD_DEAD, LOAD_PROPORTIONAL = 0, 1  # mfea_set_node_loads's mode


class SolveOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_it", C.c_int32),
                ("precond", C.c_int32), ("norm", C.c_int32), ("chunk", C.c_int32),
                ("reg", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("iters", C.c_int32), ("status", C.c_int32), ("relres", C.c_double),
                ("bnorm", C.c_double), ("n_free", C.c_int64), ("t_assemble_ms", C.c_double),
                ("t_rhs_ms", C.c_double), ("t_solve_ms", C.c_double), ("t_post_ms", C.c_double),
                ("t_setup_ms", C.c_double), ("amg_levels", C.c_int32), ("amg_rebuilt", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RunRecords(C.Structure):
    """mfea_run_records (include/mfea.h): where mfea_run writes each step's rows."""
    _fields_ = [("U", C.c_void_p), ("stress", C.c_void_p), ("active", C.c_void_p),
                ("force", C.c_void_p), ("n_active", C.c_void_p), ("stats", C.POINTER(Stats)),
                ("wall_s", C.c_void_p)]


class EventOpts(C.Structure):
    """mfea_event_opts (include/mfea.h)."""
    _fields_ = [("max_strain", C.c_double), ("tie_rtol", C.c_double), ("lam_max", C.c_double)]


class EventOut(C.Structure):
    """mfea_event_out (include/mfea.h)."""
    _fields_ = [("lam", C.c_double), ("force1", C.c_double), ("n_failed", C.c_int64),
                ("n_active", C.c_int64)]


class ElementProps(C.Structure):
    """mfea_element_props (include/mfea.h): per-element columns, NULL = the scalar."""
    _fields_ = [("E", C.c_void_p), ("A", C.c_void_p), ("I", C.c_void_p), ("max_strain", C.c_void_p)]


class ElementEnergy(C.Structure):
    """mfea_element_energy (include/mfea.h): the rows wanted, NULL = not wanted."""
    _fields_ = [("w_axial", C.c_void_p), ("w_bending", C.c_void_p), ("g_axial", C.c_void_p),
                ("g_bending", C.c_void_p)]


class EventRecords(C.Structure):
    """mfea_event_records (include/mfea.h): where mfea_run_events writes each event's rows."""
    _fields_ = [("U", C.c_void_p), ("stress", C.c_void_p), ("active", C.c_void_p),
                ("lam", C.c_void_p), ("force1", C.c_void_p), ("n_failed", C.c_void_p),
                ("n_active", C.c_void_p), ("event_of", C.c_void_p), ("stats", C.POINTER(Stats)),
                ("wall_s", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("n_elems", C.c_int64), ("n_free_nodes", C.c_int64),
                ("n_top", C.c_int64), ("n_known", C.c_int64), ("n_slices", C.c_int64),
                ("n_slots", C.c_int64), ("free_incidences", C.c_int64), ("planar", C.c_int32),
                ("cg_lanes", C.c_int32), ("n_lanes", C.c_int64), ("n_halo", C.c_int64),
                ("n_parts", C.c_int32), ("part", C.c_int32), ("n_pairs", C.c_int64),
                ("n_ghost", C.c_int64), ("halo_compact", C.c_int32), ("block_size", C.c_int32),
                ("grid", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GrowParams(C.Structure):
    """mfea_grow_params (include/mfea.h) — src/mycelium_sim_2D.cpp:17-33."""
    _fields_ = [("seed", C.c_uint64),
                ("h0", C.c_double), ("dt", C.c_double), ("lambda_angle", C.c_double),
                ("P_branch", C.c_double), ("c_g", C.c_double), ("D", C.c_double),
                ("M_cap", C.c_double), ("omega0", C.c_double),
                ("t_steps", C.c_int32), ("h0_per_point", C.c_int32),
                ("anastomosis_tol", C.c_double), ("wall_thickness", C.c_double),
                ("dish_size", C.c_double), ("substrate_width", C.c_double), ("substrate_E", C.c_double),
                ("inoc_nx", C.c_int32), ("inoc_ny", C.c_int32), ("inoc_dist", C.c_double),
                ("voxel_size", C.c_double), ("snapshot_every", C.c_int32), ("snapshot_dir", C.c_char_p),
                ("verbose", C.c_int32), ("threads", C.c_int32)]


_P = C.c_void_p
_sig = {
    "mfea_get_info": (C.c_int, [_P, C.POINTER(Info)]),
    "mfea_profile_iteration": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "mfea_profile_spmv": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    "mfea_abi_version": (C.c_int, []),
    "mfea_last_error": (C.c_int, [C.c_char_p, C.c_size_t]),
    "mfea_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "mfea_destroy": (C.c_int, [_P]),
    "mfea_set_material": (C.c_int, [_P, C.c_double, C.c_double, C.c_double]),
    "mfea_set_element_props": (C.c_int, [_P, C.POINTER(ElementProps)]),
    "mfea_get_element_props": (C.c_int, [_P, _P, _P, _P, _P]),
    "mfea_set_grip_motion": (C.c_int, [_P, _P, _P]),
    "mfea_get_grip_motion": (C.c_int, [_P, _P, _P]),
    "mfea_get_reaction": (C.c_int, [_P, _P, _P]),
    "mfea_set_grip_field": (C.c_int, [_P, _P]),
    "mfea_get_grip_field": (C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    "mfea_get_grip_work": (C.c_int, [_P, _P, _P]),
    "mfea_set_node_loads": (C.c_int, [_P, _P, C.c_int32]),
    "mfea_get_node_loads": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfea_get_load_work": (C.c_int, [_P, _P]),
    "mfea_get_energy": (C.c_int, [_P, _P, _P, _P, C.POINTER(ElementEnergy)]),
    "mfea_set_mesh": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_uint32]),
    "mfea_set_bc": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P]),
    "mfea_set_active": (C.c_int, [_P, _P]),
    "mfea_assemble": (C.c_int, [_P]),
    "mfea_solve": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(SolveOpts), C.POINTER(Stats)]),
    "mfea_post": (C.c_int, [_P, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mfea_step": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(SolveOpts), C.c_double,
                            C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(Stats)]),
    "mfea_run": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(SolveOpts), C.c_double,
                           C.POINTER(RunRecords), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfea_event": (C.c_int, [_P, C.c_double, C.c_double, C.POINTER(SolveOpts), C.POINTER(EventOpts),
                             C.POINTER(EventOut), C.POINTER(Stats)]),
    "mfea_run_events": (C.c_int, [_P, C.c_int32, C.c_double, C.c_double, C.POINTER(SolveOpts),
                                  C.POINTER(EventOpts), C.POINTER(EventRecords), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32)]),
    "mfea_get_displacement": (C.c_int, [_P, _P]),
    "mfea_get_stress": (C.c_int, [_P, _P]),
    "mfea_get_active": (C.c_int, [_P, _P]),
    "mfea_element_stiffness": (C.c_int, [_P, C.c_int64, _P, _P, C.c_double, C.c_double,
                                         C.c_double, _P, _P]),
    "mfea_export_csr": (C.c_int, [_P, C.POINTER(C.c_int64), _P, _P, _P]),
    "mfea_solve_csr": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P,
                                 C.POINTER(SolveOpts), _P, C.POINTER(Stats)]),
    "mfea_dist_unique_id": (C.c_int, [_P]),
    "mfea_dist_init": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "mfea_set_partition_axis": (C.c_int, [_P, C.c_int]),
    "mfea_get_ownership": (C.c_int, [_P, _P, _P]),
    "mfea_gather_results": (C.c_int, [_P, _P, _P, _P]),
    "mfea_write_record_npy": (C.c_int, [C.c_char_p, C.c_int, C.c_int64, C.c_int64, _P, _P]),
    "mfea_write_record_csv": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P,
                                        C.c_int]),
    "mfea_grow_default_params": (None, [C.POINTER(GrowParams)]),
    "mfea_grow": (C.c_int, [C.POINTER(GrowParams), C.POINTER(_P)]),
    "mfea_grow_info": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mfea_grow_mesh": (C.c_int, [_P, _P, _P]),
    "mfea_grow_write": (C.c_int, [_P, C.c_char_p]),
    "mfea_grow_free": (None, [_P]),
    # include/mfea_debug.h
    "mfea_debug_trace_iteration": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mfea_debug_set_parts": (C.c_int, [_P, C.c_int, C.c_int]),
    "mfea_debug_global_active": (C.c_int, [_P, C.c_void_p]),
    "mfea_debug_floating": (C.c_int, [_P, C.c_void_p]),
    "mfea_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "mfea_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "mfea_debug_option_info": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int)]),
    "mfea_debug_option_check": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "mfea_debug_amg_vcycle": (C.c_int, [_P, _P, _P]),
    "mfea_debug_amg_vector": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mfea_debug_amg_info": (C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P, C.c_int,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(_lib, _name)
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = tuple(_sig)


class MfeaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mfea error {code}: {msg}")
        self.code = code


class SolverFailure(np.linalg.LinAlgError):
    """PCG did not converge (max_it) or broke down.  Subclasses LinAlgError so
    the reference driver's ``except np.linalg.LinAlgError`` (src/fea_solver.py:247)
    catches it."""

    def __init__(self, code, msg, stats=None):
        super().__init__(f"mfea solver failure {code}: {msg}")
        self.code = code
        self.stats = stats


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    _lib.mfea_last_error(buf, len(buf))
    return buf.value.decode(errors="replace")


def _check(rc, stats=None):
    if rc == OK:
        return
    if rc in (EMAXIT, EBREAKDOWN):
        raise SolverFailure(rc, last_error(), stats)
    raise MfeaError(rc, last_error())


def _ptr(a):
    return a.ctypes.data_as(_P) if a is not None and a.size else None


def abi_version() -> int:
    return _lib.mfea_abi_version()


OPT_WRITABLE, OPT_REBUILDS_LAYOUT, OPT_KEEPS_KEPT = 1, 2, 4


def option_info():
    """Every option the library knows, without a handle (mfea_debug_option_info):
    (name, default, flags) of the writable ones in the library's table order,
    then of the read-only names (default 0, flags 0)."""
    out = []
    name, dflt, flags = C.c_char_p(), C.c_int64(), C.c_int()
    while _lib.mfea_debug_option_info(len(out), C.byref(name), C.byref(dflt), C.byref(flags)) == OK:
        out.append((name.value.decode(), dflt.value, flags.value))
    return out


def option_check(name: str, value: int) -> int:
    """What get_option would read back after set_option(name, value), without a
    handle (mfea_debug_option_check); MfeaError(EINVAL) where set_option would
    refuse."""
    v = C.c_int64()
    _check(_lib.mfea_debug_option_check(name.encode(), int(value), C.byref(v)))
    return v.value


# mfea_set_option's defaults, from the library's own table
DEFAULT_OPTIONS = {n: d for n, d, f in option_info() if f & OPT_WRITABLE}


def dist_unique_id() -> bytes:
    """The 128-byte RCCL unique id (rank 0 makes it, the launcher broadcasts it)."""
    buf = (C.c_uint8 * 128)()
    _check(_lib.mfea_dist_unique_id(buf))
    return bytes(buf)


CSV_PANDAS, CSV_PETSC = 0, 1
REC_STRESS, REC_ACTIVE, REC_DISP, REC_FORCE = 0, 1, 2, 3


def write_record_csv(path, style, kind, records, n_cols=None, threads=None):
    """One end-of-run record file through the native writer (mfea_write_record_csv):
    byte-identical to the reference's pandas / ostream writers.  records: list
    of per-step rows (or a 2-D array)."""
    flags = kind == REC_ACTIVE
    dt = np.uint8 if flags else np.float64
    if len(records):
        a = np.ascontiguousarray(np.asarray(records), dtype=dt).reshape(len(records), -1)
    else:
        a = np.zeros((0, n_cols or 0), dtype=dt)
    nr, nc = a.shape
    if threads is None:
        threads = min(16, os.cpu_count() or 1)
    p = a.ctypes.data_as(_P) if a.size else None
    _check(_lib.mfea_write_record_csv(os.fsencode(path), int(style), int(kind), nr, nc,
                                      None if flags else p, p if flags else None, int(threads)))


def write_record_npy(path, kind, records, n_cols=None):
    """The record as a .npy sidecar through the native writer
    (mfea_write_record_npy): float64 rows, or bool rows for REC_ACTIVE."""
    flags = kind == REC_ACTIVE
    dt = np.uint8 if flags else np.float64
    if len(records):
        a = np.ascontiguousarray(np.asarray(records), dtype=dt).reshape(len(records), -1)
    else:
        a = np.zeros((0, n_cols or 0), dtype=dt)
    nr, nc = a.shape
    p = a.ctypes.data_as(_P) if a.size else None
    _check(_lib.mfea_write_record_npy(os.fsencode(path), int(kind), nr, nc,
                                      None if flags else p, p if flags else None))


def grow_params(**kw) -> GrowParams:
    """The reference simulator's parameters (mfea_grow_default_params), with
    fields overridden by keyword."""
    p = GrowParams()
    _lib.mfea_grow_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(GrowParams._fields_):
            raise TypeError(f"unknown growth parameter {k!r}")
        setattr(p, k, os.fsencode(v) if k == "snapshot_dir" and v is not None else v)
    return p


def scaled_grow_params(scale=1.0, **kw) -> GrowParams:
    """A scale-times larger dish (host/mfea_grow.cpp --scale): inoculum grid
    5·scale × 5·scale at the reference's spacing, substrate and Omega0 scaled
    by the area, everything else the reference's."""
    p = grow_params()
    if scale != 1.0:
        p.dish_size *= scale
        p.substrate_width *= scale
        p.substrate_E *= scale * scale
        p.omega0 *= scale * scale
        p.inoc_nx = p.inoc_ny = int(5 * scale + 0.5)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def grow_network(params: GrowParams | None = None, out_dir=None):
    """Run the native producer (mfea_grow).  Returns (xyz, e2n) as the
    reference's nodes.csv / elements.csv would read back (6 significant
    digits), and writes those files (+ mycelium_growth_stats.csv) to out_dir
    if given."""
    p = params if params is not None else grow_params()
    g = _P()
    _check(_lib.mfea_grow(C.byref(p), C.byref(g)))
    try:
        nn, ne, nh = C.c_int64(), C.c_int64(), C.c_int64()
        _check(_lib.mfea_grow_info(g, C.byref(nn), C.byref(ne), C.byref(nh)))
        xyz = np.empty((nn.value, 3), np.float64)
        e2n = np.empty((ne.value, 2), np.int32)
        _check(_lib.mfea_grow_mesh(g, _ptr(xyz), _ptr(e2n)))
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            _check(_lib.mfea_grow_write(g, os.fsencode(out_dir)))
    finally:
        _lib.mfea_grow_free(g)
    return xyz, e2n.astype(np.int64)


def make_opts(rtol=1e-8, atol=0.0, max_it=100000, precond=PC_JACOBI, norm=NORM_UNPRECONDITIONED,
              chunk=0, reg=1e-12) -> SolveOpts:
    return SolveOpts(rtol, atol, int(max_it), int(precond), int(norm), int(chunk), reg)


def event_opts(max_strain, tie_rtol=1e-9, lam_max=np.inf) -> EventOpts:
    """mfea_event_opts, checked as the library checks them."""
    max_strain, tie_rtol, lam_max = float(max_strain), float(tie_rtol), float(lam_max)
    if not max_strain > 0.0:
        raise ValueError("max_strain must be > 0")
    if not 0.0 <= tie_rtol < 1.0:
        raise ValueError("tie_rtol must be in [0, 1)")
    if not lam_max > 0.0:
        raise ValueError("lam_max must be > 0 (inf allowed)")
    return EventOpts(max_strain, tie_rtol, lam_max)


def event_envelope(lam, force1, span):
    """The displacement-controlled force-displacement sawtooth of an event run.

    lam[k], force1[k]: load factor and reference-load reaction of event k;
    span = dy_top - dy_bot of the reference load.  Under displacement control
    the grips only ever move apart, so event k happens at the displacement
    Lam_k·span with Lam_k = max(lam[0..k]): an event with lam[k] < Lam_{k-1}
    is an avalanche break at held displacement.  Two points per event — the
    force just before the break, Lam_k·force1[k], and just after it on the new
    active set, Lam_k·force1[k+1] (the last event: Lam_k·force1[k], nothing
    follows it).  A terminal event's lam (inf on an unloaded network, or one
    beyond lam_max) is no displacement the test reached: Lam stays, and with it
    the point.  Returns (displacement, force), arrays of 2·len(lam) entries.
    """
    lam = np.asarray(lam, dtype=np.float64).ravel()
    f1 = np.asarray(force1, dtype=np.float64).ravel()
    if lam.size != f1.size:
        raise ValueError("lam and force1 must have one entry per event")
    n = lam.size
    disp = np.empty(2 * n)
    force = np.empty(2 * n)
    top = 0.0
    for k in range(n):
        if np.isfinite(lam[k]) and lam[k] > top:
            top = float(lam[k])
        nxt = f1[k + 1] if k + 1 < n else f1[k]
        disp[2 * k] = disp[2 * k + 1] = top * span
        force[2 * k] = top * f1[k]
        force[2 * k + 1] = top * nxt
    return disp, force


class Engine:
    """One device handle (mfea_handle).  Host arrays are copied on every call."""

    def __init__(self, device: int = 0):
        h = _P()
        _check(_lib.mfea_create(int(device), C.byref(h)))
        self._h = h
        self.n_nodes = 0
        self.n_elems = 0

    def close(self):
        if getattr(self, "_h", None):
            _lib.mfea_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- partitioning -------------------------------------------------------
    def dist_init(self, rank: int, world: int, unique_id: bytes):
        """Join an RCCL world (one process per GPU); call before set_mesh."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be 128 bytes")
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(_lib.mfea_dist_init(self._h, int(rank), int(world), buf))

    def set_partition_axis(self, axis: int = -1):
        _check(_lib.mfea_set_partition_axis(self._h, int(axis)))

    def global_active(self) -> np.ndarray:
        """The host's global element activity the partitioned plan reads
        (mfea_debug_global_active)."""
        out = np.zeros(self.n_elems, np.uint8)
        _check(_lib.mfea_debug_global_active(self._h, out.ctypes.data_as(C.c_void_p)))
        return out.astype(bool)

    def floating(self) -> np.ndarray:
        """Free nodes cut off from both grips by the current activity, from the
        device's connected components (mfea_debug_floating)."""
        out = np.zeros(self.n_nodes, np.uint8)
        _check(_lib.mfea_debug_floating(self._h, out.ctypes.data_as(C.c_void_p)))
        return out.astype(bool)

    def set_parts(self, nparts: int, axis: int = -1):
        """nparts partitions of the multi-GPU solve held by this handle on one
        device (mfea_debug_set_parts: the partitioned path, testable on one GPU)."""
        _check(_lib.mfea_debug_set_parts(self._h, int(nparts), int(axis)))

    def set_option(self, name: str, value: int):
        """mfea_set_option (include/mfea_debug.h): tuning / comparison knobs."""
        _check(_lib.mfea_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        """mfea_get_option: the option's current value."""
        v = C.c_int64()
        _check(_lib.mfea_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    @contextlib.contextmanager
    def options(self, **kw):
        """Set options for a block, then restore the values they had before."""
        prev = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in prev.items():
                self.set_option(k, v)

    # ---- setup --------------------------------------------------------------
    def set_material(self, E, A, I):
        _check(_lib.mfea_set_material(self._h, float(E), float(A), float(I)))

    def set_mesh(self, xyz, e2n, skip_invalid=False):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        e2n = np.ascontiguousarray(e2n, dtype=np.int64).reshape(-1, 2)
        self._xyz, self._e2n = xyz, e2n
        _check(_lib.mfea_set_mesh(self._h, xyz.shape[0], _ptr(xyz), e2n.shape[0], _ptr(e2n),
                                  MESH_SKIP_INVALID if skip_invalid else 0))
        self.n_nodes, self.n_elems = xyz.shape[0], e2n.shape[0]

    def set_element_props(self, E=None, A=None, I=None, max_strain=None):
        """Per-element modulus, section and failure strain (mfea_set_element_props):
        each a contiguous float64 array of n_elems entries in the order of the
        mesh's elements, or None for the scalar (set_material / the call's
        max_strain).  All None: back to the uniform engine.  The library copies
        the arrays."""
        if not hasattr(self, "_xyz"):  # (no mesh yet: the library's MFEA_ESTATE)
            _check(_lib.mfea_set_element_props(self._h, None))
            return
        cols, keep = ElementProps(), []
        for name, v in (("E", E), ("A", A), ("I", I), ("max_strain", max_strain)):
            if v is None:
                continue
            a = np.asarray(v)
            if a.dtype != np.float64 or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a contiguous float64 array")
            if a.ndim != 1 or a.size != self.n_elems:
                raise ValueError(f"{name} must have one entry per element ({self.n_elems})")
            keep.append(a)
            setattr(cols, name, _ptr(a))
        _check(_lib.mfea_set_element_props(self._h, C.byref(cols)))

    def element_props(self) -> dict:
        """What the engine uses (mfea_get_element_props): E, A, I filled with the
        handle's scalar where no array was set, max_strain NaN where none was."""
        out = {k: np.empty(self.n_elems, dtype=np.float64) for k in ("E", "A", "I", "max_strain")}
        _check(_lib.mfea_get_element_props(self._h, _ptr(out["E"]), _ptr(out["A"]), _ptr(out["I"]),
                                           _ptr(out["max_strain"])))
        return out

    def set_grip_motion(self, top=None, bot=None):
        """Directions of the grip motion (mfea_set_grip_motion): a top-band node
        is prescribed dy_top * top[c], a bottom-band node dy_bot * bot[c];
        None leaves a direction as it is.  Default (0, 1, 0) for both: the
        tensile test.  Not normalised."""
        vecs = []
        for name, v in (("top", top), ("bot", bot)):
            if v is None:
                vecs.append(None)
                continue
            a = np.ascontiguousarray(v, dtype=np.float64).ravel()
            if a.size != 3:
                raise ValueError(f"{name} must have three components")
            vecs.append(a)
        _check(_lib.mfea_set_grip_motion(self._h, *(None if a is None else _ptr(a) for a in vecs)))

    def grip_motion(self):
        """(top, bot): the two directions (mfea_get_grip_motion)."""
        top, bot = np.empty(3), np.empty(3)
        _check(_lib.mfea_get_grip_motion(self._h, _ptr(top), _ptr(bot)))
        return top, bot

    def reaction(self):
        """(top3, bot3): per band the sum over its rows of (K U)[3n + c], c = x,
        y, z, on the unregularised K of the last assembly and the current U
        (mfea_get_reaction)."""
        top, bot = np.empty(3), np.empty(3)
        _check(_lib.mfea_get_reaction(self._h, _ptr(top), _ptr(bot)))
        return top, bot

    def set_grip_field(self, field=None):
        """A prescribed vector per grip node (mfea_set_grip_field): field is
        n_nodes x 3 in the order of the mesh's nodes, row n the vector d_n; a
        node of the top band is prescribed dy_top * d_n, one of the bottom band
        dy_bot * d_n.  Rows of nodes in no band are ignored.  None: no field,
        back to set_grip_motion's two directions.  mfea.fields builds the usual
        ones.  The library copies the array."""
        if field is None:
            _check(_lib.mfea_set_grip_field(self._h, None))
            return
        a = np.ascontiguousarray(field, dtype=np.float64)
        if hasattr(self, "_xyz") and a.size != 3 * self.n_nodes:
            raise ValueError(f"field must have three entries per node ({self.n_nodes} nodes)")
        _check(_lib.mfea_set_grip_field(self._h, _ptr(a)))

    def grip_field(self):
        """(field, is_set): the stored n_nodes x 3 field; without one, every row
        holds the vector its node's band uses (mfea_get_grip_field)."""
        if not hasattr(self, "_xyz"):  # (no mesh yet: the library's MFEA_ESTATE)
            _check(_lib.mfea_get_grip_field(self._h, None, None))
        out = np.empty((self.n_nodes, 3), dtype=np.float64)
        is_set = C.c_int32(0)
        _check(_lib.mfea_get_grip_field(self._h, _ptr(out), C.byref(is_set)))
        return out, bool(is_set.value)

    def grip_work(self):
        """(top, bot): the generalised force of each band on the unregularised K
        of the last assembly and the current U (mfea_get_grip_work); the top one
        is what a step reports as its force."""
        top, bot = np.empty(1), np.empty(1)
        _check(_lib.mfea_get_grip_work(self._h, _ptr(top), _ptr(bot)))
        return float(top[0]), float(bot[0])

    LOAD_MODES = {"dead": LOAD_DEAD, "proportional": LOAD_PROPORTIONAL}

    def set_node_loads(self, loads=None, mode="dead"):
        """A force vector per free node (mfea_set_node_loads): loads is
        n_nodes x 3 in the order of the mesh's nodes, row n the force on node n;
        rows of grip nodes are ignored.  mode "dead": the load as given, whatever
        the amplitudes; "proportional": dy_top times the row, the load per unit
        of the top amplitude.  The load on a piece cut off from both grips is
        dropped (the piece stays at zero).  None: no loads.  mfea.loads builds
        the usual ones.  The library copies the array."""
        if loads is None:
            _check(_lib.mfea_set_node_loads(self._h, None, LOAD_DEAD))
            return
        m = self.LOAD_MODES.get(mode, mode)
        if isinstance(m, str):
            raise ValueError(f"mode must be 'dead' or 'proportional', not {mode!r}")
        a = np.ascontiguousarray(loads, dtype=np.float64)
        if hasattr(self, "_xyz") and a.size != 3 * self.n_nodes:
            raise ValueError(f"loads must have three entries per node ({self.n_nodes} nodes)")
        _check(_lib.mfea_set_node_loads(self._h, _ptr(a), int(m)))

    def node_loads(self):
        """(loads, mode, is_set): the stored n_nodes x 3 loads (zeros without
        any), "dead" or "proportional" (mfea_get_node_loads)."""
        if not hasattr(self, "_xyz"):  # (no mesh yet: the library's MFEA_ESTATE)
            _check(_lib.mfea_get_node_loads(self._h, None, None, None))
        out = np.empty((self.n_nodes, 3), dtype=np.float64)
        mode, is_set = C.c_int32(0), C.c_int32(0)
        _check(_lib.mfea_get_node_loads(self._h, _ptr(out), C.byref(mode), C.byref(is_set)))
        return out, ("proportional" if mode.value == LOAD_PROPORTIONAL else "dead"), bool(is_set.value)

    def load_work(self):
        """The work of the nodal loads on the current U, the sum of q_n . u_n
        over the free nodes that are not floating, with the amplitudes of the
        last solve (mfea_get_load_work); 0.0 without loads."""
        w = np.empty(1)
        _check(_lib.mfea_get_load_work(self._h, _ptr(w)))
        return float(w[0])

    ENERGY_ROWS = ("w_axial", "w_bending", "g_axial", "g_bending")

    def energy(self, U=None, active=None, elements=True) -> dict:
        """Strain energy per element, split into its axial and bending parts
        (mfea_get_energy).  U: 3 * n_nodes in original node order, None = the
        handle's current displacement; active: one entry per element saying
        which count, None = the handle's current activity (after a step that
        failed elements, that step's K held the activity before it).  Returns
        {"axial", "bending"}, the two totals, and with elements=True the rows
        w_axial, w_bending (energies) and g_axial, g_bending (the same per unit
        EA_e / EI12_e), in original element order."""
        if U is not None:
            U = np.ascontiguousarray(U, dtype=np.float64).ravel()
            if U.size != 3 * self.n_nodes:
                raise ValueError("U must have three entries per node")
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.uint8).ravel()
            if active.size != self.n_elems:
                raise ValueError("active must have one entry per element")
        total = np.zeros(2)
        rows = {k: np.empty(self.n_elems) for k in self.ENERGY_ROWS} if elements else {}
        out = ElementEnergy(*(_ptr(rows[k]) for k in self.ENERGY_ROWS)) if elements else None
        _check(_lib.mfea_get_energy(self._h, _ptr(U), _ptr(active), _ptr(total),
                                    C.byref(out) if elements else None))
        return {"axial": float(total[0]), "bending": float(total[1]), **rows}

    def energy_gradient(self, U=None, active=None) -> dict:
        """{"E", "A", "I"}: the derivative of the strain energy W = ½ UᵀKU with
        respect to each element's modulus, area and second moment, from the
        g rows of energy() and element_props() (include/mfea.h):
        dW/dE_e = A_e g_ax + (12 I_e) g_b, dW/dA_e = E_e g_ax,
        dW/dI_e = (12 E_e) g_b.  Gradients of the equilibrium energy when U
        solves the K of `active`."""
        en, p = self.energy(U, active), self.element_props()
        return {"E": p["A"] * en["g_axial"] + (12.0 * p["I"]) * en["g_bending"],
                "A": p["E"] * en["g_axial"],
                "I": (12.0 * p["E"]) * en["g_bending"]}

    def set_bc(self, top, bot):
        top = np.ascontiguousarray(top, dtype=np.int64).ravel()
        bot = np.ascontiguousarray(bot, dtype=np.int64).ravel()
        _check(_lib.mfea_set_bc(self._h, top.size, _ptr(top), bot.size, _ptr(bot)))

    def set_active(self, active=None):
        if active is None:
            _check(_lib.mfea_set_active(self._h, None))
        else:
            a = np.ascontiguousarray(active, dtype=np.uint8).ravel()
            if a.size != self.n_elems:
                raise ValueError("active must have one entry per element")
            _check(_lib.mfea_set_active(self._h, _ptr(a)))

    # ---- hot path -----------------------------------------------------------
    def assemble(self):
        _check(_lib.mfea_assemble(self._h))

    def solve(self, dy_top, dy_bot, opts: SolveOpts | None = None) -> Stats:
        st = Stats()
        o = opts if opts is not None else make_opts()
        _check(_lib.mfea_solve(self._h, float(dy_top), float(dy_bot), C.byref(o), C.byref(st)), st)
        return st

    def post(self, max_strain):
        f = C.c_double()
        n = C.c_int64()
        _check(_lib.mfea_post(self._h, float(max_strain), C.byref(f), C.byref(n)))
        return f.value, n.value

    def step(self, dy_top, dy_bot, opts: SolveOpts | None, max_strain):
        st = Stats()
        f = C.c_double()
        n = C.c_int64()
        o = opts if opts is not None else make_opts()
        _check(_lib.mfea_step(self._h, float(dy_top), float(dy_bot), C.byref(o), float(max_strain),
                              C.byref(f), C.byref(n), C.byref(st)), st)
        return f.value, n.value, st

    def run(self, dy_top, dy_bot, opts: SolveOpts | None, max_strain, keep=("U", "stress", "active"),
            out=None):
        """The whole step loop in one call (mfea_run): step k is
        step(dy_top[k], dy_bot[k], opts, max_strain), its records gathered on
        the device and copied out while step k + 1 computes.  keep: which of
        "U", "stress", "active" to record (the others are None).  out: optional
        dict of preallocated C-contiguous n_steps × cols arrays to write into
        (U / stress float64, active uint8); rows >= n_done stay as they were.
        Returns a dict: the records cut to [:n_done] (active as bool), force,
        n_active, stats (list of dicts), wall_s, n_done and stop_reason
        (RUN_COMPLETE, RUN_NO_ACTIVE, EMAXIT or EBREAKDOWN — a solver stop does
        not raise)."""
        dyt = np.ascontiguousarray(dy_top, dtype=np.float64).ravel()
        dyb = np.ascontiguousarray(dy_bot, dtype=np.float64).ravel()
        if dyt.size != dyb.size:
            raise ValueError("dy_top and dy_bot must have one entry per step")
        n = dyt.size
        unknown = set(keep) - {"U", "stress", "active"}
        if unknown:
            raise ValueError(f"unknown record(s) {sorted(unknown)}")
        spec = {"U": (3 * self.n_nodes, np.float64), "stress": (self.n_elems, np.float64),
                "active": (self.n_elems, np.uint8)}
        arr = {}
        for name, (cols, dt) in spec.items():
            if name not in keep:
                arr[name] = None
                continue
            a = (out or {}).get(name)
            if a is None:
                a = np.empty((n, cols), dtype=dt)
            elif a.dtype != dt or a.shape != (n, cols) or not a.flags.c_contiguous:
                raise ValueError(f"out[{name!r}] must be a C-contiguous {np.dtype(dt).name} array of shape {(n, cols)}")
            arr[name] = a
        force = np.zeros(n)
        n_active = np.zeros(n, dtype=np.int64)
        wall = np.zeros(n)
        stats = (Stats * max(n, 1))()
        rec = RunRecords(*(arr[k].ctypes.data if arr[k] is not None and arr[k].size else None
                           for k in ("U", "stress", "active")),
                         force.ctypes.data, n_active.ctypes.data, stats, wall.ctypes.data)
        o = opts if opts is not None else make_opts()
        n_done, stop = C.c_int32(), C.c_int32()
        _check(_lib.mfea_run(self._h, n, _ptr(dyt), _ptr(dyb), C.byref(o), float(max_strain), C.byref(rec),
                             C.byref(n_done), C.byref(stop)))
        m = n_done.value
        res = {k: (None if a is None else a[:m]) for k, a in arr.items()}
        if res["active"] is not None:
            res["active"] = res["active"].astype(bool)
        res.update(force=force[:m], n_active=n_active[:m], stats=[stats[i].as_dict() for i in range(m)],
                   wall_s=wall[:m], n_done=m, stop_reason=stop.value)
        return res

    def event(self, dy_top, dy_bot, opts: SolveOpts | None, max_strain, tie_rtol=1e-9, lam_max=np.inf):
        """One failure event at the reference load (mfea_event): returns
        (lam, force1, n_failed, n_active, stats); n_failed == 0 is terminal."""
        ev = event_opts(max_strain, tie_rtol, lam_max)
        out = EventOut()
        st = Stats()
        o = opts if opts is not None else make_opts()
        _check(_lib.mfea_event(self._h, float(dy_top), float(dy_bot), C.byref(o), C.byref(ev), C.byref(out),
                               C.byref(st)), st)
        return out.lam, out.force1, out.n_failed, out.n_active, st

    def run_events(self, dy_top, dy_bot, opts: SolveOpts | None, max_strain, tie_rtol=1e-9, lam_max=np.inf,
                   n_events=None, keep=("U", "stress", "active"), out=None):
        """The event-driven failure run in one call (mfea_run_events): up to
        n_events (default n_elems + 1) events at the reference load (dy_top,
        dy_bot), each break at its exact load factor.  keep / out: as run().
        Returns a dict: the records cut to [:n_done] (U rows = lam·U₁, active
        as bool), lam, force1, n_failed, n_active, event_of (int32 per element,
        -1 = never failed), stats, wall_s, n_done and stop_reason
        (EVENTS_COMPLETE, EVENTS_LAMBDA_MAX, EVENTS_UNLOADED, EMAXIT or
        EBREAKDOWN — a solver stop does not raise)."""
        ev = event_opts(max_strain, tie_rtol, lam_max)
        n = self.n_elems + 1 if n_events is None else int(n_events)
        if n < 0:
            raise ValueError("n_events must be >= 0")
        unknown = set(keep) - {"U", "stress", "active"}
        if unknown:
            raise ValueError(f"unknown record(s) {sorted(unknown)}")
        spec = {"U": (3 * self.n_nodes, np.float64), "stress": (self.n_elems, np.float64),
                "active": (self.n_elems, np.uint8)}
        arr = {}
        for name, (cols, dt) in spec.items():
            if name not in keep:
                arr[name] = None
                continue
            a = (out or {}).get(name)
            if a is None:
                a = np.empty((n, cols), dtype=dt)
            elif a.dtype != dt or a.shape != (n, cols) or not a.flags.c_contiguous:
                raise ValueError(f"out[{name!r}] must be a C-contiguous {np.dtype(dt).name} array of shape {(n, cols)}")
            arr[name] = a
        lam = np.zeros(n)
        force1 = np.zeros(n)
        n_failed = np.zeros(n, dtype=np.int64)
        n_active = np.zeros(n, dtype=np.int64)
        wall = np.zeros(n)
        event_of = np.full(self.n_elems, -1, dtype=np.int32)
        stats = (Stats * max(n, 1))()
        rec = EventRecords(*(arr[k].ctypes.data if arr[k] is not None and arr[k].size else None
                             for k in ("U", "stress", "active")),
                           lam.ctypes.data, force1.ctypes.data, n_failed.ctypes.data, n_active.ctypes.data,
                           event_of.ctypes.data if event_of.size else None, stats, wall.ctypes.data)
        o = opts if opts is not None else make_opts()
        n_done, stop = C.c_int32(), C.c_int32()
        _check(_lib.mfea_run_events(self._h, n, float(dy_top), float(dy_bot), C.byref(o), C.byref(ev),
                                    C.byref(rec), C.byref(n_done), C.byref(stop)))
        m = n_done.value
        res = {k: (None if a is None else a[:m]) for k, a in arr.items()}
        if res["active"] is not None:
            res["active"] = res["active"].astype(bool)
        res.update(lam=lam[:m], force1=force1[:m], n_failed=n_failed[:m], n_active=n_active[:m],
                   event_of=event_of, stats=[stats[i].as_dict() for i in range(m)], wall_s=wall[:m],
                   n_done=m, stop_reason=stop.value)
        return res

    # ---- results --------------------------------------------------------------
    def displacement(self):
        U = np.empty(3 * self.n_nodes)
        _check(_lib.mfea_get_displacement(self._h, _ptr(U)))
        return U

    def stress(self):
        s = np.empty(self.n_elems)
        if self.n_elems:
            _check(_lib.mfea_get_stress(self._h, _ptr(s)))
        return s

    def active(self):
        a = np.empty(self.n_elems, dtype=np.uint8)
        if self.n_elems:
            _check(_lib.mfea_get_active(self._h, _ptr(a)))
        return a.astype(bool)

    def ownership(self):
        """(node_owned, elem_owned) bool arrays: what this handle reports
        (mfea_get_ownership; one partition: everything)."""
        n = np.empty(self.n_nodes, dtype=np.uint8)
        e = np.empty(self.n_elems, dtype=np.uint8)
        _check(_lib.mfea_get_ownership(self._h, _ptr(n), _ptr(e)))
        return n.astype(bool), e.astype(bool)

    def gather_results(self):
        """mfea_gather_results: (U, stress, active) of the whole mesh on rank
        0 of an RCCL world (None elsewhere); collective."""
        U = np.empty(3 * self.n_nodes)
        S = np.empty(self.n_elems)
        A = np.empty(self.n_elems, dtype=np.uint8)
        _check(_lib.mfea_gather_results(self._h, _ptr(U), _ptr(S), _ptr(A)))
        return U, S, A.astype(bool)

    def info(self) -> dict:
        inf = Info()
        _check(_lib.mfea_get_info(self._h, C.byref(inf)))
        return inf.as_dict()

    def profile_iteration(self, precond=PC_JACOBI, reps=50) -> float:
        """Average duration (ms) of the fused SpMV + CG iteration kernel."""
        ms = C.c_double()
        _check(_lib.mfea_profile_iteration(self._h, int(precond), int(reps), C.byref(ms)))
        return ms.value

    def profile_spmv(self, reps=100) -> float:
        """GAMG: average duration (ms) of the w = A_0 u kernel (mfea_profile_spmv)."""
        ms = C.c_double()
        _check(_lib.mfea_profile_spmv(self._h, int(reps), C.byref(ms)))
        return ms.value

    def trace_iteration(self, precond=PC_JACOBI, cap=1 << 16):
        """Per-wave s_memrealtime stamps (100 MHz) of one CG iteration launch:
        (waves, 4) = entry, partials reduced, SpMV done, stores drained."""
        out = np.zeros(4 * cap, dtype=np.uint64)
        nw = C.c_int64()
        _check(_lib.mfea_debug_trace_iteration(self._h, int(precond), out.ctypes.data, out.size,
                                               C.byref(nw)))
        return out[:4 * nw.value].reshape(-1, 4)

    def amg_info(self) -> dict:
        """The MFEA_PC_GAMG hierarchy for the current active set: rows and
        stored blocks per level, index-list entries of the numeric setup."""
        cap = 64
        nl = C.c_int()
        rows = np.zeros(cap, dtype=np.int64)
        blocks = np.zeros(cap, dtype=np.int64)
        pblocks = np.zeros(cap, dtype=np.int64)
        items = C.c_int64()
        nd = C.c_int()
        ndist = C.c_int()
        ptblocks = np.zeros(cap, dtype=np.int64)
        _check(_lib.mfea_debug_amg_info(self._h, C.byref(nl), rows.ctypes.data, blocks.ctypes.data,
                                        pblocks.ctypes.data, cap, C.byref(items), C.byref(nd), C.byref(ndist),
                                        ptblocks.ctypes.data))
        n = nl.value
        return {"levels": n, "rows": rows[:n].tolist(), "blocks": blocks[:n].tolist(),
                "pblocks": pblocks[:n].tolist(), "ptblocks": ptblocks[:n].tolist(),
                "pair_items": items.value, "nd": nd.value, "n_dist": ndist.value,
                "cycle": self.get_option("amg_cycle"),
                "collapse_level": self.get_option("amg_collapse_level"),
                "collapse_blocks": self.get_option("amg_collapse_blocks"),
                "merged": self.get_option("amg_merged"),
                "merge_dq_blocks": self.get_option("amg_merge_dq_blocks"),
                "merge_u_blocks": self.get_option("amg_merge_u_blocks")}

    def amg_vcycle(self, r):
        """mfea_debug_amg_vcycle: one GAMG V-cycle u = M r (n_nodes × ND, original
        node order; call after assemble)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        u = np.empty_like(r)
        _check(_lib.mfea_debug_amg_vcycle(self._h, _ptr(r), _ptr(u)))
        return u

    def amg_vector(self, level, which):
        """mfea_debug_amg_vector: a V-cycle vector (0 b, 1 x, 2 t, 3 e) of a
        level after amg_vcycle, in the level's natural row order."""
        n = C.c_int64()
        _check(_lib.mfea_debug_amg_vector(self._h, int(level), int(which), None, 0, C.byref(n)))
        nd = self.amg_info()["nd"]
        w = nd * nd if which in (4, 6) else nd
        out = np.zeros(n.value * w)
        _check(_lib.mfea_debug_amg_vector(self._h, int(level), int(which), _ptr(out), out.size, C.byref(n)))
        return out.reshape(n.value, w)

    # ---- reference-API helpers ------------------------------------------------
    def element_stiffness(self, p1s, p2s, E, A, I):
        p1 = np.ascontiguousarray(p1s, dtype=np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2s, dtype=np.float64).reshape(-1, 3)
        n = p1.shape[0]
        Ke = np.empty((n, 6, 6))
        L = np.empty(n)
        _check(_lib.mfea_element_stiffness(self._h, n, _ptr(p1), _ptr(p2), float(E), float(A),
                                           float(I), _ptr(Ke), _ptr(L)))
        return Ke, L

    def export_csr(self):
        nnz = C.c_int64(0)
        _check(_lib.mfea_export_csr(self._h, C.byref(nnz), None, None, None))
        indptr = np.empty(3 * self.n_nodes + 1, dtype=np.int64)
        indices = np.empty(nnz.value, dtype=np.int32)
        data = np.empty(nnz.value)
        _check(_lib.mfea_export_csr(self._h, C.byref(nnz), indptr.ctypes.data_as(_P),
                                    indices.ctypes.data_as(_P), data.ctypes.data_as(_P)))
        return indptr, indices, data

    def solve_csr(self, indptr, indices, data, known_dofs, known_vals, opts=None):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        kd = np.ascontiguousarray(known_dofs, dtype=np.int64).ravel()
        kv = np.ascontiguousarray(known_vals, dtype=np.float64).ravel()
        n = indptr.size - 1
        U = np.empty(n)
        st = Stats()
        o = opts if opts is not None else make_opts()
        _check(_lib.mfea_solve_csr(self._h, n, indptr.ctypes.data_as(_P), _ptr(indices), _ptr(data),
                                   kd.size, _ptr(kd), _ptr(kv), C.byref(o), _ptr(U), C.byref(st)), st)
        return U, st
