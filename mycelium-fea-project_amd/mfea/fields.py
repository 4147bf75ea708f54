"""Grip displacement fields for Engine.set_grip_field (mfea_set_grip_field).

Pure NumPy, no device.  Every builder returns an ``n_nodes x 3`` float64 array
in the order of the mesh's nodes: row n is the vector d_n of node n, and the
rows of nodes not in ``nodes`` are zeros.  The engine prescribes
``amplitude * d_n`` at a grip node, the amplitude being the dy_top / dy_bot of
the solve, step, run or event call.
"""
from __future__ import annotations

import csv

import numpy as np

COLUMNS = ("node_id", "dx", "dy", "dz")


def _nodes(nodes, n_nodes):
    idx = np.asarray(nodes, dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= n_nodes):
        raise ValueError(f"node index out of range [0, {n_nodes})")
    return idx


def _xyz(xyz):
    return np.asarray(xyz, dtype=np.float64).reshape(-1, 3)


def rigid_rotation(xyz, nodes, axis, centre=None):
    """d_n = axis x (x_n - centre) on ``nodes``: the first-order displacement of
    a rigid rotation about ``axis`` through ``centre`` (default: the mean of
    xyz[nodes]); |axis| scales it, the amplitude of the call is the angle."""
    xyz = _xyz(xyz)
    idx = _nodes(nodes, xyz.shape[0])
    axis = np.asarray(axis, dtype=np.float64).reshape(3)
    out = np.zeros((xyz.shape[0], 3), dtype=np.float64)
    if idx.size:
        c = xyz[idx].mean(axis=0) if centre is None else np.asarray(centre, dtype=np.float64).reshape(3)
        out[idx] = np.cross(axis, xyz[idx] - c)
    return out


def affine(xyz, nodes, H, origin=(0.0, 0.0, 0.0)):
    """d_n = H @ (x_n - origin) on ``nodes``: the affine boundary displacement
    of homogenisation (H a 3 x 3 displacement gradient)."""
    xyz = _xyz(xyz)
    idx = _nodes(nodes, xyz.shape[0])
    H = np.asarray(H, dtype=np.float64).reshape(3, 3)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    out = np.zeros((xyz.shape[0], 3), dtype=np.float64)
    if idx.size:
        out[idx] = (H @ (xyz[idx] - o).T).T
    return out


def uniform(n_nodes, nodes, vec):
    """d_n = vec on ``nodes``: a band moving as a rigid block."""
    idx = _nodes(nodes, int(n_nodes))
    out = np.zeros((int(n_nodes), 3), dtype=np.float64)
    out[idx] = np.asarray(vec, dtype=np.float64).reshape(3)
    return out


def read_csv(path, n_nodes, columns=COLUMNS):
    """The field of a CSV file with the columns node_id, dx, dy, dz (a header
    line, one row per listed node, any order).  Returns (field, listed): the
    n_nodes x 3 array and the boolean mask of the nodes the file lists.
    ValueError, naming the file, for a missing column, a duplicate or
    out-of-range node id, or a value that is not finite.  ``columns``: other
    names for the four columns (mfea.loads.read_csv: node_id, fx, fy, fz)."""
    names = ",".join(columns)
    n_nodes = int(n_nodes)
    field = np.zeros((n_nodes, 3), dtype=np.float64)
    listed = np.zeros(n_nodes, dtype=bool)
    with open(path, newline="") as f:
        rd = csv.reader(f)
        header = [h.strip() for h in next(rd, [])]
        for col in columns:
            if col not in header:
                raise ValueError(f"{path}: missing column {col!r} (columns: {names})")
        at = [header.index(col) for col in columns]
        for line, row in enumerate(rd, start=2):
            if not row or all(not c.strip() for c in row):
                continue
            if len(row) <= max(at):
                raise ValueError(f"{path}:{line}: missing column (a row needs {names})")
            try:
                nid = float(row[at[0]])
                d = [float(row[k]) for k in at[1:]]
            except ValueError:
                raise ValueError(f"{path}:{line}: not a number: {row}") from None
            if not np.isfinite(nid) or nid != int(nid):
                raise ValueError(f"{path}:{line}: node_id {row[at[0]].strip()} is not an integer")
            n = int(nid)
            if n < 0 or n >= n_nodes:
                raise ValueError(f"{path}:{line}: node_id {n} out of range [0, {n_nodes})")
            if listed[n]:
                raise ValueError(f"{path}:{line}: duplicate node_id {n}")
            if not np.all(np.isfinite(d)):
                raise ValueError(f"{path}:{line}: non-finite value for node_id {n}")
            field[n] = d
            listed[n] = True
    return field, listed
