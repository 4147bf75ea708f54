"""Nodal loads for Engine.set_node_loads (mfea_set_node_loads).

Pure NumPy, no device.  Every builder returns an ``n_nodes x 3`` float64 array
in the order of the mesh's nodes: row n is the force f_n on node n, and the
rows of nodes that carry none are zeros.  The engine applies ``f_n`` as given
(mode "dead") or ``dy_top * f_n`` (mode "proportional") on the free nodes;
rows of grip nodes are ignored there.
"""
from __future__ import annotations

import numpy as np

from . import fields

COLUMNS = ("node_id", "fx", "fy", "fz")


def point(n_nodes, nodes, vector):
    """f_n = vector on ``nodes``: point loads, an indenter force.  ``vector`` is
    one 3-vector for all of them or one row per node; a node listed twice takes
    the sum."""
    n_nodes = int(n_nodes)
    idx = np.asarray(nodes, dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= n_nodes):
        raise ValueError(f"node index out of range [0, {n_nodes})")
    vec = np.asarray(vector, dtype=np.float64)
    if vec.size == 3:
        vec = np.broadcast_to(vec.reshape(1, 3), (idx.size, 3))
    elif vec.shape != (idx.size, 3):
        raise ValueError(f"vector must be one 3-vector or one row per node ({idx.size} x 3)")
    out = np.zeros((n_nodes, 3), dtype=np.float64)
    np.add.at(out, idx, vec)
    return out


def self_weight(xyz, e2n, weight_per_length, direction, active=None):
    """The weight of the elements lumped on their ends: each active element e
    puts ``0.5 * L_e * w_e * direction`` on each of its two nodes, L_e its
    length.  ``weight_per_length`` is a scalar or one value per element,
    ``direction`` a 3-vector (its length scales the load), ``active`` a mask
    over the elements (None: all)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    e2n = np.asarray(e2n, dtype=np.int64).reshape(-1, 2)
    n_elems = e2n.shape[0]
    if n_elems and (e2n.min() < 0 or e2n.max() >= xyz.shape[0]):
        raise ValueError(f"element node index out of range [0, {xyz.shape[0]})")
    w = np.asarray(weight_per_length, dtype=np.float64)
    if w.ndim == 0:
        w = np.full(n_elems, float(w))
    elif w.shape != (n_elems,):
        raise ValueError(f"weight_per_length must be a scalar or one value per element ({n_elems})")
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    on = np.ones(n_elems, dtype=bool) if active is None else np.asarray(active).ravel().astype(bool)
    if on.size != n_elems:
        raise ValueError(f"active must have one entry per element ({n_elems})")
    length = np.linalg.norm(xyz[e2n[:, 1]] - xyz[e2n[:, 0]], axis=1)
    half = np.where(on, 0.5 * length * w, 0.0)[:, None] * d[None, :]
    out = np.zeros((xyz.shape[0], 3), dtype=np.float64)
    np.add.at(out, e2n[:, 0], half)
    np.add.at(out, e2n[:, 1], half)
    return out


def read_csv(path, n_nodes):
    """The loads of a CSV file with the columns node_id, fx, fy, fz (a header
    line, one row per loaded node, any order; nodes not listed carry none).
    Returns the n_nodes x 3 array.  ValueError, naming the file, for a missing
    column, a duplicate or out-of-range node id, or a value that is not finite
    — the errors of mfea.fields.read_csv."""
    loads, _ = fields.read_csv(path, n_nodes, columns=COLUMNS)
    return loads
