"""numpy restatement of mesh extraction from the canonical TSDF ("Mesh extraction").  The HIP
kernels (csrc/lsf_mesh.hip) must equal extract() bit for bit: vertex and normal float32 bit patterns, face indices and
the order of both arrays.  Every float step below is one float64 IEEE operation in the order written; numpy never
contracts, and the kernels are built with -ffp-contract=off.  The case table is tools/gen_mesh_tables.py's.  Host numpy
only: no package import.  Also the mesh checks the tests use: directed-edge manifoldness and the Euler
characteristic."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mesh_tables as G  # noqa: E402

__all__ = ["TRI_COUNT", "TRI_EDGES", "extract", "directed_edges", "is_closed_manifold", "euler_characteristic"]

TRI_COUNT, TRI_EDGES = G.tables()
# the offset (x, y, z) of each edge's lower corner in its cell, and its axis
EDGE_OFFSET = np.array([G.CORNERS[c] for c in G.EDGE_LOW], np.int64)
EDGE_AXIS = np.array(G.EDGE_AXIS, np.int64)


def _usable(tsdf, weight, min_weight):
    """weight > min_weight in float64 (NaN fails) and a finite tsdf"""
    with np.errstate(invalid="ignore"):
        return (weight.astype(np.float64) > float(min_weight)) & np.isfinite(tsdf)


def _gradient(t64, usable, i, j, k, axis):
    """the float64 gradient of the tsdf along axis (0 = x, 1 = y, 2 = z) at voxels (i, j, k)"""
    n = t64.shape[2 - axis]
    idx = [i, j, k][2 - axis]

    def neighbour(d):
        at = [i.copy(), j.copy(), k.copy()]
        p = idx + d
        ok = (p >= 0) & (p < n)
        at[2 - axis] = np.clip(p, 0, n - 1)
        return ok & usable[tuple(at)], t64[tuple(at)]

    up_ok, up = neighbour(1)
    dn_ok, dn = neighbour(-1)
    v = t64[i, j, k]
    both = (up - dn) / 2.0
    return np.where(up_ok & dn_ok, both, np.where(up_ok, up - v, np.where(dn_ok, v - dn, 0.0)))


def extract(tsdf, weight, offset, voxel_size=0.004, iso=0.0, min_weight=0.0, normals=False):
    """(vertices float32 (V, 3) in world (x, y, z), faces int32 (F, 3), normals float32 (V, 3) or None)"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.float32)
    if tsdf.ndim != 3 or min(tsdf.shape) < 2 or weight.shape != tsdf.shape:
        raise ValueError("mesh extraction needs one 3-D (Z, Y, X) shape of extents >= 2")
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    vs, iso = float(voxel_size), float(iso)
    nz, ny, nx = tsdf.shape
    usable = _usable(tsdf, weight, min_weight)
    t64 = tsdf.astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = t64 < iso
    # cells, named by their lowest voxel: valid when all 8 corners are usable; case bit c set when corner c is inside
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        x, y, z = G.CORNERS[c]
        sl = (slice(z, nz - 1 + z), slice(y, ny - 1 + y), slice(x, nx - 1 + x))
        valid &= usable[sl]
        case |= inside[sl].astype(np.int64) << c
    code = np.where(valid, case, 0)  # an invalid cell draws nothing, as an empty case
    # a vertex on the grid edge (voxel, axis) when some cell holding the edge crosses it
    mask = np.zeros((nz, ny, nx, 3), bool)
    for e in range(12):
        x, y, z = EDGE_OFFSET[e]
        a = EDGE_AXIS[e]
        lo, hi = G.EDGE_LOW[e], G.EDGE_HIGH[e]
        crossing = ((code >> lo) ^ (code >> hi)) & 1 == 1
        mask[z:nz - 1 + z, y:ny - 1 + y, x:nx - 1 + x, a] |= crossing
    flat = mask.reshape(-1)
    vid = np.full(flat.shape, -1, np.int64)
    vid[flat] = np.arange(int(flat.sum()))
    vid = vid.reshape(mask.shape)
    # vertices in (voxel linear index, axis) order
    i, j, k, axis = np.nonzero(mask)
    step = np.stack([axis == 0, axis == 1, axis == 2], 1).astype(np.int64)  # (x, y, z) unit step
    i1, j1, k1 = i + step[:, 2], j + step[:, 1], k + step[:, 0]
    a, b = t64[i, j, k], t64[i1, j1, k1]
    t = (iso - a) / (b - a)
    grid = [k, j, i]
    verts = np.empty((i.size, 3), np.float32)
    for ax in range(3):
        q = np.where(axis == ax, grid[ax].astype(np.float64) + t, grid[ax].astype(np.float64))
        verts[:, ax] = ((q + off[ax]) * vs).astype(np.float32)
    out_normals = None
    if normals:
        n = []
        for ax in range(3):
            ga = _gradient(t64, usable, i, j, k, ax)
            gb = _gradient(t64, usable, i1, j1, k1, ax)
            n.append(ga * (1.0 - t) + gb * t)
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        out_normals = np.zeros((i.size, 3), np.float32)
        nonzero = length != 0.0
        safe = np.where(nonzero, length, 1.0)
        for ax in range(3):
            out_normals[:, ax] = np.where(nonzero, n[ax] / safe, 0.0).astype(np.float32)
    # faces in (cell linear index, table order) order
    flat_code = code.reshape(-1)
    count = TRI_COUNT[flat_code].astype(np.int64)
    cells = np.repeat(np.arange(flat_code.size), count)
    first = np.cumsum(count) - count
    tri = np.arange(cells.size) - np.repeat(first, count)
    ci, cj, ck = np.unravel_index(cells, code.shape)
    faces = np.empty((cells.size, 3), np.int32)
    for m in range(3):
        e = TRI_EDGES[flat_code[cells], 3 * tri + m].astype(np.int64)
        o = EDGE_OFFSET[e]
        ids = vid[ci + o[:, 2], cj + o[:, 1], ck + o[:, 0], EDGE_AXIS[e]]
        assert np.all(ids >= 0)
        faces[:, m] = ids
    return verts, faces, out_normals


def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_manifold(faces):
    """every directed edge appears exactly once, and so does its reverse: a closed, consistently oriented 2-manifold
    (vertices are never merged, so each vertex belongs to one surface sheet)"""
    d = directed_edges(faces)
    if d.size == 0:
        return True
    key = d[:, 0] * (int(d.max()) + 1) + d[:, 1]
    rev = d[:, 1] * (int(d.max()) + 1) + d[:, 0]
    if np.unique(key).size != key.size:
        return False
    return bool(np.all(np.isin(rev, key)))


def boundary_edges(faces):
    """the directed edges whose reverse is not an edge"""
    d = directed_edges(faces)
    if d.size == 0:
        return d
    m = int(d.max()) + 1
    key, rev = d[:, 0] * m + d[:, 1], d[:, 1] * m + d[:, 0]
    return d[~np.isin(rev, key)]


def euler_characteristic(vertex_count, faces):
    f = np.asarray(faces, np.int64)
    d = directed_edges(f)
    undirected = np.unique(np.sort(d, axis=1), axis=0) if d.size else d
    return int(vertex_count) - len(undirected) + len(f)
