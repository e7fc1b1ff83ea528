"""Torch-facing wrapper of mesh smoothing (include/lsf_hip.h: lsf_mesh_smooth_prepare, _run, lsf_mesh_vertex_normals):
Taubin passes over a mesh's edge neighbours with its open borders pinned, and vertex normals rebuilt from the faces
("Mesh smoothing"; tests/mesh_smooth_restatement.py restates the rule).  Every argument is
checked on the host before a launch.  prepare() enqueues the launches that validate the mesh and build the edge table,
the pins and the compressed-row neighbour list, and reads the record back: the one host synchronisation of a call, and
where a refused mesh raises.  smooth() goes on with the passes and, when the mesh has normals, the normals; nothing
waits for them.  Outputs are device tensors.  The public interface is fusion.smooth_mesh and
fusion.mesh_vertex_normals."""
import ctypes
import math

import torch

from . import _lib
from ._lib import MeshSmoothParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_mesh_simplify import _check, _ptr

RECORD_FIELDS = _lib.MESH_SMOOTH_RECORD_FIELDS
DEFAULT_ITERATIONS, DEFAULT_LAM, DEFAULT_MU = 10, 0.5, -0.53


def least_table_slots(face_count):
    """the smallest legal table_slots: the power of two >= 2 * max(3F, 1)"""
    need = 2 * max(3 * int(face_count), 1)
    return 1 << (need - 1).bit_length()


def params(vertex_count, face_count, iterations=DEFAULT_ITERATIONS, lam=DEFAULT_LAM, mu=DEFAULT_MU, boundary="fixed",
           table_slots=None, max_blocks=None, fresh_record=False):
    """the lsf_mesh_smooth_params of a call, after the host checks"""
    v, f = int(vertex_count), int(face_count)
    if v < 0 or f < 0 or max(v, f) > _lib.MESH_SMOOTH_MAX_ITEMS:
        raise ValueError("a mesh of %d vertices and %d faces is beyond the %d of either that the edge table reaches"
                         % (v, f, _lib.MESH_SMOOTH_MAX_ITEMS))
    try:
        whole = not isinstance(iterations, bool) and int(iterations) == iterations
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or not 0 <= iterations <= _lib.MESH_SMOOTH_MAX_ITERATIONS:
        raise ValueError("iterations must be a whole number in 0 .. %d, got %r"
                         % (_lib.MESH_SMOOTH_MAX_ITERATIONS, iterations))
    try:
        lam, mu = float(lam), float(mu)
    except (TypeError, ValueError):
        raise ValueError("lam and mu must be numbers, got %r and %r" % (lam, mu)) from None
    if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError("lam must be finite and in (0, 1], got %r" % (lam,))
    if not (math.isfinite(mu) and mu <= 0.0):
        raise ValueError("mu must be finite and <= 0 (0 leaves the mu passes out), got %r" % (mu,))
    if not isinstance(boundary, str) or boundary not in _lib.MESH_SMOOTH_BOUNDARIES:
        raise ValueError("boundary must be 'fixed' or 'free', got %r" % (boundary,))
    least = least_table_slots(f)
    slots = least if table_slots is None else int(table_slots)
    if slots < least or slots & (slots - 1) or slots > _lib.MESH_SMOOTH_MAX_SLOTS:
        raise ValueError("table_slots must be None or a power of two in %d .. %d, got %r"
                         % (least, _lib.MESH_SMOOTH_MAX_SLOTS, table_slots))
    blocks = 0 if max_blocks is None else int(max_blocks)
    if max_blocks is not None and not 1 <= blocks <= _lib.MESH_SMOOTH_MAX_BLOCKS:
        raise ValueError("max_blocks must be None or 1 .. %d, got %r" % (_lib.MESH_SMOOTH_MAX_BLOCKS, max_blocks))
    p = MeshSmoothParams()
    p.vertex_count, p.face_count, p.table_slots = v, f, slots
    p.boundary_fixed, p.fresh_record = _lib.MESH_SMOOTH_BOUNDARIES[boundary], int(bool(fresh_record))
    p.iterations, p.max_blocks, p.reserved = int(iterations), blocks, 0
    p.lam, p.mu = lam, mu
    return p


def unpack_record(record):
    """{field: int} of a host copy of the record"""
    return dict(zip(RECORD_FIELDS, (int(x) for x in record)))


def _refuse(rec, vertex_count):
    for field, what in (("invalid_vertices", "vertices with a non-finite coordinate"),
                        ("invalid_faces", "faces with an index outside [0, %d)" % vertex_count)):
        if rec[field]:
            raise ValueError("mesh smoothing refused: %d %s" % (rec[field], what))


def _mesh(vertices, faces):
    _check(vertices, "vertices", torch.float32, None, None)
    _check(faces, "faces", torch.int32, None, vertices.device)
    return int(vertices.shape[0]), int(faces.shape[0])


class _Prepared:
    """one prepare call's inputs, params, workspaces and record"""


def prepare(vertices, faces, iterations=DEFAULT_ITERATIONS, lam=DEFAULT_LAM, mu=DEFAULT_MU, boundary="fixed",
            table_slots=None, max_blocks=None):
    """lsf_mesh_smooth_prepare and the one read of the record.  vertices float32 (V, 3), faces int32 (F, 3): contiguous
    device tensors.  Returns the prepared call: its params, its workspaces (the neighbour list at its bound of 6F words,
    so that no host read sizes it) and `rec`, the record as a dict.  Raises ValueError when the record counts a
    non-finite vertex or a face index outside [0, V), RuntimeError when the edge table overflowed, which a table of the
    legal sizes cannot.  table_slots and max_blocks are for tests: None picks the smallest legal table and the library's
    grid cap; no output depends on either."""
    v_count, f_count = _mesh(vertices, faces)
    p = params(v_count, f_count, iterations, lam, mu, boundary, table_slots, max_blocks)
    require_gpu()
    dev = vertices.device
    if not vertices.is_cuda:
        raise ValueError("vertices and faces must be device tensors, got tensors on %s" % dev)
    tile = _lib.MESH_SMOOTH_TILE
    c = _Prepared()
    c.p, c.P, c.dev, c.V, c.F = p, ctypes.byref(p), dev, v_count, f_count
    c.vertices, c.faces = vertices, faces
    c.vertex_work = torch.empty((_lib.MESH_SMOOTH_VERTEX_WORDS, max(v_count, 1)), dtype=torch.int32, device=dev)
    c.edge_keys = torch.empty(p.table_slots, dtype=torch.int64, device=dev)
    c.edge_counts = torch.empty(p.table_slots, dtype=torch.int32, device=dev)
    c.tile_offsets = torch.empty(max((v_count + tile - 1) // tile, 1), dtype=torch.int32, device=dev)
    c.neighbours = torch.empty(max(6 * f_count, 1), dtype=torch.int32, device=dev)
    c.scalars = torch.empty(_lib.MESH_SMOOTH_SCALAR_WORDS, dtype=torch.int64, device=dev)
    c.record = torch.empty(_lib.MESH_SMOOTH_RECORD_WORDS, dtype=torch.int64, device=dev)
    check(lib.lsf_mesh_smooth_prepare(_ptr(vertices), _ptr(faces), _ptr(c.vertex_work), _ptr(c.edge_keys),
                                      _ptr(c.edge_counts), _ptr(c.tile_offsets), _ptr(c.neighbours), _ptr(c.scalars),
                                      _ptr(c.record), c.P, stream_ptr()), "lsf_mesh_smooth_prepare")
    c.rec = unpack_record(c.record.tolist())  # host synchronisation: the call's one
    _refuse(c.rec, v_count)
    if c.rec["table_overflow"]:
        raise RuntimeError("mesh smoothing: %d corner pairs found no slot in an edge table of %d slots, which holds "
                           "every edge of %d faces" % (c.rec["table_overflow"], p.table_slots, f_count))
    return c


def run(c):
    """lsf_mesh_smooth_run of a prepared call: float32 (V, 3), the smoothed positions, enqueued without waiting"""
    out = torch.empty((c.V, 3), dtype=torch.float32, device=c.dev)
    c.scratch = torch.empty((c.V, 3), dtype=torch.float32, device=c.dev)
    check(lib.lsf_mesh_smooth_run(_ptr(c.vertices), _ptr(c.vertex_work), _ptr(c.neighbours), _ptr(out),
                                  _ptr(c.scratch), _ptr(c.scalars), _ptr(c.record), c.P, stream_ptr()),
          "lsf_mesh_smooth_run")
    return out


def _normals(vertices, faces, p, scalars, record):
    v_count = int(vertices.shape[0])
    sums = torch.empty((max(v_count, 1), 3), dtype=torch.int64, device=vertices.device)
    out = torch.empty((v_count, 3), dtype=torch.float32, device=vertices.device)
    check(lib.lsf_mesh_vertex_normals(_ptr(vertices), _ptr(faces), _ptr(sums), _ptr(out), _ptr(scalars), _ptr(record),
                                      ctypes.byref(p), stream_ptr()), "lsf_mesh_vertex_normals")
    return out


def smooth(vertices, faces, normals=None, colours=None, iterations=DEFAULT_ITERATIONS, lam=DEFAULT_LAM, mu=DEFAULT_MU,
           boundary="fixed", recompute_normals=True, return_record=False, table_slots=None, max_blocks=None):
    """prepare(), lsf_mesh_smooth_run and, with normals given and recompute_normals, lsf_mesh_vertex_normals of the
    smoothed positions.  normals float32 (V, 3) or None, colours uint8 (V, 3) or None.  Returns (vertices, faces,
    normals or None, colours or None, record): the smoothed positions and the rebuilt normals are new device tensors,
    enqueued without waiting; faces, colours and normals that are not rebuilt are the tensors that came in.  record is
    the dict read after prepare -- nonfinite_out and zero_normals still 0 -- or with return_record the whole record, read
    a second time behind the last launch.  Raises as prepare() does."""
    v_count, _ = _mesh(vertices, faces)
    if normals is not None:
        _check(normals, "normals", torch.float32, v_count, vertices.device)
    if colours is not None:
        _check(colours, "colours", torch.uint8, v_count, vertices.device)
    c = prepare(vertices, faces, iterations, lam, mu, boundary, table_slots, max_blocks)
    out = run(c)
    if normals is not None and recompute_normals:
        normals = _normals(out, faces, c.p, c.scalars, c.record)
    rec = unpack_record(c.record.tolist()) if return_record else c.rec
    return out, faces, normals, colours, rec


def vertex_normals(vertices, faces, max_blocks=None):
    """lsf_mesh_vertex_normals on its own and one read of its record.  Returns (normals float32 (V, 3), record): the
    area-weighted vertex normals of the faces, (0, 0, 0) where the faces around a vertex sum to no length, which the
    record's zero_normals counts.  Raises ValueError when the record counts a non-finite vertex or a face index outside
    [0, V)."""
    v_count, f_count = _mesh(vertices, faces)
    p = params(v_count, f_count, 0, max_blocks=max_blocks, fresh_record=True)
    require_gpu()
    if not vertices.is_cuda:
        raise ValueError("vertices and faces must be device tensors, got tensors on %s" % vertices.device)
    scalars = torch.empty(_lib.MESH_SMOOTH_SCALAR_WORDS, dtype=torch.int64, device=vertices.device)
    record = torch.empty(_lib.MESH_SMOOTH_RECORD_WORDS, dtype=torch.int64, device=vertices.device)
    out = _normals(vertices, faces, p, scalars, record)
    rec = unpack_record(record.tolist())  # host synchronisation: the call's one
    _refuse(rec, v_count)
    return out, rec
