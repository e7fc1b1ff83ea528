"""Torch-facing wrapper of mesh simplification (include/lsf_hip.h: lsf_mesh_simplify_count, lsf_mesh_simplify_emit):
welding vertices of equal bits, or clustering them by the cell of a lattice ("Mesh
simplification"; tests/mesh_simplify_restatement.py restates the rule).  Every argument is checked on the host before a
launch.  A call enqueues the counting launches, reads the record back (its one host synchronisation), raises when the
record reports invalid input, allocates the outputs at their exact size and enqueues the two emitting launches.  The
outputs are returned as device tensors without waiting for them.  The public interface is fusion.simplify_mesh."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import MeshSimplifyParams, check, lib
from .device_core import require_gpu, stream_ptr

RECORD_FIELDS = _lib.MESH_SIMPLIFY_RECORD_FIELDS


def smallest_table_slots(vertex_count, face_count):
    """the smallest legal table: a power of two, at least twice the larger count"""
    need = 2 * max(int(vertex_count), int(face_count), 1)
    return 1 << (need - 1).bit_length()


def params(vertex_count, face_count, cell_size=None, origin=(0.0, 0.0, 0.0), table_slots=None, normals=False,
           colours=False):
    """the lsf_mesh_simplify_params of a call, after the host checks"""
    v, f = int(vertex_count), int(face_count)
    if v < 0 or f < 0 or max(v, f) > _lib.MESH_SIMPLIFY_MAX_ITEMS:
        raise ValueError("a mesh of %d vertices and %d faces is beyond the %d of either that the int32 workspaces reach"
                         % (v, f, _lib.MESH_SIMPLIFY_MAX_ITEMS))
    p = MeshSimplifyParams()
    p.vertex_count, p.face_count = v, f
    p.cluster = 0 if cell_size is None else 1
    if cell_size is not None:
        p.cell_size = float(cell_size)
        if not (np.isfinite(p.cell_size) and p.cell_size > 0):
            raise ValueError("cell_size must be None (weld) or finite and positive, got %r" % (cell_size,))
    o = np.asarray(origin, dtype=np.float64)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    p.origin_x, p.origin_y, p.origin_z = (float(x) for x in o)
    least = smallest_table_slots(v, f)
    slots = least if table_slots is None else int(table_slots)
    if slots < least or slots & (slots - 1) or slots > 1 << 30:
        raise ValueError("table_slots must be a power of two, at least %d and at most 2^30, got %r"
                         % (least, table_slots))
    p.table_slots = slots
    p.has_normals, p.has_colours = int(bool(normals)), int(bool(colours))
    return p


def _check(t, name, dtype, rows, device):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a device tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, str(dtype).replace("torch.", ""), t.dtype))
    if t.dim() != 2 or t.shape[1] != 3 or (rows is not None and t.shape[0] != rows):
        raise ValueError("%s must have shape (%s, 3), got %s" % (name, "N" if rows is None else rows, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if device is not None and t.device != device:
        raise ValueError("%s lies on %s, the vertices on %s" % (name, t.device, device))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def unpack_record(record):
    """{field: int} of a host copy of the record"""
    return dict(zip(RECORD_FIELDS, (int(x) for x in record)))


def simplify(vertices, faces, normals=None, colours=None, cell_size=None, origin=(0.0, 0.0, 0.0), table_slots=None):
    """lsf_mesh_simplify_count, one read of the record, lsf_mesh_simplify_emit.  vertices float32 (V, 3), faces int32
    (F, 3), normals float32 (V, 3) or None, colours uint8 (V, 3) or None: contiguous device tensors.  cell_size None
    welds the vertices whose positions are equal bit for bit (-0 as +0); a cell size clusters the vertices of one cell
    of the lattice of that edge through origin.  Returns (vertices, faces, normals or None, colours or None, record):
    device tensors, enqueued without waiting, and the record as a dict.  Raises ValueError when the record counts an
    invalid vertex (a non-finite coordinate, or in cluster mode a cell beyond 2^20 on an axis), an invalid face (an
    index outside [0, V)) or a full table; no output is produced then.  table_slots is for tests: None picks the
    smallest legal size."""
    _check(vertices, "vertices", torch.float32, None, None)
    dev = vertices.device
    _check(faces, "faces", torch.int32, None, dev)
    v_count, f_count = int(vertices.shape[0]), int(faces.shape[0])
    if normals is not None:
        _check(normals, "normals", torch.float32, v_count, dev)
    if colours is not None:
        _check(colours, "colours", torch.uint8, v_count, dev)
    p = params(v_count, f_count, cell_size, origin, table_slots, normals is not None, colours is not None)
    require_gpu()
    if not vertices.is_cuda:
        raise ValueError("vertices, faces, normals and colours must be device tensors, got tensors on %s" % dev)
    k = 3 * (p.cluster + p.has_normals + p.has_colours)
    tile = _lib.MESH_SIMPLIFY_TILE
    tiles = 3 * ((v_count + tile - 1) // tile) + 3 * ((f_count + tile - 1) // tile)

    def work(words, dtype=torch.int32):
        return torch.empty(max(int(words), 1), dtype=dtype, device=dev)

    table = work(p.table_slots)
    vertex_work = work(_lib.MESH_SIMPLIFY_VERTEX_WORDS * v_count)
    cluster_work = work(_lib.MESH_SIMPLIFY_CLUSTER_WORDS * v_count)
    sums = work(k * v_count, torch.int64)
    face_work = work(_lib.MESH_SIMPLIFY_FACE_WORDS * f_count)
    tile_offsets = work(tiles)
    record = torch.empty(_lib.MESH_SIMPLIFY_RECORD_WORDS, dtype=torch.int64, device=dev)
    stream, P = stream_ptr(), ctypes.byref(p)
    check(lib.lsf_mesh_simplify_count(_ptr(vertices), _ptr(faces), _ptr(normals), _ptr(colours), _ptr(table),
                                      _ptr(vertex_work), _ptr(cluster_work), _ptr(sums), _ptr(face_work),
                                      _ptr(tile_offsets), _ptr(record), P, stream), "lsf_mesh_simplify_count")
    rec = unpack_record(record.tolist())  # the call's one host synchronisation
    for field, what in (("invalid_vertices", "vertices with a non-finite coordinate or a cell beyond 2^20"),
                        ("invalid_faces", "faces with an index outside [0, %d) or an invalid vertex" % v_count),
                        ("table_overflow", "items that found the hash table full")):
        if rec[field]:
            raise ValueError("mesh simplification refused: %d %s" % (rec[field], what))
    out_v, out_f = rec["vertices_out"], rec["faces_out"]
    out_vertices = torch.empty((out_v, 3), dtype=torch.float32, device=dev)
    out_faces = torch.empty((out_f, 3), dtype=torch.int32, device=dev)
    out_normals = torch.empty((out_v, 3), dtype=torch.float32, device=dev) if normals is not None else None
    out_colours = torch.empty((out_v, 3), dtype=torch.uint8, device=dev) if colours is not None else None
    if out_v:
        check(lib.lsf_mesh_simplify_emit(_ptr(vertices), _ptr(faces), _ptr(vertex_work), _ptr(cluster_work),
                                         _ptr(sums), _ptr(face_work), _ptr(tile_offsets), _ptr(out_vertices),
                                         _ptr(out_normals), _ptr(out_colours), _ptr(out_faces), rec["clusters"], out_v,
                                         out_f, P, stream), "lsf_mesh_simplify_emit")
    return out_vertices, out_faces, out_normals, out_colours, rec
