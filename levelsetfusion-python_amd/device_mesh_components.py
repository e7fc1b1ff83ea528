"""Torch-facing wrapper of mesh components (include/lsf_hip.h: lsf_mesh_components_label, _table, _select, _emit):
the connected components of a triangle mesh, their table, and the filter that removes components (INTEGRATION.md
section 3, "Mesh components"; tests/mesh_components_restatement.py restates the rule).  Every argument is checked on the
host before a launch.  components() enqueues the labelling launches, reads the record back (its one host
synchronisation), raises when the record reports invalid input, allocates the table at its exact size and enqueues the
launches that fill it.  filter() goes on from there: the kept rows are chosen with torch on the C-row table alone, the
selecting launches count what stays, the record is read a second time (two host synchronisations in all) and the
emitting launches write outputs of exactly those sizes.  Outputs are device tensors, returned without waiting for them.
The public interface is fusion.mesh_components and fusion.filter_mesh_components."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import MeshComponentsParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_mesh_simplify import _check, _ptr

RECORD_FIELDS = _lib.MESH_COMPONENTS_RECORD_FIELDS
TABLE_FIELDS = ("labels", "vertex_counts", "face_counts", "bounds")


def params(vertex_count, face_count, normals=False, colours=False, max_blocks=None):
    """the lsf_mesh_components_params of a call, after the host checks"""
    v, f = int(vertex_count), int(face_count)
    if v < 0 or f < 0 or max(v, f) > _lib.MESH_COMPONENTS_MAX_ITEMS:
        raise ValueError("a mesh of %d vertices and %d faces is beyond the %d of either that the int32 workspaces reach"
                         % (v, f, _lib.MESH_COMPONENTS_MAX_ITEMS))
    blocks = 0 if max_blocks is None else int(max_blocks)
    if max_blocks is not None and not 1 <= blocks <= _lib.MESH_COMPONENTS_MAX_BLOCKS:
        raise ValueError("max_blocks must be None or 1 .. %d, got %r" % (_lib.MESH_COMPONENTS_MAX_BLOCKS, max_blocks))
    p = MeshComponentsParams()
    p.vertex_count, p.face_count = v, f
    p.has_normals, p.has_colours = int(bool(normals)), int(bool(colours))
    p.max_blocks = blocks
    return p


def criteria(min_faces=None, min_vertices=None, min_extent=None, keep_largest=None):
    """the filter's criteria after their checks: (min_faces, min_vertices, min_extent, keep_largest), None where not
    given.  No criterion at all is a ValueError."""
    if min_faces is None and min_vertices is None and min_extent is None and keep_largest is None:
        raise ValueError("filter_mesh_components needs a criterion: min_faces, min_vertices, min_extent or keep_largest")
    out = []
    for value, name in ((min_faces, "min_faces"), (min_vertices, "min_vertices")):
        if value is not None:
            if isinstance(value, bool) or int(value) != value or value < 0:
                raise ValueError("%s must be None or a whole number >= 0, got %r" % (name, value))
            value = int(value)
        out.append(value)
    if min_extent is not None:
        min_extent = float(min_extent)
        if not (np.isfinite(min_extent) and min_extent >= 0):
            raise ValueError("min_extent must be None or finite and >= 0, got %r" % (min_extent,))
    out.append(min_extent)
    if keep_largest is not None:
        if isinstance(keep_largest, bool) or int(keep_largest) != keep_largest or keep_largest < 1:
            raise ValueError("keep_largest must be None or a whole number >= 1, got %r" % (keep_largest,))
        keep_largest = int(keep_largest)
    out.append(keep_largest)
    return tuple(out)


def unpack_record(record):
    """{field: int} of a host copy of the record"""
    return dict(zip(RECORD_FIELDS, (int(x) for x in record)))


class _Labelled:
    """one labelling call's inputs, workspaces and table"""


def _label(vertices, faces, normals, colours, max_blocks):
    _check(vertices, "vertices", torch.float32, None, None)
    dev = vertices.device
    _check(faces, "faces", torch.int32, None, dev)
    v_count, f_count = int(vertices.shape[0]), int(faces.shape[0])
    if normals is not None:
        _check(normals, "normals", torch.float32, v_count, dev)
    if colours is not None:
        _check(colours, "colours", torch.uint8, v_count, dev)
    p = params(v_count, f_count, normals is not None, colours is not None, max_blocks)
    require_gpu()
    if not vertices.is_cuda:
        raise ValueError("vertices, faces, normals and colours must be device tensors, got tensors on %s" % dev)
    tile = _lib.MESH_COMPONENTS_TILE
    tiles = 3 * ((v_count + tile - 1) // tile) + (f_count + tile - 1) // tile
    c = _Labelled()
    c.p, c.P, c.dev, c.V, c.F = p, ctypes.byref(p), dev, v_count, f_count
    c.vertices, c.faces, c.normals, c.colours = vertices, faces, normals, colours
    c.vertex_work = torch.empty((_lib.MESH_COMPONENTS_VERTEX_WORDS, max(v_count, 1)), dtype=torch.int32, device=dev)
    c.tile_offsets = torch.empty(max(tiles, 1), dtype=torch.int32, device=dev)
    c.record = torch.empty(_lib.MESH_COMPONENTS_RECORD_WORDS, dtype=torch.int64, device=dev)
    stream = stream_ptr()
    check(lib.lsf_mesh_components_label(_ptr(vertices), _ptr(faces), _ptr(c.vertex_work), _ptr(c.tile_offsets),
                                        _ptr(c.record), c.P, stream), "lsf_mesh_components_label")
    rec = unpack_record(c.record.tolist())  # host synchronisation: the number of components
    for field, what in (("invalid_vertices", "vertices with a non-finite coordinate"),
                        ("invalid_faces", "faces with an index outside [0, %d)" % v_count)):
        if rec[field]:
            raise ValueError("mesh components refused: %d %s" % (rec[field], what))
    if rec["step_cap"]:
        raise RuntimeError("mesh components: %d lanes of the union-find met the step cap of %d, which no mesh reaches"
                           % (rec["step_cap"], v_count + 1))
    n = c.C = rec["components"]
    c.labels = torch.empty(n, dtype=torch.int32, device=dev)
    c.vertex_counts = torch.empty(n, dtype=torch.int32, device=dev)
    c.face_counts = torch.empty(n, dtype=torch.int32, device=dev)
    c.bounds = torch.empty((n, 2, 3), dtype=torch.float32, device=dev)
    c.face_labels = torch.empty(f_count, dtype=torch.int32, device=dev)
    check(lib.lsf_mesh_components_table(_ptr(faces), _ptr(c.vertex_work), _ptr(c.labels), _ptr(c.vertex_counts),
                                        _ptr(c.face_counts), _ptr(c.bounds), _ptr(c.face_labels), n, c.P, stream),
          "lsf_mesh_components_table")
    c.vertex_labels = c.vertex_work[1, :v_count]
    c.table = dict(labels=c.labels, vertex_counts=c.vertex_counts, face_counts=c.face_counts, bounds=c.bounds)
    return c, rec


def components(vertices, faces, max_blocks=None):
    """lsf_mesh_components_label, one read of the record, lsf_mesh_components_table.  vertices float32 (V, 3), faces
    int32 (F, 3): contiguous device tensors.  Returns (vertex_labels int32 (V,), face_labels int32 (F,), table): device
    tensors, enqueued without waiting; table is a dict of labels, vertex_counts, face_counts int32 (C,) and bounds
    float32 (C, 2, 3), the C components in ascending label order.  Raises ValueError when the record counts a non-finite
    vertex or a face index outside [0, V), RuntimeError when a lane met the union-find's step cap.  max_blocks is for
    tests: the cap of every grid, None for the library's; no output depends on it."""
    c, _ = _label(vertices, faces, None, None, max_blocks)
    return c.vertex_labels, c.face_labels, c.table


def keep_rows(table, min_faces=None, min_vertices=None, min_extent=None, keep_largest=None):
    """int32 (C,) on the table's device: 1 for the rows the criteria keep.  Torch on the compact table only.  A row passes
    when it meets every threshold given (the longest edge of the bounds is compared in float64 of the float32 bounds);
    with keep_largest = k the first k passing rows stay, in the order face count descending, label ascending."""
    labels, faces = table["labels"], table["face_counts"]
    passing = torch.ones(labels.shape[0], dtype=torch.bool, device=labels.device)
    if min_faces is not None:
        passing &= faces >= min_faces
    if min_vertices is not None:
        passing &= table["vertex_counts"] >= min_vertices
    if min_extent is not None and labels.shape[0]:
        b = table["bounds"].to(torch.float64)
        passing &= (b[:, 1] - b[:, 0]).max(dim=1).values >= min_extent
    if keep_largest is not None and labels.shape[0]:
        # one int64 key per row: passing rows first, then faces descending, then label ascending (labels are unique)
        key = ((faces.max().to(torch.int64) - faces.to(torch.int64)) << 32) | labels.to(torch.int64)
        key = torch.where(passing, key, torch.full_like(key, torch.iinfo(torch.int64).max))
        first = torch.argsort(key)[:keep_largest]
        chosen = torch.zeros_like(passing)
        chosen[first] = True
        passing &= chosen
    return passing.to(torch.int32)


def filter(vertices, faces, normals=None, colours=None, min_faces=None, min_vertices=None, min_extent=None,
           keep_largest=None, max_blocks=None):
    """The mesh without the components the criteria reject: lsf_mesh_components_label and _table as components(), the
    kept rows by keep_rows, lsf_mesh_components_select, a second read of the record, lsf_mesh_components_emit.  Returns
    (vertices, faces, normals or None, colours or None, record): device tensors of exactly the record's sizes, enqueued
    without waiting, and the record as a dict.  Kept vertices and faces keep their input order, faces are re-indexed,
    normals and colours are carried bit for bit.  Two host synchronisations.  Raises as components() does, and
    ValueError when no criterion is given."""
    crit = criteria(min_faces, min_vertices, min_extent, keep_largest)
    c, _ = _label(vertices, faces, normals, colours, max_blocks)
    dev, stream = c.dev, stream_ptr()
    keep = keep_rows(c.table, *crit)
    check(lib.lsf_mesh_components_select(_ptr(faces), _ptr(c.vertex_work), _ptr(keep), _ptr(c.tile_offsets),
                                         _ptr(c.record), c.C, c.P, stream), "lsf_mesh_components_select")
    rec = unpack_record(c.record.tolist())  # host synchronisation: the sizes of the outputs
    out_v, out_f = rec["vertices_out"], rec["faces_out"]
    out_vertices = torch.empty((out_v, 3), dtype=torch.float32, device=dev)
    out_faces = torch.empty((out_f, 3), dtype=torch.int32, device=dev)
    out_normals = torch.empty((out_v, 3), dtype=torch.float32, device=dev) if normals is not None else None
    out_colours = torch.empty((out_v, 3), dtype=torch.uint8, device=dev) if colours is not None else None
    if out_v:
        check(lib.lsf_mesh_components_emit(_ptr(vertices), _ptr(faces), _ptr(normals), _ptr(colours),
                                           _ptr(c.vertex_work), _ptr(keep), _ptr(c.tile_offsets), _ptr(out_vertices),
                                           _ptr(out_normals), _ptr(out_colours), _ptr(out_faces), c.C, out_v, out_f,
                                           c.P, stream), "lsf_mesh_components_emit")
    return out_vertices, out_faces, out_normals, out_colours, rec
