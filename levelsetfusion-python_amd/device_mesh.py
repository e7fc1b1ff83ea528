"""Torch-facing wrapper of mesh extraction (include/lsf_hip.h: lsf_mesh_count, lsf_mesh_emit,
lsf_mesh_vertex_colours).  Every argument is checked on the host before a launch.  A call enqueues the three counting
launches, reads the two totals back (its one host synchronisation), allocates the outputs at their exact size and
enqueues the two emitting launches; with a colour volume one more launch colours the vertices.  The outputs are
returned as device tensors without waiting for them.  The public interface is fusion.CanonicalVolume.extract_mesh."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import MeshParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import check_colour_volume, check_model
from .tsdf.generation import offsets_of

INT32_MAX = 0x7fffffff


def params(shape, array_offset, voxel_size=0.004, iso=0.0, min_weight=0.0):
    """the lsf_mesh_params of a call, after the host checks"""
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError("mesh extraction needs a 3-D (Z, Y, X) volume of extents >= 2, got shape %s"
                         % (tuple(shape),))
    z, y, x = (int(v) for v in shape)
    if 3 * z * y * x > INT32_MAX or _lib.MESH_MAX_TRIANGLES * (z - 1) * (y - 1) * (x - 1) > INT32_MAX:
        raise ValueError("a volume of shape %s may hold more vertices or faces than int32 indices reach"
                         % (tuple(shape),))
    p = MeshParams()
    p.voxel_size = float(voxel_size)
    if not (np.isfinite(p.voxel_size) and p.voxel_size > 0):
        raise ValueError("voxel_size must be finite and positive")
    p.offset_x, p.offset_y, p.offset_z = (float(v) for v in offsets_of(array_offset))
    p.iso = float(iso)
    if not np.all(np.isfinite([p.offset_x, p.offset_y, p.offset_z, p.iso])):
        raise ValueError("array_offset and iso must be finite")
    p.min_weight = float(min_weight)
    if np.isnan(p.min_weight):
        raise ValueError("min_weight must not be NaN")
    p.depth, p.height, p.width = z, y, x
    return p


DEFAULT_COLOUR = (128, 128, 128)


def default_colour_of(default_colour):
    """(R, G, B) as three ints after the check: three integers in 0..255"""
    c = np.asarray(default_colour)
    if c.shape != (3,) or c.dtype.kind not in "iu" or c.min() < 0 or c.max() > 255:
        raise ValueError("default_colour must be three integers in 0..255, got %r" % (default_colour,))
    return tuple(int(v) for v in c)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def extract_mesh(tsdf, weight, array_offset, voxel_size=0.004, iso=0.0, min_weight=0.0, normals=False, colour=None,
                 default_colour=DEFAULT_COLOUR):
    """lsf_mesh_count, one read of the totals, lsf_mesh_emit on the (Z, Y, X) model.  Returns (vertices (V, 3) float32,
    faces (F, 3) int32, normals (V, 3) float32 or None) as device tensors.  With colour (the model's colour volume,
    float32 (Z, Y, X, 4)) lsf_mesh_vertex_colours follows and a fourth tensor is returned: the uint8 (V, 3) vertex
    colours ("Colour fusion"), default_colour where neither end of a vertex's edge has a colour."""
    require_gpu()
    check_model(tsdf, weight)
    if colour is not None:
        check_colour_volume(colour, tsdf, weight)
        rgb = default_colour_of(default_colour)
    p = params(tuple(tsdf.shape), array_offset, voxel_size, iso, min_weight)
    dev = tsdf.device
    voxels = tsdf.numel()
    blocks = (voxels + _lib.MESH_TILE - 1) // _lib.MESH_TILE
    cell_code = torch.empty(voxels, dtype=torch.uint8, device=dev)
    edge_mask = torch.empty(voxels, dtype=torch.uint8, device=dev)
    offsets = torch.empty(2 * blocks, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    stream, P = stream_ptr(), ctypes.byref(p)
    t, w = ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr())
    check(lib.lsf_mesh_count(t, w, _ptr(cell_code), _ptr(edge_mask), _ptr(offsets), _ptr(totals), P, stream),
          "lsf_mesh_count")
    v_count, f_count = (int(v) for v in totals.tolist())  # the call's one host synchronisation
    vertices = torch.empty((v_count, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((f_count, 3), dtype=torch.int32, device=dev)
    out_normals = torch.empty((v_count, 3), dtype=torch.float32, device=dev) if normals else None
    if v_count or f_count:
        vertex_base = torch.empty(voxels, dtype=torch.int32, device=dev)
        check(lib.lsf_mesh_emit(t, w, _ptr(cell_code), _ptr(edge_mask), _ptr(offsets), _ptr(vertex_base),
                                _ptr(vertices), _ptr(out_normals), _ptr(faces), v_count, f_count, P, stream),
              "lsf_mesh_emit")
    if colour is None:
        return vertices, faces, out_normals
    colours = torch.empty((v_count, 3), dtype=torch.uint8, device=dev)
    if v_count:
        check(lib.lsf_mesh_vertex_colours(t, ctypes.c_void_p(colour.data_ptr()), _ptr(edge_mask), _ptr(vertex_base),
                                          _ptr(colours), v_count, rgb[0], rgb[1], rgb[2], P, stream),
              "lsf_mesh_vertex_colours")
    return vertices, faces, out_normals, colours
