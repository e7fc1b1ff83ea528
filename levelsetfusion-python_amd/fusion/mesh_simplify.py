"""simplify_mesh: welding and vertex-clustering decimation of a mesh in extract_mesh's layout (the package's docstring
has the rule)."""
import numpy as np
import torch

from .. import device_mesh_simplify
from ..device_core import require_gpu
from .moving_volume import _mesh_layout


def _checked(a, dtype, name):
    """a tensor as it is (the device wrapper checks it); a host array after the checks of its type and shape"""
    if isinstance(a, torch.Tensor):
        return a
    a = np.asarray(a)
    if a.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, np.dtype(dtype).name, a.dtype))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must have shape (N, 3), got %s" % (name, a.shape))
    return a


def _as_device(a):
    if isinstance(a, torch.Tensor):
        return a if a.is_cuda else a.to("cuda")
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def simplify_mesh(mesh, cell_size=None, origin=(0.0, 0.0, 0.0), as_tensor=False, return_record=False):
    """mesh: (vertices, faces[, normals][, colours]) in extract_mesh's layout, host arrays or device tensors.  With
    cell_size None the vertices whose positions are equal bit for bit become one (welding, what closes the seams of
    merge_meshes); with a cell size every vertex of one cell of the lattice of that edge through origin becomes one
    vertex at the members' mean (vertex-clustering decimation).  Faces are remapped, faces that collapse are dropped,
    of faces that land on one vertex triple one survives (none when they fold onto each other), and vertices no face
    uses are removed.  Returns the mesh in the same layout -- numpy copies, or device tensors with as_tensor -- and with
    return_record the record dict behind it.  A non-finite vertex or a face index outside the vertices raises
    ValueError.  One host synchronisation: the read of the record."""
    with_normals, coloured = _mesh_layout(mesh)
    p = device_mesh_simplify.params(len(mesh[0]), len(mesh[1]), cell_size, origin, None, with_normals, coloured)
    del p  # the checks that need no device, before anything is copied to it
    v = _checked(mesh[0], np.float32, "vertices")
    f = _checked(mesh[1], np.int32, "faces")
    n = _checked(mesh[2], np.float32, "normals") if with_normals else None
    c = _checked(mesh[-1], np.uint8, "colours") if coloured else None
    require_gpu()
    out = device_mesh_simplify.simplify(_as_device(v), _as_device(f), None if n is None else _as_device(n),
                                        None if c is None else _as_device(c), cell_size, origin)
    kept = tuple(t for t in out[:4] if t is not None)
    if not as_tensor:
        kept = tuple(t.cpu().numpy() for t in kept)
    return kept + (out[4],) if return_record else kept
