"""mesh_components and filter_mesh_components: the connected components of a mesh in extract_mesh's layout, and the
mesh without the components one does not want (the package's docstring has the rule)."""
import numpy as np

from .. import device_mesh_components
from ..device_core import require_gpu
from .mesh_simplify import _as_device, _checked
from .moving_volume import _mesh_layout


def _inputs(mesh):
    """the mesh's arrays after the checks that need no device: (vertices, faces, normals or None, colours or None)"""
    with_normals, coloured = _mesh_layout(mesh)
    p = device_mesh_components.params(len(mesh[0]), len(mesh[1]), with_normals, coloured)
    del p  # the checks of the sizes, before anything is copied to the device
    v = _checked(mesh[0], np.float32, "vertices")
    f = _checked(mesh[1], np.int32, "faces")
    n = _checked(mesh[2], np.float32, "normals") if with_normals else None
    c = _checked(mesh[-1], np.uint8, "colours") if coloured else None
    return v, f, n, c


def mesh_components(mesh, as_tensor=False):
    """mesh: (vertices, faces[, normals][, colours]) in extract_mesh's layout, host arrays or device tensors.  Two
    vertices are connected when some face names both; a component is a connected set of vertices, and its label is the
    smallest vertex index in it.  Returns (vertex_labels int32 (V,), face_labels int32 (F,), table): a face's label is
    the label of its first vertex; table is a dict of labels, vertex_counts, face_counts int32 (C,) and bounds float32
    (C, 2, 3) -- the minimum and maximum of the members' positions -- for the C components in ascending label order.
    numpy copies, or device tensors with as_tensor.  A non-finite vertex or a face index outside the vertices raises
    ValueError.  One host synchronisation: the read of the record."""
    v, f, _, _ = _inputs(mesh)
    require_gpu()
    vertex_labels, face_labels, table = device_mesh_components.components(_as_device(v), _as_device(f))
    if as_tensor:
        return vertex_labels, face_labels, table
    return (vertex_labels.cpu().numpy(), face_labels.cpu().numpy(), {k: t.cpu().numpy() for k, t in table.items()})


def filter_mesh_components(mesh, min_faces=None, min_vertices=None, min_extent=None, keep_largest=None, as_tensor=False,
                           return_record=False):
    """The mesh without the components that fail a criterion.  A component passes when it meets every threshold that is
    given: face count >= min_faces, vertex count >= min_vertices, the longest edge of its bounds >= min_extent (compared
    in float64 of the float32 bounds).  With keep_largest = k only the first k passing components stay, in the order
    face count descending, label ascending.  Kept vertices and faces keep their input order, faces are re-indexed,
    normals and colours are carried bit for bit.  Returns the mesh in the same layout -- numpy copies, or device tensors
    with as_tensor -- and with return_record the record dict behind it.  No criterion at all, a non-finite vertex or a
    face index outside the vertices raises ValueError.  Two host synchronisations: the reads of the record for the
    table's size and for the outputs' sizes."""
    device_mesh_components.criteria(min_faces, min_vertices, min_extent, keep_largest)
    v, f, n, c = _inputs(mesh)
    require_gpu()
    out = device_mesh_components.filter(_as_device(v), _as_device(f), None if n is None else _as_device(n),
                                        None if c is None else _as_device(c), min_faces, min_vertices, min_extent,
                                        keep_largest)
    kept = tuple(t for t in out[:4] if t is not None)
    if not as_tensor:
        kept = tuple(t.cpu().numpy() for t in kept)
    return kept + (out[4],) if return_record else kept
