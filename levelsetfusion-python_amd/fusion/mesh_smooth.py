"""smooth_mesh and mesh_vertex_normals: Taubin smoothing of a mesh in extract_mesh's layout with its open borders held
in place, and area-weighted vertex normals from the faces (the package's docstring has the rule)."""
import numpy as np

from .. import device_mesh_smooth
from ..device_core import require_gpu
from .mesh_simplify import _as_device, _checked
from .moving_volume import _mesh_layout


def _inputs(mesh, **call):
    """the mesh's arrays after the checks that need no device: (vertices, faces, normals or None, colours or None)"""
    with_normals, coloured = _mesh_layout(mesh)
    p = device_mesh_smooth.params(len(mesh[0]), len(mesh[1]), **call)
    del p  # the checks of the sizes and of the call's arguments, before anything is copied to the device
    v = _checked(mesh[0], np.float32, "vertices")
    f = _checked(mesh[1], np.int32, "faces")
    n = _checked(mesh[2], np.float32, "normals") if with_normals else None
    c = _checked(mesh[-1], np.uint8, "colours") if coloured else None
    return v, f, n, c


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", recompute_normals=True, as_tensor=False,
                return_record=False):
    """mesh: (vertices, faces[, normals][, colours]) in extract_mesh's layout, host arrays or device tensors.  Every
    iteration is a pass with weight lam and, unless mu is 0, a pass with weight mu (Taubin's lambda | mu, which does not
    shrink the model as plain Laplacian passes -- mu=0.0 -- do): a pass moves every vertex by the weight times the way
    to the mean of its edge neighbours.  With boundary="fixed" the ends of every edge that does not have exactly two
    faces -- open borders, seams, non-manifold edges -- stay bit for bit, with "free" nothing is pinned; a vertex without
    an edge always stays.  Vertex count and order, faces and colours are unchanged, iterations=0 returns the positions
    bit for bit.  Normals, when the mesh has them, are rebuilt from the smoothed faces (mesh_vertex_normals) unless
    recompute_normals=False, which carries them bit for bit.  Returns the mesh in the same layout -- numpy copies, or
    device tensors with as_tensor -- and with return_record the record dict behind it.  ValueError: iterations not a
    whole number in 0 .. 1000, lam not finite or outside (0, 1], mu not finite or > 0, another boundary, a layout that
    is none of extract_mesh's, and after the read of the record a non-finite vertex or a face index outside the
    vertices.  One host synchronisation, the read of the record; return_record=True reads it a second time."""
    v, f, n, c = _inputs(mesh, iterations=iterations, lam=lam, mu=mu, boundary=boundary)
    require_gpu()
    out = device_mesh_smooth.smooth(_as_device(v), _as_device(f), None if n is None else _as_device(n),
                                    None if c is None else _as_device(c), iterations, lam, mu, boundary,
                                    recompute_normals, return_record)
    kept = tuple(t for t in out[:4] if t is not None)
    if not as_tensor:
        kept = tuple(t.cpu().numpy() for t in kept)
    return kept + (out[4],) if return_record else kept


def mesh_vertex_normals(mesh, as_tensor=False):
    """float32 (V, 3): the area-weighted vertex normals of a mesh in extract_mesh's layout, from its faces alone -- every
    face adds the cross product of its edges, the right-hand normal that extract_mesh's faces turn towards larger tsdf,
    to its three vertices, and the sums are scaled to length 1; (0, 0, 0) where the faces around a vertex sum to no
    length.  What the normals of a mesh are after its vertices moved, or after simplify_mesh averaged them.  A numpy
    copy, or a device tensor with as_tensor.  A non-finite vertex or a face index outside the vertices raises
    ValueError.  One host synchronisation: the read of the record."""
    v, f, _, _ = _inputs(mesh, iterations=0)
    require_gpu()
    normals, _ = device_mesh_smooth.vertex_normals(_as_device(v), _as_device(f))
    return normals if as_tensor else normals.cpu().numpy()
