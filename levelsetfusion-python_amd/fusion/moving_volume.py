"""MovingVolume, the policy of a window that follows the camera, and merge_meshes, which joins the meshes of what left
it to the window's (the package's docstring, "Moving volume").  Host only."""
import numpy as np

from ..math_utils.transformation import twist_vector_to_matrix3d
from ..tsdf.generation import offsets_of


class MovingVolume:
    """the policy of a window that follows the camera in whole-voxel steps (package docstring, "Moving volume").  Host
    only.  threshold_voxels: positive; the window stays while the anchor is within that many voxels of its centre on
    every axis.  anchor: the point in CAMERA coordinates (metres) the window keeps near its centre, (0, 0, depth) some
    way in front of the lens -- the model is where the camera looks; it has no default, since no depth is right
    across scenes.  stream_mesh, min_weight, normals: whether and how SequenceFusion3d meshes the cells that leave.
    keep_tsdf: SequenceFusion3d keeps what leaves with data in it as bricks (its `brick_store`) and writes back what
    the window re-enters; it does not combine with stream_mesh, which would mesh a re-entered region twice, and since
    stream_mesh defaults to True, keep_tsdf=True needs stream_mesh=False said explicitly."""

    def __init__(self, threshold_voxels, anchor, stream_mesh=True, min_weight=0.0, normals=False, keep_tsdf=False):
        if keep_tsdf and stream_mesh:
            raise ValueError("keep_tsdf=True does not combine with stream_mesh=True (a region the window re-enters "
                             "would be meshed twice); stream_mesh defaults to True, so pass stream_mesh=False "
                             "explicitly with keep_tsdf=True")
        self.keep_tsdf = bool(keep_tsdf)
        self.threshold_voxels = float(threshold_voxels)
        if not (np.isfinite(self.threshold_voxels) and self.threshold_voxels > 0):
            raise ValueError("threshold_voxels must be finite and positive, got %r" % (threshold_voxels,))
        a = np.asarray(anchor, dtype=np.float64).reshape(-1)
        if a.size != 3 or not np.all(np.isfinite(a)):
            raise ValueError("anchor must be three finite camera coordinates in metres, got %r" % (anchor,))
        self.anchor = a.copy()
        self.min_weight = float(min_weight)
        if np.isnan(self.min_weight):
            raise ValueError("min_weight must not be NaN")
        self.stream_mesh, self.normals = bool(stream_mesh), bool(normals)

    def shift_for(self, twist, array_offset, shape, voxel_size):
        """(sx, sy, sz), Python ints, all zero for "stay".  The anchor goes to world coordinates by the inverse of
        twist_vector_to_matrix3d of the float32-rounded twist (the generator's convention, raycast's); d is its
        position in voxels minus the window's centre array_offset + (n - 1) / 2 per axis, in float64.  While no |d_j|
        exceeds the threshold the window stays; otherwise the shift is trunc(d_j) on EVERY axis, so one shift
        re-centres all three and shifts stay rare.  shape is the model's (Z, Y, X)."""
        if len(shape) != 3:
            raise ValueError("a moving volume needs a 3-D (Z, Y, X) model, got shape %s" % (tuple(shape),))
        if not (np.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError("voxel_size must be finite and positive")
        t32 = np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32)
        m = twist_vector_to_matrix3d(t32)  # world -> camera
        rot, t = m[:3, :3].astype(np.float64), m[:3, 3].astype(np.float64)
        world = rot.T @ (self.anchor - t)
        n = np.array([shape[2], shape[1], shape[0]], dtype=np.float64)  # x, y, z
        d = world / float(voxel_size) - (offsets_of(array_offset) + (n - 1.0) / 2.0)
        if not np.all(np.isfinite(d)):
            raise ValueError("the anchor's world position is not finite under twist %r" % (twist,))
        if not np.any(np.abs(d) > self.threshold_voxels):
            return (0, 0, 0)
        return tuple(int(v) for v in np.trunc(d))


def _mesh_layout(mesh):
    """(with normals, with colours) of a mesh tuple in extract_mesh's layout, host arrays or tensors: (V, F), (V, F, N),
    (V, F, C) or (V, F, N, C), C being uint8"""
    if not isinstance(mesh, (tuple, list)) or not 2 <= len(mesh) <= 4:
        raise ValueError("a mesh is a tuple (vertices, faces[, normals][, colours])")
    extras = [a if hasattr(a, "dtype") else np.asarray(a) for a in mesh[2:]]
    coloured = bool(extras) and str(extras[-1].dtype).split(".")[-1] == "uint8"  # numpy's or torch's
    with_normals = len(extras) - int(coloured) == 1
    if len(extras) - int(coloured) not in (0, 1):
        raise ValueError("a mesh is a tuple (vertices, faces[, normals][, colours])")
    return with_normals, coloured


def merge_meshes(meshes, weld=False):
    """the concatenation of host meshes in extract_mesh's layout (numpy tuples (vertices, faces[, normals][, colours])):
    vertices, normals and colours stacked in order, every mesh's face indices offset by the vertices before it.
    Without weld nothing is welded: a seam's vertices appear once per mesh.  With weld the concatenation goes through
    simplify_mesh on the device, which makes one vertex of the vertices whose positions are equal bit for bit (package
    docstring, "Mesh simplification").  Meshes of different layouts are refused, and so is an empty list: it has no
    layout."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError("merge_meshes needs at least one mesh")
    layout = _mesh_layout(meshes[0])
    for m in meshes[1:]:
        if _mesh_layout(m) != layout:
            raise ValueError("merge_meshes needs meshes of one layout (normals and colours in all or in none)")
    counts = [len(m[0]) for m in meshes]
    if sum(counts) > 0x7fffffff:
        raise ValueError("the merged mesh has more vertices than int32 face indices reach")
    bases = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    out = [np.concatenate([np.asarray(m[0], dtype=np.float32).reshape(-1, 3) for m in meshes]),
           np.concatenate([np.asarray(m[1], dtype=np.int32).reshape(-1, 3) + b for m, b in zip(meshes, bases)])]
    for j in range(2, len(meshes[0])):
        out.append(np.concatenate([np.asarray(m[j]).reshape(-1, 3) for m in meshes]))
    if weld:
        from .mesh_simplify import simplify_mesh
        return simplify_mesh(tuple(out))
    return tuple(out)
