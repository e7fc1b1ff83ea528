"""Numpy restatements of the moving volume ("Moving volume"), which the HIP kernel
(lsf_volume_shift in csrc/lsf_volume_shift.hip) and the host rules of the package (device_volume_shift.leaving_boxes,
fusion.MovingVolume.shift_for) must equal: the shifted copy as slice assignment on uint32 views, the boxes of cells that
leave, and the policy.  Host numpy only; none of it calls the package's own versions."""
import numpy as np

import rigid_restatement as R

TSDF_FILL = np.float32(1.0).view(np.uint32)
WEIGHT_FILL = np.uint32(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.uint32)
    return a.view(np.uint32)


def retained(n, s):
    """the voxels [r0, r1) of an axis of n that a shift by s keeps; (0, 0) when none"""
    r0, r1 = max(0, s), min(n, n + s)
    return (r0, r1) if r0 < r1 else (0, 0)


def shift_array(a, shift, fill):
    """dst(v) = src(v + s) inside, `fill` (a uint32 pattern) elsewhere, for a (Z, Y, X[, C]) float32 array; the shift is
    (sx, sy, sz).  Works on the bit patterns, so NaN payloads and -0.0 survive.  Returns float32."""
    src = _bits(a)
    out = np.full(src.shape, fill, dtype=np.uint32)
    sx, sy, sz = (int(v) for v in shift)
    ranges = [retained(n, s) for n, s in zip(src.shape[:3], (sz, sy, sx))]
    if all(r1 > r0 for r0, r1 in ranges):
        (z0, z1), (y0, y1), (x0, x1) = ranges
        out[z0 - sz:z1 - sz, y0 - sy:y1 - sy, x0 - sx:x1 - sx] = src[z0:z1, y0:y1, x0:x1]
    return out.view(np.float32)


def shift_model(tsdf, weight, colour, shift):
    """(tsdf, weight, colour or None) after the shift: empty voxels are tsdf 1, weight 0, colour record 0"""
    return (shift_array(tsdf, shift, TSDF_FILL), shift_array(weight, shift, WEIGHT_FILL),
            None if colour is None else shift_array(colour, shift, np.uint32(0)))


def retained_mask(shape, shift):
    """bool (Z, Y, X): the DESTINATION voxels that hold a source voxel"""
    return shift_array(np.ones(shape, np.float32), shift, np.uint32(0)) != 0


def leaving_cell_mask(shape, shift):
    """bool over the cells (Z - 1, Y - 1, X - 1) of the OLD volume: the cell leaves when any of its 8 corners does"""
    z, y, x = shape
    sx, sy, sz = (int(v) for v in shift)
    keep = np.zeros(shape, bool)
    (z0, z1), (y0, y1), (x0, x1) = retained(z, sz), retained(y, sy), retained(x, sx)
    keep[z0:z1, y0:y1, x0:x1] = True
    all_corners = np.ones((z - 1, y - 1, x - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                all_corners &= keep[dz:z - 1 + dz, dy:y - 1 + dy, dx:x - 1 + dx]
    return ~all_corners


def leaving_boxes(shape, shift):
    """the leaving cells as boxes ((x0, x1), (y0, y1), (z0, z1)) of cells, by the rule of the document: per axis the
    retained cells are [r0, r1 - 1); the x-slab spans the full y and z cell ranges, the y-slab the retained x cells, the
    z-slab the retained x and y cells; when no cell is retained the one box is every cell"""
    n = (shape[2], shape[1], shape[0])
    full = [(0, m - 1) for m in n]
    kept = []
    for m, s in zip(n, (int(v) for v in shift)):
        r0, r1 = retained(m, s)
        kept.append((r0, r1 - 1))
    if any(b <= a for a, b in kept):
        return [tuple(full)] if all(b > a for a, b in full) else []
    boxes = []
    for axis in range(3):
        below, above = (0, kept[axis][0]), (kept[axis][1], n[axis] - 1)
        for part in (below, above):
            box = [kept[j] if j < axis else full[j] for j in range(3)]
            box[axis] = part
            if all(b > a for a, b in box):
                boxes.append(tuple(box))
    return boxes


def policy_shift(anchor, threshold, twist, array_offset, shape, voxel_size):
    """(sx, sy, sz): the anchor (camera coordinates, metres) in world coordinates by the inverse of the generator's
    world -> camera matrix of the float32-rounded twist; d = its voxel position minus the window's centre
    array_offset + (n - 1) / 2; zero while no |d_j| exceeds the threshold, else trunc(d) on every axis"""
    t32 = np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32)
    m = R.matrix3d(t32)
    rot, t = np.asarray(m[:3, :3], np.float64), np.asarray(m[:3, 3], np.float64)
    world = rot.T @ (np.asarray(anchor, np.float64) - t)
    n = np.array([shape[2], shape[1], shape[0]], np.float64)
    d = world / voxel_size - (np.asarray(array_offset, np.float64).reshape(3) + (n - 1) / 2)
    if not np.any(np.abs(d) > threshold):
        return (0, 0, 0)
    return tuple(int(v) for v in np.trunc(d))
