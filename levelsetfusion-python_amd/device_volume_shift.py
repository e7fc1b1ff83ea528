"""Torch-facing wrapper of the moving volume's shifted copy (include/lsf_hip.h: lsf_volume_shift; INTEGRATION.md section
3, "Moving volume"; tests/volume_shift_restatement.py restates it).  Every argument is checked on the host before the
launch; the call is enqueued and nothing waits.  leaving_boxes is the host rule for the cells a shift drops.  The
public interface is fusion.CanonicalVolume.shift and fusion.MovingVolume."""
import ctypes

import numpy as np

from ._lib import VolumeShiftParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import _check_others, check_colour_volume, check_model

INT32_MAX = 0x7fffffff


def shift_of(shift_voxels):
    """(sx, sy, sz) as three Python ints after the check: three integers (numpy ints too, and floats without a
    fraction), each within int32"""
    s = np.asarray(shift_voxels)
    if s.shape != (3,) or s.dtype.kind not in "iuf":
        raise ValueError("shift_voxels must be three integers (sx, sy, sz), got %r" % (shift_voxels,))
    if s.dtype.kind == "f" and not (np.all(np.isfinite(s)) and np.all(s == np.trunc(s))):
        raise ValueError("shift_voxels must be whole voxels, got %r" % (shift_voxels,))
    out = tuple(int(v) for v in s)
    if max(abs(v) for v in out) > INT32_MAX:
        raise ValueError("shift_voxels must fit int32, got %r" % (shift_voxels,))
    return out


def retained_range(n, s):
    """the voxels [r0, r1) of an axis of n voxels that a shift by s keeps (they move to [r0 - s, r1 - s)); empty as
    (0, 0)"""
    r0, r1 = max(0, s), min(n, n + s)
    return (r0, r1) if r0 < r1 else (0, 0)


def leaving_boxes(shape, shift_voxels):
    """the CELLS of a (Z, Y, X) volume that a shift drops -- a cell is the cube between voxel c and c + 1 and leaves
    when any of its 8 corners does -- as at most three disjoint boxes of cells [((x0, x1), (y0, y1), (z0, z1)), ...]:
    the x-slab(s) over the full y and z cell ranges, the y-slab(s) over the retained x cells, the z-slab(s) over the
    retained x and y cells.  A shift is one-sided per axis, so each slab is one box.  When nothing is retained the one
    box is every cell.  Empty boxes are left out; a zero shift gives none."""
    z, y, x = (int(v) for v in shape)
    n = (x, y, z)
    s = shift_of(shift_voxels)
    cells = [(0, max(m - 1, 0)) for m in n]
    kept = []
    for m, sj in zip(n, s):
        r0, r1 = retained_range(m, sj)
        kept.append((r0, max(r1 - 1, r0)))  # retained cells [r0, r1 - 1)
    if any(k[0] >= k[1] for k in kept):  # no cell survives
        return [tuple(cells)] if all(c[0] < c[1] for c in cells) else []
    boxes = []
    for axis in range(3):
        lo, hi = cells[axis]
        k0, k1 = kept[axis]
        for a, b in ((lo, k0), (k1, hi)):  # the cells below and above the retained ones: at most one is non-empty
            if a >= b:
                continue
            box = [kept[j] if j < axis else cells[j] for j in range(3)]
            box[axis] = (a, b)
            if all(c[0] < c[1] for c in box):
                boxes.append(tuple(box))
    return boxes


def params(shape, shift_voxels):
    """the lsf_volume_shift_params of a call, after the host checks"""
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("a volume shift needs a 3-D (Z, Y, X) volume, got shape %s" % (tuple(shape),))
    z, y, x = (int(v) for v in shape)
    if z * y * x > INT32_MAX:
        raise ValueError("a volume of shape %s has more voxels than int32 indices reach" % (tuple(shape),))
    p = VolumeShiftParams()
    p.depth, p.height, p.width = z, y, x
    p.shift_x, p.shift_y, p.shift_z = shift_of(shift_voxels)
    return p


def shift(tsdf, weight, colour, out_tsdf, out_weight, out_colour, shift_voxels):
    """lsf_volume_shift: out(v) = in(v + s) where v + s = (x + sx, y + sy, z + sz) lies inside the (Z, Y, X) volume,
    else the empty voxel (tsdf 1, weight 0, colour record 0).  tsdf, weight, out_tsdf, out_weight: float32 contiguous
    device tensors of one 3-D shape; colour, out_colour: both None, or float32 of that shape + (4,), 16-byte aligned.
    No output may share memory with an input or another output.  One launch, enqueued; nothing waits."""
    require_gpu()
    if tsdf is not None and hasattr(tsdf, "ndim") and tsdf.ndim != 3:
        raise ValueError("a volume shift needs a 3-D (Z, Y, X) volume, got shape %s" % (tuple(tsdf.shape),))
    check_model(tsdf, weight)
    check_model(out_tsdf, out_weight)
    if tuple(out_tsdf.shape) != tuple(tsdf.shape) or out_tsdf.device != tsdf.device:
        raise ValueError("out_tsdf has shape %s on %s, tsdf %s on %s: source and destination must have one shape on "
                         "one device" % (tuple(out_tsdf.shape), out_tsdf.device, tuple(tsdf.shape), tsdf.device))
    if (colour is None) != (out_colour is None):
        raise ValueError("colour and out_colour go together: both tensors or both None")
    p = params(tuple(tsdf.shape), shift_voxels)
    ins = [("tsdf", tsdf), ("weight", weight)]
    outs = [("out_tsdf", out_tsdf), ("out_weight", out_weight)]
    if colour is not None:
        check_colour_volume(colour, tsdf, weight)
        check_colour_volume(out_colour, out_tsdf, out_weight)
        ins.append(("colour", colour))
        outs.append(("out_colour", out_colour))
    for name, t in outs:
        _check_others(name, t, ins)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    check(lib.lsf_volume_shift(ptr(tsdf), ptr(weight), ptr(colour), ptr(out_tsdf), ptr(out_weight), ptr(out_colour),
                               ctypes.byref(p), stream_ptr()), "lsf_volume_shift")
