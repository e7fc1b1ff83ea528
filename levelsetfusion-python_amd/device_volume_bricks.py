"""Torch-facing wrappers of the moving volume's brick store on the card (include/lsf_hip.h: lsf_volume_bricks_count,
_gather, _scatter; INTEGRATION.md section 3, "Brick store"; tests/volume_bricks_restatement.py restates them), and the
host rules of the lattice: brick_grid, entering_bricks / entering_flags and the leaving and entering masks of bricks.  Every argument
is checked on the host before a launch; the calls are enqueued and nothing waits.  The public interface is
fusion.BrickStore, fusion.CanonicalVolume.shift(brick_store=) and fusion.CanonicalVolume.assemble."""
import ctypes

import numpy as np
import torch

from ._lib import VOLUME_BRICK, VolumeBricksParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import _check_others, check_colour_volume, check_model
from .device_volume_shift import INT32_MAX, retained_range, shift_of

BRICK = VOLUME_BRICK
BRICK_VOXELS = BRICK ** 3
VALID_BYTES = BRICK * BRICK


def origin_of(origin):
    """g = (gx, gy, gz) as three Python ints after the check: whole numbers, exactly, each within int32"""
    g = np.asarray(origin)
    if g.shape != (3,) or g.dtype.kind not in "iuf":
        raise ValueError("the window's lattice origin must be three whole numbers (gx, gy, gz), got %r" % (origin,))
    if g.dtype.kind == "f" and not (np.all(np.isfinite(g)) and np.all(g == np.floor(g))):
        raise ValueError("the window must lie on the store's lattice: array_offset - store.origin must be whole "
                         "voxels on every axis, got %r" % (origin,))
    out = tuple(int(v) for v in g)
    if max(abs(v) for v in out) > INT32_MAX:
        raise ValueError("the window's lattice origin must fit int32, got %r" % (origin,))
    return out


def params(shape, origin, shift_voxels=(0, 0, 0)):
    """the lsf_volume_bricks_params of a call, after the host checks"""
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("the brick store needs a 3-D (Z, Y, X) volume, got shape %s" % (tuple(shape),))
    z, y, x = (int(v) for v in shape)
    if z * y * x > INT32_MAX:
        raise ValueError("a volume of shape %s has more voxels than int32 indices reach" % (tuple(shape),))
    g = origin_of(origin)
    for gj, nj in zip(g, (x, y, z)):
        if abs(gj) + nj > INT32_MAX:
            raise ValueError("lattice origin %r with shape %s leaves int32" % (g, tuple(shape)))
    p = VolumeBricksParams()
    p.depth, p.height, p.width = z, y, x
    p.origin_x, p.origin_y, p.origin_z = g
    p.shift_x, p.shift_y, p.shift_z = shift_of(shift_voxels)
    return p


def brick_grid(shape, origin):
    """the box of bricks a (Z, Y, X) window with lattice origin g = (gx, gy, gz) touches: (first, counts), the first
    brick (bx, by, bz) = floor(g / 8) and the number of bricks per axis (nbx, nby, nbz); brick b of the grid, z-major,
    is first + (b % nbx, b // nbx % nby, b // (nbx nby))"""
    g = origin_of(origin)
    n = (int(shape[2]), int(shape[1]), int(shape[0]))
    first = tuple(gj // BRICK for gj in g)
    counts = tuple((gj + nj - 1) // BRICK - f + 1 for gj, nj, f in zip(g, n, first))
    return first, counts


def grid_coords(shape, origin):
    """int32 [nbricks][3]: the lattice coordinate (bx, by, bz) of every brick of the grid, in grid order"""
    first, counts = brick_grid(shape, origin)
    bz, by, bx = np.meshgrid(*(np.arange(f, f + c, dtype=np.int32) for f, c in zip(first[::-1], counts[::-1])),
                             indexing="ij")
    return np.stack([bx.reshape(-1), by.reshape(-1), bz.reshape(-1)], axis=1)


def leaving_mask(shape, origin, shift_voxels, coords):
    """bool [K][8][8][8] (z, y, x) for bricks `coords` (int [K][3], (bx, by, bz)) of a window at lattice origin g: the
    brick voxels that lie inside the window and leave under lsf_volume_shift by s -- u - s outside the volume"""
    return _outside(shape, origin, shift_of(shift_voxels), coords)


def entering_mask(shape, origin, shift_voxels, coords):
    """as leaving_mask for the NEW window (origin = its g): the brick voxels inside the window that entered under the
    shift by s, since nothing was copied into them -- v + s outside the volume"""
    return _outside(shape, origin, tuple(-v for v in shift_of(shift_voxels)), coords)


def _outside(shape, origin, s, coords):
    """the voxels of the bricks inside the window and outside the range of source voxels a shift by s retains"""
    g = origin_of(origin)
    n = (int(shape[2]), int(shape[1]), int(shape[0]))
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    inside, kept = [], []
    for j in range(3):
        v = coords[:, j, None] * BRICK - g[j] + np.arange(BRICK)[None, :]  # window coordinate per brick and place
        r0, r1 = retained_range(n[j], max(-n[j], min(n[j], s[j])))
        inside.append((v >= 0) & (v < n[j]))
        kept.append((v >= r0) & (v < r1))
    box = lambda a: a[2][:, :, None, None] & a[1][:, None, :, None] & a[0][:, None, None, :]
    return box(inside) & ~box(kept)


def entering_flags(shape, origin, shift_voxels):
    """(first, (fx, fy, fz)): the window's first brick and per axis a bool per brick of the grid -- whether the brick's
    voxels inside the window reach outside the range that did not enter on that axis.  A brick of the grid holds a voxel
    that entered under the shift when the flag of any of its three coordinates is set."""
    g = origin_of(origin)
    s = shift_of(shift_voxels)
    n = (int(shape[2]), int(shape[1]), int(shape[0]))
    first, counts = brick_grid(shape, g)
    flags = []
    for j in range(3):
        w0 = (first[j] + np.arange(counts[j], dtype=np.int64)) * BRICK - g[j]
        r0, r1 = retained_range(n[j], max(-n[j], min(n[j], -s[j])))
        flags.append((np.maximum(w0, 0) < r0) | (np.minimum(w0 + BRICK, n[j]) > r1))
    return first, tuple(flags)


def entering_bricks(shape, origin, shift_voxels):
    """int32 [K][3]: the bricks (bx, by, bz) of the window's grid that hold a voxel which entered under the shift, in
    grid order -- the only ones a store has to be asked for"""
    _, (fx, fy, fz) = entering_flags(shape, origin, shift_voxels)
    touched = fz[:, None, None] | fy[None, :, None] | fx[None, None, :]
    return grid_coords(shape, origin)[touched.reshape(-1)]


def pack_valid(mask):
    """bool [K][8][8][8] -> uint8 [K][64]: byte r = zl * 8 + yl, bit xl"""
    return np.packbits(np.asarray(mask, dtype=bool).reshape(-1, VALID_BYTES, BRICK), axis=2,
                       bitorder="little").reshape(-1, VALID_BYTES)


def unpack_valid(valid):
    """uint8 [K][64] -> bool [K][8][8][8]"""
    v = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1, VALID_BYTES, 1)
    return np.unpackbits(v, axis=2, bitorder="little").reshape(-1, BRICK, BRICK, BRICK).astype(bool)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check_volume(tsdf, weight, colour):
    if tsdf is not None and hasattr(tsdf, "ndim") and tsdf.ndim != 3:
        raise ValueError("the brick store needs a 3-D (Z, Y, X) volume, got shape %s" % (tuple(tsdf.shape),))
    check_model(tsdf, weight)
    if colour is not None:
        check_colour_volume(colour, tsdf, weight)


def _check_buffer(name, t, dtype, shape, like, aligned=4):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, str(dtype).split(".")[-1], t.dtype))
    if t.device != like.device:
        raise ValueError("%s is on %s, the volume on %s: all buffers must be on one device" % (name, t.device,
                                                                                               like.device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, the call needs %s" % (name, tuple(t.shape), tuple(shape)))
    if t.data_ptr() % aligned:
        raise ValueError("%s must be %d-byte aligned" % (name, aligned))


def _no_alias(outs, ins):
    for i, (name, t) in enumerate(outs):
        _check_others(name, t, ins)
        _check_others(name, t, outs[i + 1:])


def count(weight, flags, offsets, total, origin, shift_voxels):
    """lsf_volume_bricks_count: per brick of the window's grid flags = 1 when a voxel of it inside the window leaves
    under the shift and holds data, offsets = the exclusive prefix of the flags in grid order, total = their sum.
    weight: float32 (Z, Y, X) device tensor; flags, offsets: int32 [nbricks]; total: int64 [1], all on its device.
    Two launches, enqueued; nothing waits."""
    require_gpu()
    if not isinstance(weight, torch.Tensor) or weight.ndim != 3:
        raise ValueError("the brick store needs a 3-D (Z, Y, X) float32 device tensor of weights")
    _check_buffer("weight", weight, torch.float32, weight.shape, weight)
    if not weight.is_cuda:
        raise ValueError("weight must be on the GPU")
    p = params(tuple(weight.shape), origin, shift_voxels)
    nbricks = int(np.prod(brick_grid(tuple(weight.shape), origin)[1]))
    _check_buffer("flags", flags, torch.int32, (nbricks,), weight)
    _check_buffer("offsets", offsets, torch.int32, (nbricks,), weight)
    _check_buffer("total", total, torch.int64, (1,), weight, aligned=8)
    _no_alias([("flags", flags), ("offsets", offsets), ("total", total)], [("weight", weight)])
    check(lib.lsf_volume_bricks_count(_ptr(weight), _ptr(flags), _ptr(offsets), _ptr(total), ctypes.byref(p),
                                      stream_ptr()), "lsf_volume_bricks_count")


def _check_rows(prefix, volume, coords, tsdf, weight, colour, valid, brick_count):
    k = int(brick_count)
    cube = (k, BRICK, BRICK, BRICK)
    _check_buffer(prefix + "coords", coords, torch.int32, (k, 3), volume)
    _check_buffer(prefix + "tsdf", tsdf, torch.float32, cube, volume)
    _check_buffer(prefix + "weight", weight, torch.float32, cube, volume)
    if colour is not None:
        _check_buffer(prefix + "colour", colour, torch.float32, cube + (4,), volume, aligned=16 if k else 1)
    _check_buffer(prefix + "valid", valid, torch.uint8, (k, VALID_BYTES), volume, aligned=1)
    rows = [(prefix + "coords", coords), (prefix + "tsdf", tsdf), (prefix + "weight", weight),
            (prefix + "valid", valid)]
    return rows + ([(prefix + "colour", colour)] if colour is not None else [])


def gather(tsdf, weight, colour, flags, offsets, brick_count, out_coords, out_tsdf, out_weight, out_colour, out_valid,
           origin, shift_voxels):
    """lsf_volume_bricks_gather, after count with the same weight, origin and shift and after the host has read its
    total into brick_count: row offsets[b] of the outputs takes flagged brick b -- out_coords int32 [K][3] (bx, by, bz),
    out_tsdf / out_weight float32 [K][8][8][8], out_colour float32 [K][8][8][8][4] (with a colour volume; both None
    otherwise), out_valid uint8 [K][64].  Every word of every row is written.  One launch, none for K = 0."""
    require_gpu()
    _check_volume(tsdf, weight, colour)
    if (colour is None) != (out_colour is None):
        raise ValueError("colour and out_colour go together: both tensors or both None")
    p = params(tuple(tsdf.shape), origin, shift_voxels)
    nbricks = int(np.prod(brick_grid(tuple(tsdf.shape), origin)[1]))
    if not 0 <= int(brick_count) <= nbricks:
        raise ValueError("brick_count must lie in [0, %d], got %r" % (nbricks, brick_count))
    _check_buffer("flags", flags, torch.int32, (nbricks,), tsdf)
    _check_buffer("offsets", offsets, torch.int32, (nbricks,), tsdf)
    outs = _check_rows("out_", tsdf, out_coords, out_tsdf, out_weight, out_colour, out_valid, brick_count)
    ins = [("tsdf", tsdf), ("weight", weight), ("colour", colour), ("flags", flags), ("offsets", offsets)]
    _no_alias(outs, ins)
    if int(brick_count) == 0:
        return
    check(lib.lsf_volume_bricks_gather(_ptr(tsdf), _ptr(weight), _ptr(colour), _ptr(flags), _ptr(offsets),
                                       int(brick_count), _ptr(out_coords), _ptr(out_tsdf), _ptr(out_weight),
                                       _ptr(out_colour), _ptr(out_valid), ctypes.byref(p), stream_ptr()),
          "lsf_volume_bricks_gather")


def scatter(coords, brick_tsdf, brick_weight, brick_colour, brick_valid, tsdf, weight, colour, origin, shift_voxels):
    """lsf_volume_bricks_scatter: IN PLACE, every voxel of the given bricks (gather's layout; distinct coordinates)
    that lies inside the window, entered under the shift and has its validity bit set is written into tsdf, weight and
    colour; nothing else is touched.  A shift with |s_j| >= n_j on some axis makes every voxel one that entered.
    One launch, none for no bricks."""
    require_gpu()
    _check_volume(tsdf, weight, colour)
    if (colour is None) != (brick_colour is None):
        raise ValueError("colour and brick_colour go together: both tensors or both None")
    p = params(tuple(tsdf.shape), origin, shift_voxels)
    if not isinstance(coords, torch.Tensor) or coords.ndim != 2:
        raise ValueError("coords must be an int32 [K][3] device tensor")
    ins = _check_rows("brick_", tsdf, coords, brick_tsdf, brick_weight, brick_colour, brick_valid, coords.shape[0])
    _no_alias([("tsdf", tsdf), ("weight", weight)] + ([("colour", colour)] if colour is not None else []), ins)
    if coords.shape[0] == 0:
        return
    check(lib.lsf_volume_bricks_scatter(_ptr(coords), _ptr(brick_tsdf), _ptr(brick_weight), _ptr(brick_colour),
                                        _ptr(brick_valid), int(coords.shape[0]), _ptr(tsdf), _ptr(weight),
                                        _ptr(colour), ctypes.byref(p), stream_ptr()), "lsf_volume_bricks_scatter")
