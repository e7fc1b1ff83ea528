"""Numpy restatements of the moving volume's brick store ("Brick store"), which the HIP kernels
(lsf_volume_bricks_count / _gather / _scatter in csrc/lsf_volume_bricks.hip), the package's host rules
(device_volume_bricks.brick_grid, entering_bricks) and fusion.BrickStore's merge and clear rules must equal.  Written from
the contract: the window is laid into a padded array that covers its brick grid, and bricks are that array cut by
reshape -- no per-brick index arithmetic like the kernels'.  The shift itself is volume_shift_restatement's.  Host numpy
only; none of it calls the package's own versions."""
import numpy as np

import volume_shift_restatement as V

BRICK = 8
DATA_BITS = np.uint32(0x7fffffff)
EMPTY = (V.TSDF_FILL, np.uint32(0), np.uint32(0))  # tsdf, weight, every word of the colour record


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.uint32)
    return a.view(np.uint32)


def holds_data(weight):
    """any non-zero weight, a NaN included: the low 31 bits"""
    return (_u32(weight) & DATA_BITS) != 0


def floor_div(a, d=BRICK):
    """floor(a / d) for Python ints of any sign, without // : by counting down or up from zero"""
    q = int(abs(a)) // d
    if a >= 0:
        return q
    return -q if q * d == -a else -q - 1


def brick_grid(shape, g):
    """(first, counts): the first brick (bx, by, bz) the window touches and the bricks per axis (x, y, z)"""
    n = (shape[2], shape[1], shape[0])
    first = tuple(floor_div(gj) for gj in g)
    counts = tuple(floor_div(gj + nj - 1) - f + 1 for gj, nj, f in zip(g, n, first))
    return first, counts


def grid_coords(shape, g):
    """int32 [nbricks][3], rows (bx, by, bz), z-major with x fastest"""
    first, counts = brick_grid(shape, g)
    return np.array([(first[0] + i, first[1] + j, first[2] + k) for k in range(counts[2]) for j in range(counts[1])
                     for i in range(counts[0])], np.int32).reshape(-1, 3)


def entering(shape, shift):
    """bool (Z, Y, X) over the NEW window: nothing was copied into v, since v + s lies outside the volume"""
    return ~V.retained_mask(shape, shift)


def leaving(shape, shift):
    """bool (Z, Y, X) over the OLD window: u is no destination voxel's source, since u - s lies outside the volume
    (s clamped to [-n, n])"""
    z, y, x = shape
    sx, sy, sz = (max(-n, min(n, int(s))) for s, n in zip(shift, (x, y, z)))
    keep = np.zeros(shape, bool)
    (z0, z1), (y0, y1), (x0, x1) = V.retained(z, sz), V.retained(y, sy), V.retained(x, sx)
    keep[z0:z1, y0:y1, x0:x1] = True
    return ~keep


def _pad(a, shape, g, fill):
    """the window array `a` ((Z, Y, X) + extra) laid into an array over its whole brick grid, `fill` around it"""
    first, counts = brick_grid(shape, g)
    full = np.full((counts[2] * BRICK, counts[1] * BRICK, counts[0] * BRICK) + a.shape[3:], fill, a.dtype)
    x0, y0, z0 = (gj - f * BRICK for gj, f in zip(g, first))
    full[z0:z0 + shape[0], y0:y0 + shape[1], x0:x0 + shape[2]] = a
    return full


def _window(full, shape, g):
    first, _ = brick_grid(shape, g)
    x0, y0, z0 = (gj - f * BRICK for gj, f in zip(g, first))
    return full[z0:z0 + shape[0], y0:y0 + shape[1], x0:x0 + shape[2]]


def _cut(full):
    """(nbz 8, nby 8, nbx 8) + extra -> [nbricks][8][8][8] + extra, in grid order"""
    nz, ny, nx = (v // BRICK for v in full.shape[:3])
    extra = full.shape[3:]
    a = full.reshape((nz, BRICK, ny, BRICK, nx, BRICK) + extra)
    order = (0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(extra)))
    return a.transpose(order).reshape((nz * ny * nx, BRICK, BRICK, BRICK) + extra)


def _uncut(bricks, counts):
    """the inverse of _cut for a grid of counts = (nbx, nby, nbz)"""
    nx, ny, nz = counts
    extra = bricks.shape[4:]
    a = bricks.reshape((nz, ny, nx, BRICK, BRICK, BRICK) + extra)
    order = (0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(extra)))
    return a.transpose(order).reshape((nz * BRICK, ny * BRICK, nx * BRICK) + extra)


def pack_valid(mask):
    """bool [K][8][8][8] -> uint8 [K][64]: byte zl * 8 + yl, bit xl"""
    m = np.asarray(mask, bool).reshape(-1, 64, 8)
    return (m * (1 << np.arange(8))[None, None, :]).sum(axis=2).astype(np.uint8)


def unpack_valid(valid):
    v = np.asarray(valid, np.uint8).reshape(-1, 64, 1)
    return ((v >> np.arange(8)[None, None, :]) & 1).astype(bool).reshape(-1, 8, 8, 8)


def leaving_data_bricks(weight, g, shift):
    """bool [nbricks][8][8][8]: per brick of the grid, the voxels inside the window that leave and hold data"""
    shape = weight.shape
    return _cut(_pad(leaving(shape, shift) & holds_data(weight), shape, g, False))


def count(weight, g, shift):
    """(flags int32 [nbricks], offsets int32 [nbricks], total int)"""
    flags = leaving_data_bricks(weight, g, shift).reshape(-1, BRICK ** 3).any(axis=1).astype(np.int32)
    offsets = (np.cumsum(flags) - flags).astype(np.int32)
    return flags, offsets, int(flags.sum())


def gather(tsdf, weight, colour, g, shift):
    """(coords int32 [K][3], tsdf uint32 [K][8][8][8], weight uint32 [K][8][8][8], colour uint32 [K][8][8][8][4] or
    None, valid uint8 [K][64]) of the flagged bricks, in grid order"""
    shape = weight.shape
    keep = leaving_data_bricks(weight, g, shift)
    flagged = keep.reshape(len(keep), -1).any(axis=1)
    cut = lambda a, fill: _cut(_pad(_u32(a), shape, g, fill))
    t = np.where(keep, cut(tsdf, EMPTY[0]), EMPTY[0])[flagged]
    w = np.where(keep, cut(weight, EMPTY[1]), EMPTY[1])[flagged]
    c = None if colour is None else np.where(keep[..., None], cut(colour, EMPTY[2]), EMPTY[2])[flagged]
    return grid_coords(shape, g)[flagged], t, w, c, pack_valid(keep[flagged])


def scatter(coords, brick_tsdf, brick_weight, brick_colour, valid, tsdf, weight, colour, g, shift):
    """(tsdf, weight, colour or None) as uint32 after the scatter in place: the brick's words where a voxel is inside
    the window, entered under `shift` and is valid; every other word as it was"""
    shape = weight.shape
    first, counts = brick_grid(shape, g)
    nb = counts[0] * counts[1] * counts[2]
    bt = np.full((nb, 8, 8, 8), EMPTY[0], np.uint32)
    bw = np.zeros((nb, 8, 8, 8), np.uint32)
    bc = np.zeros((nb, 8, 8, 8, 4), np.uint32)
    bv = np.zeros((nb, 8, 8, 8), bool)
    masks = unpack_valid(valid)
    for k, (bx, by, bz) in enumerate(np.asarray(coords).reshape(-1, 3).tolist()):
        i, j, l = bx - first[0], by - first[1], bz - first[2]
        if not (0 <= i < counts[0] and 0 <= j < counts[1] and 0 <= l < counts[2]):
            continue  # outside the window's grid
        b = (l * counts[1] + j) * counts[0] + i
        bt[b], bw[b], bv[b] = _u32(brick_tsdf)[k], _u32(brick_weight)[k], masks[k]
        if brick_colour is not None:
            bc[b] = _u32(brick_colour)[k]
    take = entering(shape, shift) & _window(_uncut(bv, counts), shape, g)
    out_t = np.where(take, _window(_uncut(bt, counts), shape, g), _u32(tsdf))
    out_w = np.where(take, _window(_uncut(bw, counts), shape, g), _u32(weight))
    out_c = None if colour is None else np.where(take[..., None], _window(_uncut(bc, counts), shape, g), _u32(colour))
    return out_t, out_w, out_c


class Store:
    """fusion.BrickStore's rules restated with a dict of whole bricks: merge (valid voxels overwrite, validity ORed),
    clear (bits off, the voxel empty again, a brick without a valid bit dropped), to_volume"""

    def __init__(self, colour=False):
        self.colour = colour
        self.bricks = {}  # (bx, by, bz) -> [tsdf, weight, colour, valid] : uint32 / bool arrays

    def merge(self, coords, tsdf, weight, colour, valid):
        masks = unpack_valid(valid)
        for k, key in enumerate(map(tuple, np.asarray(coords).reshape(-1, 3).tolist())):
            if key not in self.bricks:
                self.bricks[key] = [np.full((8, 8, 8), EMPTY[0], np.uint32), np.zeros((8, 8, 8), np.uint32),
                                    np.zeros((8, 8, 8, 4), np.uint32), np.zeros((8, 8, 8), bool)]
            b, m = self.bricks[key], masks[k]
            b[0][m], b[1][m] = _u32(tsdf)[k][m], _u32(weight)[k][m]
            if self.colour:
                b[2][m] = _u32(colour)[k][m]
            b[3] |= m

    def clear(self, coords, masks):
        for key, m in zip(map(tuple, np.asarray(coords).reshape(-1, 3).tolist()), masks):
            b = self.bricks[key]
            b[0][m], b[1][m], b[2][m] = EMPTY[0], EMPTY[1], EMPTY[2]
            b[3] &= ~m
            if not b[3].any():
                del self.bricks[key]

    def coords(self):
        keys = sorted(self.bricks, key=lambda k: (k[2], k[1], k[0]))
        return np.array(keys, np.int32).reshape(-1, 3)

    def voxel_count(self):
        return int(sum(b[3].sum() for b in self.bricks.values()))

    def to_volume(self, lo, hi):
        """(tsdf, weight, colour) uint32 over the lattice box [lo, hi), (x, y, z); the empty voxel where nothing is
        valid"""
        shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        t = np.full(shape, EMPTY[0], np.uint32)
        w = np.zeros(shape, np.uint32)
        c = np.zeros(shape + (4,), np.uint32)
        for (bx, by, bz), b in self.bricks.items():
            for zl, yl, xl in zip(*np.nonzero(b[3])):
                x, y, z = bx * 8 + xl - lo[0], by * 8 + yl - lo[1], bz * 8 + zl - lo[2]
                if 0 <= x < shape[2] and 0 <= y < shape[1] and 0 <= z < shape[0]:
                    t[z, y, x], w[z, y, x], c[z, y, x] = b[0][zl, yl, xl], b[1][zl, yl, xl], b[2][zl, yl, xl]
        return t, w, c
