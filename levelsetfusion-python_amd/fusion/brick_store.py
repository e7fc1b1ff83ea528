"""The host side of the moving volume's brick store ("Brick store";
tests/volume_bricks_restatement.py restates its merge and clear rules): the bricks that left the window, keyed by their
lattice coordinate, in numpy arrays that grow by doubling.  Host numpy only; the card's side is device_volume_bricks."""
import numpy as np

from ..device_volume_bricks import BRICK, VALID_BYTES, origin_of, pack_valid, unpack_valid

TSDF_EMPTY = np.float32(1.0).view(np.uint32)
_CUBE = (BRICK, BRICK, BRICK)


def _words(a, shape):
    """a float32 (or uint32) array as uint32 words of `shape`: values are kept as bits, NaN payloads and -0.0 included"""
    a = np.ascontiguousarray(a)
    if a.dtype not in (np.float32, np.uint32):
        raise ValueError("brick values must be float32, got %s" % a.dtype)
    return a.view(np.uint32).reshape(shape)


class BrickStore:
    """what left a moving window, kept as 8^3 bricks on an integer lattice (module docstring of fusion, "Brick
    store").  Host only.  Per stored brick: its lattice coordinate (bx, by, bz), `tsdf` and `weight` as float32
    [8][8][8] (z, y, x), with colour=True the colour records float32 [8][8][8][4], and 64 validity bytes (byte
    zl * 8 + yl, bit xl) that say where the store's copy is the authoritative one.  The contract: a lattice voxel with
    data lives in exactly one place, the window or the store -- a voxel inside the current window is never valid here.
    A voxel that left without data is not kept and comes back as the empty voxel (tsdf 1, weight 0, colour 0).
    `origin` is the array_offset (float64 (3,), fractions allowed) of the first shift that used the store: it fixes the
    lattice, and every later window must lie a whole number of voxels from it.  `last` counts the latest shift:
    bricks_out / voxels_out merged in, bricks_in / voxels_in written back to the window.  clear() drops the bricks and
    keeps the lattice."""

    def __init__(self, colour=False):
        self.colour = bool(colour)
        self.origin = None
        self.clear()

    def clear(self):
        self._index = {}
        self._n = 0
        self._coords = np.zeros((0, 3), np.int32)
        self._tsdf = np.zeros((0,) + _CUBE, np.uint32)
        self._weight = np.zeros((0,) + _CUBE, np.uint32)
        self._colour = np.zeros((0,) + _CUBE + (4,), np.uint32) if self.colour else None
        self._valid = np.zeros((0, VALID_BYTES), np.uint8)
        self.last = {"bricks_out": 0, "voxels_out": 0, "bricks_in": 0, "voxels_in": 0}

    # ---- the lattice ---------------------------------------------------------------------------------------------------
    def lattice_origin(self, array_offset, fix=True):
        """g = array_offset - origin as three Python ints (gx, gy, gz); the first call with fix=True sets origin.
        ValueError when g is not whole on every axis, exactly."""
        off = np.asarray(array_offset, dtype=np.float64).reshape(-1)
        if off.size != 3 or not np.all(np.isfinite(off)):
            raise ValueError("array_offset must be three finite numbers, got %r" % (array_offset,))
        if self.origin is None:
            if fix:
                self.origin = off.copy()
            return (0, 0, 0)
        return origin_of(off - self.origin)

    # ---- what is stored ------------------------------------------------------------------------------------------------
    def __len__(self):
        return self._n

    def coords(self):
        """int32 [K][3], rows (bx, by, bz), sorted ascending by (z, y, x)"""
        c = self._coords[:self._n]
        return c[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))].copy()

    @property
    def voxel_count(self):
        """the number of valid voxels"""
        return int(np.unpackbits(self._valid[:self._n]).sum())

    @property
    def nbytes(self):
        """the bytes the stored bricks take (not the spare capacity behind them)"""
        per = 12 + VALID_BYTES + BRICK ** 3 * (8 + (16 if self.colour else 0))
        return self._n * per

    def bounds(self):
        """(lo, hi): the lattice box [lo, hi) of the stored bricks in voxels, (x, y, z) each, or None when empty"""
        if self._n == 0:
            return None
        c = self._coords[:self._n].astype(np.int64)
        return tuple(int(v) for v in c.min(axis=0) * BRICK), tuple(int(v) for v in (c.max(axis=0) + 1) * BRICK)

    def _rows(self, coords, create):
        """the row of every coordinate of int [K][3]; -1 where it is not stored, unless create appends an empty brick"""
        keys = [tuple(c) for c in np.asarray(coords, dtype=np.int64).reshape(-1, 3).tolist()]
        rows = np.array([self._index.get(k, -1) for k in keys], dtype=np.int64).reshape(len(keys))
        if create and np.any(rows < 0):
            new = [k for k in dict.fromkeys(keys) if k not in self._index]
            self._reserve(self._n + len(new))
            at = np.arange(self._n, self._n + len(new))
            self._coords[at] = np.array(new, dtype=np.int32).reshape(-1, 3)
            self._tsdf[at], self._weight[at], self._valid[at] = TSDF_EMPTY, 0, 0
            if self.colour:
                self._colour[at] = 0
            self._index.update(zip(new, at.tolist()))
            self._n += len(new)
            rows = np.array([self._index[k] for k in keys], dtype=np.int64)
        return rows

    def _reserve(self, n):
        cap = len(self._coords)
        if n <= cap:
            return
        cap = max(n, 2 * cap, 16)
        grow = lambda a: np.concatenate([a, np.zeros((cap - len(a),) + a.shape[1:], a.dtype)])
        self._coords, self._tsdf, self._weight, self._valid = (grow(a) for a in (self._coords, self._tsdf,
                                                                               self._weight, self._valid))
        if self.colour:
            self._colour = grow(self._colour)

    def merge(self, coords, tsdf, weight, colour, valid):
        """take rows in lsf_volume_bricks_gather's layout (distinct coordinates): where a row's validity bit is set its
        words overwrite the store's, and the validity bits are ORed.  Returns the number of voxels taken."""
        coords = np.asarray(coords).reshape(-1, 3)
        k = len(coords)
        if (colour is not None) != self.colour:
            raise ValueError("the rows %s colour records, the store was made with colour=%r"
                             % ("carry" if colour is not None else "carry no", self.colour))
        if k == 0:
            return 0
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(k, VALID_BYTES)
        mask = unpack_valid(valid)
        rows = self._rows(coords, create=True)
        self._tsdf[rows] = np.where(mask, _words(tsdf, (k,) + _CUBE), self._tsdf[rows])
        self._weight[rows] = np.where(mask, _words(weight, (k,) + _CUBE), self._weight[rows])
        if self.colour:
            self._colour[rows] = np.where(mask[..., None], _words(colour, (k,) + _CUBE + (4,)), self._colour[rows])
        self._valid[rows] |= valid
        return int(mask.sum())

    def lookup(self, coords):
        """the stored ones among int [K][3] coordinates, as copies in gather's layout:
        (coords int32 [M][3], tsdf, weight float32 [M][8][8][8], colour float32 [M][8][8][8][4] or None, valid uint8
        [M][64]), in the order given"""
        coords = np.asarray(coords, dtype=np.int32).reshape(-1, 3)
        rows = self._rows(coords, create=False)
        found = rows >= 0
        rows = rows[found]
        return (coords[found].copy(), self._tsdf[rows].view(np.float32), self._weight[rows].view(np.float32),
                self._colour[rows].view(np.float32) if self.colour else None, self._valid[rows])

    def lookup_entering(self, first, flags):
        """lookup of the stored bricks inside a window's grid -- first = its first brick (bx, by, bz), flags = a bool
        per brick of the grid and axis, (fx, fy, fz) -- that have the flag of any of their coordinates set
        (device_volume_bricks.entering_flags): one pass over the store's coordinates, no search per brick"""
        c = self._coords[:self._n].astype(np.int64) - np.asarray(first, dtype=np.int64)
        rows = np.nonzero(np.all((c >= 0) & (c < [len(f) for f in flags]), axis=1))[0]
        c = c[rows]
        rows = rows[flags[0][c[:, 0]] | flags[1][c[:, 1]] | flags[2][c[:, 2]]]
        return (self._coords[rows].copy(), self._tsdf[rows].view(np.float32), self._weight[rows].view(np.float32),
                self._colour[rows].view(np.float32) if self.colour else None, self._valid[rows])

    def clear_valid(self, coords, mask):
        """clear the validity bits `mask` (bool [K][8][8][8]) of the stored bricks `coords`, make those voxels the empty
        voxel, and drop every brick left without a valid bit"""
        coords = np.asarray(coords).reshape(-1, 3)
        if len(coords) == 0:
            return
        rows = self._rows(coords, create=False)
        if np.any(rows < 0):
            raise ValueError("clear_valid of a brick that is not stored")
        mask = np.asarray(mask, dtype=bool).reshape((len(coords),) + _CUBE)
        self._valid[rows] &= ~pack_valid(mask)
        gone = mask
        self._tsdf[rows] = np.where(gone, TSDF_EMPTY, self._tsdf[rows])
        self._weight[rows] = np.where(gone, np.uint32(0), self._weight[rows])
        if self.colour:
            self._colour[rows] = np.where(gone[..., None], np.uint32(0), self._colour[rows])
        keep = self._valid[:self._n].any(axis=1)
        if not keep.all():
            n = int(keep.sum())
            for name in ("_coords", "_tsdf", "_weight", "_valid") + (("_colour",) if self.colour else ()):
                a = getattr(self, name)
                a[:n] = a[:self._n][keep]
            self._n = n
            self._index = dict(zip((tuple(c) for c in self._coords[:n].tolist()), range(n)))

    def to_volume(self, lo, hi):
        """dense host arrays (tsdf, weight[, colour]) of the lattice box [lo, hi), lo and hi in voxels (x, y, z):
        float32 (Z, Y, X) and (Z, Y, X, 4), the empty voxel wherever nothing valid is stored"""
        lo = np.array(origin_of(lo), dtype=np.int64)
        hi = np.array(origin_of(hi), dtype=np.int64)
        if np.any(hi <= lo):
            raise ValueError("to_volume needs a box with lo < hi on every axis, got %r, %r" % (tuple(lo), tuple(hi)))
        shape = tuple(int(v) for v in (hi - lo)[::-1])
        tsdf = np.full(shape, TSDF_EMPTY, np.uint32)
        weight = np.zeros(shape, np.uint32)
        colour = np.zeros(shape + (4,), np.uint32) if self.colour else None
        c = self._coords[:self._n].astype(np.int64)
        near = np.all((c + 1) * BRICK > lo, axis=1) & np.all(c * BRICK < hi, axis=1)
        rows = np.nonzero(near)[0]
        if len(rows):
            place = np.arange(BRICK)
            at = [c[rows, j, None] * BRICK + place[None, :] - lo[j] for j in range(3)]  # box coordinate per brick, place
            inside = [(a >= 0) & (a < hi[j] - lo[j]) for j, a in enumerate(at)]
            take = unpack_valid(self._valid[rows]) & inside[2][:, :, None, None] & inside[1][:, None, :, None] & \
                inside[0][:, None, None, :]
            k, zl, yl, xl = np.nonzero(take)
            z, y, x = at[2][k, zl], at[1][k, yl], at[0][k, xl]
            tsdf[z, y, x] = self._tsdf[rows][k, zl, yl, xl]
            weight[z, y, x] = self._weight[rows][k, zl, yl, xl]
            if self.colour:
                colour[z, y, x] = self._colour[rows][k, zl, yl, xl]
        out = (tsdf.view(np.float32), weight.view(np.float32))
        return out + ((colour.view(np.float32),) if self.colour else ())
