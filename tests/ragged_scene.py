"""Closed-form (canonical, live) TSDF pairs on ragged and non-cubic arrays: an ellipsoid (an ellipse in 2-D) and the same
body shifted and anisotropically scaled, truncated to [-1, 1].  No extent has to be a cube's, a multiple of the box edge (4),
of a tile or of the 1024-voxel chunk of the prepare pass; the scenes below are the ones tests/test_gpu_ragged_volumes.py
drives the KillingFusion engine with, and tests/test_ragged_scene_host.py holds the properties it relies on against the
oracle.  numpy only: importable without a GPU."""
import numpy as np

SHIFT = (0.75, -0.5, 1.0)
SCALE = (1.05, 0.95, 1.0)


def pair(shape, semi, h=4.0, shift=SHIFT, scale=SCALE, centre=None):
    """(canonical, live), float32, of `shape` (array order: [z,] y, x).  semi, shift, scale, centre: (x, y[, z]).
    field = clip((sqrt(sum(((q_i - (c_i + shift_i)) / (semi_i * scale_i))^2)) - 1) * min(semi) / h, -1, 1); the canonical
    field has zero shift and unit scale.  The default centre, (extent - 1) / 2 + 0.3 per axis, lies off every symmetry
    plane of the voxel grid: with the anisotropic scale it keeps the longest update from tying between voxels."""
    shape = tuple(int(s) for s in shape)
    d = len(shape)
    if d not in (2, 3):
        raise ValueError("2-D or 3-D shapes, got %r" % (shape,))
    semi = tuple(float(s) for s in semi)
    if len(semi) != d:
        raise ValueError("semi must hold one semi-axis per dimension (x, y[, z])")
    extents = shape[::-1]  # (x, y[, z])
    if centre is None:
        centre = tuple((n - 1) / 2.0 + 0.3 for n in extents)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    coords = grids[::-1]  # (x, y[, z])

    def tsdf(shift_, scale_):
        sq = 0.0
        for i in range(d):
            sq = sq + ((coords[i] - (centre[i] + shift_[i])) / (semi[i] * scale_[i])) ** 2
        return np.clip((np.sqrt(sq) - 1.0) * min(semi) / h, -1.0, 1.0).astype(np.float32)

    return tsdf((0.0,) * d, (1.0,) * d), tsdf(tuple(shift)[:d], tuple(scale)[:d])


# name -> (shape in array order, keyword arguments of pair())
SCENES = {
    "odd": ((21, 30, 37), dict(semi=(22.0, 9.0, 6.5))),      # no extent a multiple of 4, nx odd, 22.76 chunks
    "fours": ((20, 28, 36), dict(semi=(11.0, 16.0, 6.0))),   # every extent a multiple of 4, none of 8, all different
    "tiny": ((5, 7, 9), dict(semi=(3.0, 2.5, 4.0))),         # less than one chunk, all of it in the band
    "far": ((61, 50, 45), dict(semi=(7.0, 8.0, 9.0), centre=(14.3, 15.2, 16.1))),  # a slice is 2.2 chunks; small updates
    "flat": ((33, 70), dict(semi=(25.0, 40.0))),             # 2-D
}


def scene(name):
    shape, kw = SCENES[name]
    return pair(shape, **kw)
