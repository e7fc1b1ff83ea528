"""numpy restatement of the Euclidean distance field ("Euclidean distance field"), line by line
and by brute force over the sites.  The HIP kernels (csrc/lsf_esdf.hip, lsf_esdf_compute) must equal it exactly:
distance2, nearest, the bits of esdf and the record.  Host numpy only: no package import."""
import numpy as np

INT32_MAX = 0x7fffffff
MAX_DISTANCE = 4096
UNKNOWN = ("free", "occupied")
RECORD_FIELDS = ("sites", "finite", "max_distance2")


def observed(weight, min_weight=0.0):
    """weight > min_weight in float32; a NaN weight is not observed"""
    with np.errstate(invalid="ignore"):
        return np.asarray(weight, dtype=np.float32) > np.float32(min_weight)


def inside(tsdf, weight, iso=0.0, min_weight=0.0):
    """observed and tsdf < iso in float32; a NaN tsdf is not inside"""
    with np.errstate(invalid="ignore"):
        return observed(weight, min_weight) & (np.asarray(tsdf, dtype=np.float32) < np.float32(iso))


def sites(tsdf, weight, iso=0.0, min_weight=0.0, unknown="free"):
    """(Z, Y, X) bool: an observed voxel with an in-bounds 6-neighbour that is observed and has the other inside flag --
    both sides of every zero crossing between observed voxels --, and with unknown="occupied" every voxel that is not
    observed.  A neighbour outside the volume never makes a site."""
    if unknown not in UNKNOWN:
        raise ValueError("unknown must be 'free' or 'occupied', got %r" % (unknown,))
    obs, ins = observed(weight, min_weight), inside(tsdf, weight, iso, min_weight)
    site = np.zeros(obs.shape, dtype=bool)
    for axis in range(3):
        low = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        high = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        crossing = obs[low] & obs[high] & (ins[low] != ins[high])
        site[low] |= crossing
        site[high] |= crossing
    if unknown == "occupied":
        site |= ~obs
    return site


def transform(tsdf, weight, voxel_size=0.004, max_distance_voxels=32, iso=0.0, min_weight=0.0, unknown="free", box=None):
    """(distance2 int32, nearest int32, esdf float32, record) of the (Z, Y, X) model.  key(v) = min over the sites s of
    (|v - s|^2, flat(s)), lexicographic, flat(s) = (z Y + y) X + x: the sites are visited in flat order and a later one
    replaces the key only when it is strictly nearer, so a tie stays with the smallest flat index.  A site farther than
    R = max_distance_voxels on an axis cannot give a key <= R^2, so each site visits its box of +-R only; that is the
    cap, not an approximation.  box = ((z0, z1), (y0, y1), (x0, x1)) evaluates the voxels of that box alone (the sites
    are still the whole volume's, nearest still indexes the whole volume): the outputs have the box's shape and the
    record is None."""
    tsdf, weight = np.asarray(tsdf, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    R = int(max_distance_voxels)
    if tsdf.ndim != 3 or tsdf.shape != weight.shape or not 1 <= R <= MAX_DISTANCE:
        raise ValueError("a 3-D model and 1 <= max_distance_voxels <= %d are needed" % MAX_DISTANCE)
    nz, ny, nx = tsdf.shape
    (z0, z1), (y0, y1), (x0, x1) = box if box is not None else ((0, nz), (0, ny), (0, nx))
    site = sites(tsdf, weight, iso, min_weight, unknown)
    key_d = np.full((z1 - z0, y1 - y0, x1 - x0), np.iinfo(np.int64).max, dtype=np.int64)
    key_flat = np.full(key_d.shape, -1, dtype=np.int64)
    for flat in np.flatnonzero(site):  # ascending flat order
        sz, rest = divmod(int(flat), ny * nx)
        sy, sx = divmod(rest, nx)
        za, zb = max(z0, sz - R), min(z1, sz + R + 1)
        ya, yb = max(y0, sy - R), min(y1, sy + R + 1)
        xa, xb = max(x0, sx - R), min(x1, sx + R + 1)
        if za >= zb or ya >= yb or xa >= xb:
            continue
        d = ((np.arange(za, zb, dtype=np.int64) - sz) ** 2)[:, None, None] \
            + ((np.arange(ya, yb, dtype=np.int64) - sy) ** 2)[None, :, None] \
            + ((np.arange(xa, xb, dtype=np.int64) - sx) ** 2)[None, None, :]
        part = (slice(za - z0, zb - z0), slice(ya - y0, yb - y0), slice(xa - x0, xb - x0))
        nearer = d < key_d[part]
        key_d[part] = np.where(nearer, d, key_d[part])
        key_flat[part] = np.where(nearer, flat, key_flat[part])
    kept = key_d <= R * R  # inclusive
    distance2 = np.where(kept, key_d, INT32_MAX).astype(np.int32)
    nearest = np.where(kept, key_flat, -1).astype(np.int32)
    root = np.where(kept, np.sqrt(np.where(kept, key_d, 0).astype(np.float32)), np.float32(R)).astype(np.float32)
    metres = root * np.float32(voxel_size)  # one float32 multiply
    part = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    esdf = np.where(inside(tsdf, weight, iso, min_weight)[part], -metres, metres).astype(np.float32)
    record = None
    if box is None:
        record = {"sites": int(np.count_nonzero(site)), "finite": int(np.count_nonzero(kept)),
                  "max_distance2": int(key_d[kept].max()) if kept.any() else 0}
    return distance2, nearest, esdf, record
