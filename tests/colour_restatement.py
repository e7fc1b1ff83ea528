"""numpy restatement of colour fusion and of the mesh's vertex colours ("Colour fusion").  The
HIP kernels (lsf_fusion_integrate_depth_colour in csrc/lsf_fusion.hip, lsf_mesh_vertex_colours in csrc/lsf_mesh.hip) must
equal it: tsdf, weight and the colour volume bit for bit, the record's counts exactly (its float64 sum to 1e-12 relative,
as fusion_weighted_restatement's), the vertex colours as equal uint8.  The geometry is fusion_weighted_restatement's own
function; what a voxel sees (live value, pixel, valid flag) is restated there and in rigid3d_restatement and is used
unchanged.  The vertex order and t are mesh_restatement's.  numpy never contracts a multiply and an add, and the kernels
are built with -ffp-contract=off.  Host numpy only: no package import."""
import numpy as np

import fusion_weighted_restatement as FW
import mesh_restatement as M
import rigid3d_restatement as R3

__all__ = ["observe", "colour_update", "fuse_depth_colour", "colour_byte", "vertex_colours"]

DEFAULT_COLOUR = (128, 128, 128)


def observe(depth, K, ratio, shape, offset, twist, band=20, voxel_size=0.004):
    """(l, iy, ix, valid) per voxel: the live value and the pixel the weighted rule reads"""
    l = R3.live_volume(depth, K, ratio, shape, offset, twist, band, voxel_size)
    iy, ix, valid = FW.pixel_of_voxels(depth, K, ratio, shape, offset, twist, voxel_size)
    return l, iy, ix, valid


def colour_update(colour, l, iy, ix, valid, image, w=1.0, max_weight=np.inf, pixel_weight=None, colour_band=1.0):
    """(new colour volume, {coloured, first_coloured}) of one call.  colour: (..., 4) float32 (R, G, B, Wc); l, iy, ix,
    valid: per voxel, of colour's leading shape; image: uint8 (H, W, 3).  The input is not changed"""
    C = np.array(colour, dtype=np.float32, copy=True)
    l = np.asarray(l, dtype=np.float32)
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and C.shape == l.shape + (4,)
    w32, cap, cb = np.float32(w), np.float32(max_weight), np.float32(colour_band)
    assert cb > 0 and cb <= 1
    with np.errstate(all="ignore"):
        if pixel_weight is None:
            w_eff = np.full(l.shape, w32, np.float32)
        else:
            w_eff = w32 * np.asarray(pixel_weight, dtype=np.float32)[iy, ix]  # the geometry rule's one multiply
        usable = (w_eff > 0) & np.isfinite(w_eff)
        inside = np.asarray(valid, bool) & (l > -cb) & (l < cb)  # strictly; l == 1 (carved) and NaN are outside
        update = inside & usable
        we = w_eff[update]
        c = image[iy[update], ix[update]].astype(np.float32)  # (n, 3)
        old = C[update]
        Wc = old[:, 3]
        Wc1 = Wc + we
        new = np.empty_like(old)
        for j in range(3):
            new[:, j] = (Wc * old[:, j] + we * c[:, j]) / Wc1  # the uncapped Wc1
        new[:, 3] = np.minimum(Wc1, cap)
    C[update] = new
    return C, {"coloured": int(np.count_nonzero(update)), "first_coloured": int(np.count_nonzero(Wc == 0))}


def fuse_depth_colour(tsdf, weight, colour, depth, image, K, ratio, offset, twist, band=20, voxel_size=0.004, w=1.0,
                      max_weight=np.inf, pixel_weight=None, carve=False, colour_band=1.0, seen=None):
    """(new tsdf, new weight, new colour, record) of one colour call; the inputs are not changed.  seen: observe() of
    the same frame, volume and twist when the caller has it already"""
    shape = np.shape(tsdf)
    t, W, record = FW.fuse_depth_weighted(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, w, max_weight,
                                          pixel_weight, carve)
    l, iy, ix, valid = observe(depth, K, ratio, shape, offset, twist, band, voxel_size) if seen is None else seen
    C, counts = colour_update(colour, l, iy, ix, valid, image, w, max_weight, pixel_weight, colour_band)
    record = dict(record)
    record.update(counts)
    return t, W, C, record


def colour_byte(x):
    """floor(min(max(x, 0), 255) + 0.5) as uint8; 0 for a NaN"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y = np.floor(np.minimum(np.maximum(x, 0.0), 255.0) + 0.5)
    return np.where(np.isnan(x), 0.0, y).astype(np.uint8)


def _edge_mask(tsdf, weight, iso, min_weight):
    """mesh_restatement.extract's vertex mask: (Z, Y, X, 3) bool, a vertex on the grid edge (voxel, axis)"""
    nz, ny, nx = tsdf.shape
    usable = M._usable(tsdf, weight, min_weight)
    with np.errstate(invalid="ignore"):
        inside = tsdf.astype(np.float64) < iso
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        x, y, z = M.G.CORNERS[c]
        sl = (slice(z, nz - 1 + z), slice(y, ny - 1 + y), slice(x, nx - 1 + x))
        valid &= usable[sl]
        case |= inside[sl].astype(np.int64) << c
    code = np.where(valid, case, 0)
    mask = np.zeros((nz, ny, nx, 3), bool)
    for e in range(12):
        x, y, z = M.EDGE_OFFSET[e]
        lo, hi = M.G.EDGE_LOW[e], M.G.EDGE_HIGH[e]
        mask[z:nz - 1 + z, y:ny - 1 + y, x:nx - 1 + x, M.EDGE_AXIS[e]] |= ((code >> lo) ^ (code >> hi)) & 1 == 1
    return mask


def vertex_colours(tsdf, weight, colour, iso=0.0, min_weight=0.0, default_colour=DEFAULT_COLOUR):
    """uint8 (V, 3): row i the colour of vertex i of mesh_restatement.extract(tsdf, weight, ...)"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.float32)
    colour = np.asarray(colour, dtype=np.float32)
    assert colour.shape == tsdf.shape + (4,)
    iso = float(iso)
    i, j, k, axis = np.nonzero(_edge_mask(tsdf, weight, iso, min_weight))  # (voxel linear index, axis) order
    i1, j1, k1 = i + (axis == 2), j + (axis == 1), k + (axis == 0)
    t64 = tsdf.astype(np.float64)
    a, b = t64[i, j, k], t64[i1, j1, k1]
    t = (iso - a) / (b - a)
    ca, cb = colour[i, j, k].astype(np.float64), colour[i1, j1, k1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        has_a, has_b = colour[i, j, k, 3] > 0, colour[i1, j1, k1, 3] > 0  # NaN weights fail
    out = np.empty((i.size, 3), np.uint8)
    for ch in range(3):
        with np.errstate(invalid="ignore"):
            both = ca[:, ch] * (1.0 - t) + cb[:, ch] * t
        out[:, ch] = np.where(has_a & has_b, colour_byte(both),
                              np.where(has_a, colour_byte(ca[:, ch]),
                                       np.where(has_b, colour_byte(cb[:, ch]), np.uint8(default_colour[ch]))))
    return out
