"""numpy restatement of warped depth fusion ("Warped depth fusion"): the weighted rule with
carving and the colour rule, with every voxel observing the frame at its point displaced by a warp field psi.  The HIP
kernel (lsf_fusion_integrate_depth_warped in csrc/lsf_fusion.hip) must equal it: tsdf, weight and the colour volume bit for
bit, the record's counts and maximum exactly, its float64 sum to 1e-12 relative, as fusion_weighted_restatement's.
What a point sees is rigid_restatement.tsdf_nearest's and fusion_weighted_restatement.pixel_of_voxels' expressions with the
per-voxel warped point in place of _coords -- float64 add and multiply, a float32 point, a float64 extrinsic product, the
projection in the promoted intrinsics' dtype; the update is fusion_weighted_restatement.fuse_depth_weighted's, and the
colour is colour_restatement.colour_update itself.  tests/test_warped_fusion_host.py holds the restatement to those two
at psi = 0 and at integer shifts.  Host numpy only: no package import."""
import numpy as np

import colour_restatement as C
import rigid3d_restatement as R3
from rigid_restatement import _trunc_index

__all__ = ["warped_points", "observe_points", "fuse_depth_warped", "WARPED_RECORD_FIELDS"]

WARPED_RECORD_FIELDS = ("fused", "first_seen", "sum_abs_change", "max_abs_change", "carved", "weight_rejected",
                        "coloured", "first_coloured", "warp_rejected")


def warped_points(shape, offset, warp, voxel_size=0.004):
    """(x, y, z, finite): the float32 point of every voxel of the (Z, Y, X) volume displaced by warp (Z, Y, X, 3; x, y,
    z channels, voxels), float32(((float64 index + float64 psi) + offset) * voxel_size) per axis, and whether all three
    components of its psi are finite"""
    warp = np.asarray(warp)
    assert warp.dtype == np.float32 and warp.shape == tuple(shape) + (3,)
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    index = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")  # z, y, x
    with np.errstate(all="ignore"):
        x, y, z = ((((index[2 - c] + warp[..., c].astype(np.float64)) + float(offset[c])) * voxel_size).astype(np.float32)
                   for c in range(3))
    return x, y, z, np.all(np.isfinite(warp), axis=-1)


def observe_points(depth, K, ratio, x, y, z, twist, band=20, voxel_size=0.004):
    """(l, iy, ix, valid) of the float32 points (x, y, z): the live value tsdf_nearest gives a voxel with that point
    under twist_vector_to_matrix3d(float32(twist)) (default 1), the pixel it reads and whether the generator does not
    return its default there"""
    depth = np.asarray(depth)
    E = R3.matrix3d(np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32))  # float64
    K = np.asarray(K)
    pt = np.float32 if K.dtype == np.float32 else np.float64
    qt = np.result_type(np.float64, pt).type
    half = band / 2 * voxel_size
    x, y, z = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (x, y, z))
    with np.errstate(all="ignore"):
        pc = [((E[k, 0] * x + E[k, 1] * y) + E[k, 2] * z) + E[k, 3] * 1.0 for k in range(3)]
        ix = _trunc_index(((qt(pt(K[0, 0])) * pc[0].astype(qt)) / pc[2].astype(qt) + qt(pt(K[0, 2]))) + qt(0.5))
        iy = _trunc_index(((qt(pt(K[1, 1])) * pc[1].astype(qt)) / pc[2].astype(qt) + qt(pt(K[1, 2]))) + qt(0.5))
        inside = (pc[2] > 0) & (ix >= 0) & (ix < depth.shape[1]) & (iy >= 0) & (iy < depth.shape[0])
        iy, ix = np.where(inside, iy, 0), np.where(inside, ix, 0)
        raw = depth[iy, ix]
        d = raw * np.float32(ratio) if depth.dtype == np.float32 else raw.astype(np.float64) * float(ratio)
        st = np.result_type(d.dtype, np.float64).type
        sd = d.astype(st) - pc[2].astype(st)
        hs = st(half)
        val = np.where(sd < -hs, st(-1), np.where(sd > hs, st(1), sd / hs)).astype(np.float32)
        valid = inside & ~(d <= 0)
        return np.where(valid, val, np.float32(1)).astype(np.float32), iy, ix, valid


def _weighted_update(tsdf, weight, l, iy, ix, valid, w, max_weight, pixel_weight, carve):
    """fusion_weighted_restatement.fuse_depth_weighted from its live values and pixels on"""
    shape = np.shape(tsdf)
    t = np.array(tsdf, dtype=np.float32, copy=True)
    W = np.array(weight, dtype=np.float32, copy=True)
    w32, cap = np.float32(w), np.float32(max_weight)
    with np.errstate(all="ignore"):
        band_ = valid & (l > np.float32(-1)) & (l < np.float32(1))
        carved = valid & (l == np.float32(1)) if carve else np.zeros(shape, bool)
        seen = band_ | carved
        if pixel_weight is None:
            w_eff = np.full(shape, w32, np.float32)
        else:
            w_eff = w32 * np.asarray(pixel_weight, dtype=np.float32)[iy, ix]  # one float32 multiply
        usable = (w_eff > 0) & np.isfinite(w_eff)
        update = seen & usable
        t0, W0, lo, we = t[update], W[update], l[update], w_eff[update]
        W1 = W0 + we
        t1 = (W0 * t0 + we * lo) / W1  # the uncapped W1
        change = np.abs(t1 - t0)  # float32
    t[update] = t1
    W[update] = np.minimum(W1, cap)
    record = {"fused": int(np.count_nonzero(band_ & usable)), "first_seen": int(np.count_nonzero(W0 == 0)),
              "sum_abs_change": float(np.sum(change.astype(np.float64))),
              "max_abs_change": float(change.max()) if change.size else 0.0,
              "carved": int(np.count_nonzero(carved & usable)),
              "weight_rejected": int(np.count_nonzero(seen & ~usable))}
    return t, W, record


def fuse_depth_warped(tsdf, weight, depth, K, ratio, offset, twist, warp, band=20, voxel_size=0.004, w=1.0,
                      max_weight=np.inf, pixel_weight=None, carve=False, colour=None, colour_image=None,
                      colour_band=1.0):
    """(new tsdf, new weight, new colour or None, record) of one warped call; the inputs are not changed.  colour and
    colour_image are given together or not at all; without them coloured and first_coloured are 0"""
    assert (colour is None) == (colour_image is None)
    shape = np.shape(tsdf)
    x, y, z, finite = warped_points(shape, offset, warp, voxel_size)
    l, iy, ix, valid = observe_points(depth, K, ratio, x, y, z, twist, band, voxel_size)
    valid = valid & finite  # a voxel whose psi is not finite sees nothing
    t, W, record = _weighted_update(tsdf, weight, l, iy, ix, valid, w, max_weight, pixel_weight, carve)
    counts = {"coloured": 0, "first_coloured": 0}
    new_colour = None
    if colour is not None:
        new_colour, counts = C.colour_update(colour, l, iy, ix, valid, colour_image, w, max_weight, pixel_weight,
                                             colour_band)
    record.update(counts)
    record["warp_rejected"] = int(np.count_nonzero(~finite))
    return t, W, new_colour, record
