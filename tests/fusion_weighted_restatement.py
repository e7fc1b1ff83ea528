"""numpy restatement of the weighted fusion rule with free-space carving and of the depth confidence image
("Weighted fusion and carving" and "Depth confidence").  The HIP kernels
(lsf_fusion_integrate_depth_weighted in csrc/lsf_fusion.hip, csrc/lsf_depth_confidence.hip) must equal it bit for bit in
tsdf, weight and the confidence image and exactly in the record's counts and maximum; the record's float64 sum is
compared to 1e-12 relative, as fusion_restatement's is.  The live value is the rigid 3-D tracker's restated generation
(rigid3d_restatement.live_volume); the pixel a voxel projects to and its valid flag are restated next to it with the
same expressions.  Host numpy only: no package import."""
import numpy as np

import rigid3d_restatement as R3
from rigid_restatement import _coords, _trunc_index

__all__ = ["pixel_of_voxels", "fuse_depth_weighted", "confidence"]


def pixel_of_voxels(depth, K, ratio, shape, offset, twist, voxel_size=0.004):
    """(iy, ix, valid) per voxel of the (Z, Y, X) volume: the pixel tsdf_nearest reads under
    twist_vector_to_matrix3d(float32(twist)), and whether the generator does not return its default there -- the voxel
    in front of the camera, the pixel in the image and its scaled depth not <= 0 (NaN goes on)"""
    depth = np.asarray(depth)
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    E = R3.matrix3d(np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32))  # float64, as live_volume's
    K = np.asarray(K)
    pt = np.float32 if K.dtype == np.float32 else np.float64
    qt = np.result_type(np.float64, pt).type
    nz, ny, nx = shape
    x = np.broadcast_to(_coords(nx, offset[0], voxel_size)[None, None, :], shape).astype(np.float64)
    y = np.broadcast_to(_coords(ny, offset[1], voxel_size)[None, :, None], shape).astype(np.float64)
    z = np.broadcast_to(_coords(nz, offset[2], voxel_size)[:, None, None], shape).astype(np.float64)
    pc = [((E[k, 0] * x + E[k, 1] * y) + E[k, 2] * z) + E[k, 3] * 1.0 for k in range(3)]
    with np.errstate(all="ignore"):
        ix = _trunc_index(((qt(pt(K[0, 0])) * pc[0].astype(qt)) / pc[2].astype(qt) + qt(pt(K[0, 2]))) + qt(0.5))
        iy = _trunc_index(((qt(pt(K[1, 1])) * pc[1].astype(qt)) / pc[2].astype(qt) + qt(pt(K[1, 2]))) + qt(0.5))
        inside = (pc[2] > 0) & (ix >= 0) & (ix < depth.shape[1]) & (iy >= 0) & (iy < depth.shape[0])
        iy, ix = np.where(inside, iy, 0), np.where(inside, ix, 0)
        raw = depth[iy, ix]
        d = raw * np.float32(ratio) if depth.dtype == np.float32 else raw.astype(np.float64) * float(ratio)
        return iy, ix, inside & ~(d <= 0)


def fuse_depth_weighted(tsdf, weight, depth, K, ratio, offset, twist, band=20, voxel_size=0.004, w=1.0,
                        max_weight=np.inf, pixel_weight=None, carve=False):
    """(new tsdf, new weight, record) of one weighted depth-mode call; the inputs are not changed"""
    shape = np.shape(tsdf)
    t = np.array(tsdf, dtype=np.float32, copy=True)
    W = np.array(weight, dtype=np.float32, copy=True)
    l = R3.live_volume(depth, K, ratio, shape, offset, twist, band, voxel_size)
    iy, ix, valid = pixel_of_voxels(depth, K, ratio, shape, offset, twist, voxel_size)
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


def confidence(depth_m, normals, K, reference_depth):
    """(H, W) float32: |n . r| min(1, (reference_depth / z)^2), every step one float64 operation in the order of
    csrc/lsf_depth_confidence.hip's header, rounded once; 0 where z is not > 0 or the normal is the zero vector"""
    z = np.asarray(depth_m, dtype=np.float32).astype(np.float64)
    n = np.asarray(normals, dtype=np.float32).astype(np.float64)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    v, u = np.meshgrid(np.arange(z.shape[0], dtype=np.float64), np.arange(z.shape[1], dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        x, y = (u - cx) / fx, (v - cy) / fy
        length = np.sqrt((x * x + y * y) + 1.0)
        dot = (n[..., 0] * x + n[..., 1] * y) + n[..., 2]
        a = np.abs(dot) / length
        q = float(reference_depth) / z
        s = q * q
        m = np.where(s < 1.0, s, 1.0)
        c = (a * m).astype(np.float32)
        ok = (z > 0) & ~((n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0))
    return np.where(ok, c, np.float32(0)).astype(np.float32)
