"""numpy restatement of the fusion rule ("Fusion"): the model update of
levelsetfusion_python_amd.fusion, which the reference does not have.  The HIP kernel (csrc/lsf_fusion.hip) must equal it
bit for bit in tsdf and weight and exactly in the record's counts and maximum; the record's float64 sum is compared to
1e-12 relative, since the device reduces in a tree.  Depth mode generates the live volume with the rigid 3-D tracker's
restatement (rigid3d_restatement.live_volume).  Host numpy only: no package import."""
import numpy as np

import rigid3d_restatement as R3

__all__ = ["empty_model", "fuse", "fuse_depth", "sequence"]


def empty_model(shape):
    """(tsdf, weight): 1 and 0 everywhere, float32"""
    return np.ones(shape, np.float32), np.zeros(shape, np.float32)


def fuse(tsdf, weight, live, w=1.0, max_weight=np.inf):
    """(new tsdf, new weight, record) of one call; the inputs are not changed"""
    t = np.array(tsdf, dtype=np.float32, copy=True)
    W = np.array(weight, dtype=np.float32, copy=True)
    l = np.asarray(live, dtype=np.float32)
    w32, cap = np.float32(w), np.float32(max_weight)
    with np.errstate(invalid="ignore"):
        observed = (l > np.float32(-1)) & (l < np.float32(1))  # +-1 and NaN are not fused
    t0, W0, lo = t[observed], W[observed], l[observed]
    W1 = W0 + w32
    t1 = (W0 * t0 + w32 * lo) / W1  # the uncapped W1
    change = np.abs(t1 - t0)  # float32
    t[observed] = t1
    W[observed] = np.minimum(W1, cap)
    record = {"fused": int(np.count_nonzero(observed)), "first_seen": int(np.count_nonzero(W0 == 0)),
              "sum_abs_change": float(np.sum(change.astype(np.float64))),
              "max_abs_change": float(change.max()) if change.size else 0.0}
    return t, W, record


def fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band=20, voxel_size=0.004, w=1.0, max_weight=np.inf):
    """depth mode: the live volume of the rigid tracker under twist (float32-rounded), then fuse"""
    live = R3.live_volume(depth, K, ratio, np.shape(tsdf), offset, twist, band, voxel_size)
    return fuse(tsdf, weight, live, w, max_weight)


def sequence(frames, K, ratio, shape, offset, rigid_iterations=60, band=20, voxel_size=0.004, rate=0.5, eta=0.01,
             initial_twist=None, max_weight=np.inf):
    """SequenceFusion3d without a non-rigid step: frame 0 fused under initial_twist, every later frame tracked against
    the model from the previous twist, then fused in depth mode.  Returns (tsdf, weight, twists, fusion records)."""
    tsdf, weight = empty_model(shape)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records = [], []
    for k, depth in enumerate(frames):
        if k > 0 and rigid_iterations > 0:
            _, twist = R3.optimize(tsdf, depth, K, ratio, offset, rigid_iterations, band, eta, voxel_size, rate,
                                   twist=twist)
        tsdf, weight, rec = fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0,
                                       max_weight)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, twists, records
