"""numpy restatement of point-to-SDF tracking ("Point-to-SDF tracking") and of
SequenceFusion3d's "sdf" tracking mode.  The HIP kernel (csrc/lsf_point_sdf.hip) must equal the per-pixel arithmetic bit
for bit (the residual image, the weight image, the counts); A, b, the energy and the weight sum are sums, which the
device reduces in a tree, so they are compared with a tolerance.  Every step below is one float64 IEEE operation in the
order written; numpy never contracts, and the kernel is built with -ffp-contract=off.  The pose, the vertex, the world
point and the composed update are icp_restatement's, the sample is raycast_restatement's, the weights are
robust_icp_restatement's.  Host numpy only: no package import."""
import numpy as np

import fusion_restatement as F
import icp_restatement as I
import raycast_restatement as RC
import robust_icp_restatement as RR
from rigid_restatement import rodrigues

__all__ = ["ITERATIONS", "STRIDES", "MAX_DISTANCE", "sample_gradient", "iteration", "track", "sequence"]

ITERATIONS, STRIDES, MAX_DISTANCE = I.ITERATIONS, I.STRIDES, I.MAX_DISTANCE


def sample_gradient(tsdf, weight, p):
    """(valid, phi, d) of the trilinear samples at voxel coordinates p = (px, py, pz): raycast_restatement's sample, and
    the gradient of its interpolant in voxel units from the same 8 corners t0 .. t7 (x fastest)"""
    valid, phi = RC._sample(tsdf, weight, p)
    i0 = [np.floor(np.where(valid, p[j], 0.0)).astype(np.int64) for j in range(3)]
    fx, fy, fz = [np.where(valid, p[j], 0.0) - i0[j].astype(np.float64) for j in range(3)]
    hx, hy, hz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    x0, y0, z0 = i0
    t = [tsdf[z0 + dz, y0 + dy, x0 + dx].astype(np.float64) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    c00 = t[0] * hx + t[1] * fx
    c01 = t[2] * hx + t[3] * fx
    c10 = t[4] * hx + t[5] * fx
    c11 = t[6] * hx + t[7] * fx
    c0 = c00 * hy + c01 * fy
    c1 = c10 * hy + c11 * fy
    dx = ((t[1] - t[0]) * hy + (t[3] - t[2]) * fy) * hz + ((t[5] - t[4]) * hy + (t[7] - t[6]) * fy) * fz
    dy = (c01 - c00) * hz + (c11 - c10) * fz
    dz = c1 - c0
    return valid, phi, [dx, dy, dz]


def iteration(tsdf, weight, live_depth, K, ratio, twist, offset, stride=1, max_distance=MAX_DISTANCE, band=20,
              voxel_size=0.004, loss=None):
    """one iteration at twist over the live pixels (stride * i, stride * j): (record dict, residual image of live_depth's
    extents -- float32, NaN where a pixel has no pair --, weight image (None without a loss), next twist).  loss: None or
    a robust_icp_restatement.Loss, whose scale weighs r"""
    tsdf = np.asarray(tsdf, np.float32)
    weight = np.asarray(weight, np.float32)
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    off = np.asarray(offset, np.float64).reshape(3)
    vs = float(voxel_size)
    mu = float(band) * vs
    d = I.scaled_depth(live_depth, ratio)
    tw = np.asarray(twist, np.float64).reshape(6)
    R, t = rodrigues(tw[3:]), tw[:3]
    rows, cols = np.meshgrid(np.arange(0, d.shape[0], stride), np.arange(0, d.shape[1], stride), indexing="ij")
    u, v = cols.astype(np.float64), rows.astype(np.float64)
    dd = d[rows, cols]
    live = dd > 0.0
    vx = [dd * ((u - cx) / fx), dd * ((v - cy) / fy), dd * 1.0]
    g = I._rt(R, vx, t)
    p = [g[j] / vs - off[j] for j in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        valid, phi, dv = sample_gradient(tsdf, weight, p)
        r = mu * phi
        grad = [(mu * dv[j]) / vs for j in range(3)]
        pair = live & valid & (np.abs(r) <= float(max_distance)) & \
            ((grad[0] != 0.0) | (grad[1] != 0.0) | (grad[2] != 0.0))
        J = [grad[0], grad[1], grad[2], g[1] * grad[2] - g[2] * grad[1], g[2] * grad[0] - g[0] * grad[2],
             g[0] * grad[1] - g[1] * grad[0]]
        if loss is None:
            w, outlier, wJ = np.ones_like(r), np.zeros(r.shape, bool), J
        else:
            w, outlier = RR.weight(loss.kind, r, float(loss.scale))
            wJ = [w * j for j in J]
        a, a_abs = np.zeros((6, 6)), np.zeros((6, 6))
        b, b_abs = np.zeros(6), np.zeros(6)
        for i in range(6):
            for j in range(i, 6):
                a[i, j] = a[j, i] = np.sum((wJ[i] * J[j])[pair])
                a_abs[i, j] = a_abs[j, i] = np.sum(np.abs(wJ[i] * J[j])[pair])
            b[i] = -np.sum((wJ[i] * r)[pair])
            b_abs[i] = np.sum(np.abs(wJ[i] * r)[pair])
        energy = float(np.sum((r * r)[pair])) if loss is None else float(np.sum(((w * r) * r)[pair]))
    residuals = np.full(np.shape(live_depth), np.nan, np.float32)
    residuals[rows[pair], cols[pair]] = r[pair].astype(np.float32)
    weights = None
    if loss is not None:
        weights = np.full(np.shape(live_depth), np.nan, np.float32)
        weights[rows[pair], cols[pair]] = w[pair].astype(np.float32)
    skipped = 1 if not np.all(np.isfinite(a)) else I._singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        tw = I.compose(tw, delta)
    # A_abs, b_abs: the sums of the terms' magnitudes, the scale of a sum's rounding in another order
    rec = dict(A=a, b=b, energy=energy, count=int(pair.sum()), delta=delta, twist=tw.copy(), skipped=skipped,
               A_abs=a_abs, b_abs=b_abs, no_sample=int((live & ~valid).sum()),
               weight_sum=0.0 if loss is None else float(np.sum(w[pair])), outliers=int((outlier & pair).sum()))
    return rec, residuals, weights, tw


def track(tsdf, weight, live_depth, K, ratio, twist, offset, iterations=ITERATIONS, strides=STRIDES,
          max_distance=MAX_DISTANCE, band=20, voxel_size=0.004, loss=None):
    """the whole run from twist, coarse first: (records, final twist, the last iteration's residual image and weight
    image).  Each record carries its level"""
    twist = np.asarray(twist, np.float64).reshape(6).copy()
    records, residuals, weights = [], None, None
    for level, (n, s) in enumerate(zip(iterations, strides)):
        for _ in range(n):
            rec, residuals, weights, twist = iteration(tsdf, weight, live_depth, K, ratio, twist, offset, s,
                                                       max_distance, band, voxel_size, loss)
            rec["level"] = level
            records.append(rec)
    return records, twist, residuals, weights


def sequence(frames, K, ratio, shape, offset, iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE,
             band=20, voxel_size=0.004, initial_twist=None, max_weight=np.inf, loss=None):
    """SequenceFusion3d(tracking_reference="sdf") without a non-rigid step: frame 0 fused under initial_twist; frame
    k >= 1 tracked from twist_{k-1} against the model itself, then fused in depth mode.  Returns (tsdf, weight, twists,
    fusion records, tracking records per frame)."""
    tsdf, weight = F.empty_model(shape)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records, sdf_records = [], [], []
    for k, depth in enumerate(frames):
        recs = []
        if k > 0 and sum(iterations) > 0:
            recs, twist, _, _ = track(tsdf, weight, depth, K, ratio, twist, offset, iterations, strides, max_distance,
                                      band, voxel_size, loss)
        sdf_records.append(recs)
        tsdf, weight, rec = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0,
                                         max_weight)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, twists, records, sdf_records
