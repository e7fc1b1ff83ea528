"""numpy restatement of projective point-to-plane ICP against the ray-cast prediction (INTEGRATION.md section 3,
"Projective ICP") and of SequenceFusion3d's "icp" tracking mode.  The HIP kernel (csrc/lsf_icp.hip) must equal the
per-pixel arithmetic bit for bit (the residual image, the correspondence count); A, b and the energy are sums, which
the device reduces in a tree, so they are compared with a tolerance.  Every step below is one float64 IEEE operation in
the order written; numpy never contracts, and the kernel is built with -ffp-contract=off.  Host numpy only: no package
import."""
import math

import numpy as np

import fusion_restatement as F
import raycast_restatement as RC
from rigid_restatement import rodrigues

__all__ = ["ITERATIONS", "STRIDES", "MAX_DISTANCE", "scaled_depth", "log_rotation", "compose", "associate",
           "iteration", "icp", "sequence"]

ITERATIONS, STRIDES, MAX_DISTANCE = (4, 4, 6), (4, 2, 1), 0.02


def scaled_depth(depth, ratio):
    """the live depth in metres as float64, scaled as the generators scale it: uint16 and float64 in float64, float32
    in float32"""
    d = np.asarray(depth)
    if d.dtype == np.float32:
        return (d * np.float32(ratio)).astype(np.float64)
    if d.dtype in (np.uint16, np.float64):
        return d.astype(np.float64) * float(ratio)
    raise ValueError("live depth must be uint16, float32 or float64")


def log_rotation(R):
    """the rotation vector of R: theta = atan2(|w|, (tr R - 1) / 2), w = vee(R - R^T) / 2, r = w (theta / |w|), 0 when
    |w| = 0.  Accurate away from theta = pi only"""
    w = np.array([(R[2, 1] - R[1, 2]) / 2.0, (R[0, 2] - R[2, 0]) / 2.0, (R[1, 0] - R[0, 1]) / 2.0])
    nw = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if nw == 0.0:
        return np.zeros(3)
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    theta = math.atan2(nw, (tr - 1.0) / 2.0)
    return w * (theta / nw)


def _mat_mat_t(A, B):
    """A B^T, each entry ((A[i,0] B[j,0] + A[i,1] B[j,1]) + A[i,2] B[j,2])"""
    out = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            out[i, j] = (A[i, 0] * B[j, 0] + A[i, 1] * B[j, 1]) + A[i, 2] * B[j, 2]
    return out


def compose(twist, delta):
    """the twist after a step delta = (tau, omega) of the left perturbation g <- g + omega x g + tau:
    R' = R Rodrigues(omega)^T, t' = t - R' tau, twist' = (t', log R')"""
    twist = np.asarray(twist, np.float64).reshape(6)
    R = rodrigues(twist[3:])
    Rn = _mat_mat_t(R, rodrigues(np.asarray(delta[3:], np.float64)))
    t = np.array([twist[i] - ((Rn[i, 0] * delta[0] + Rn[i, 1] * delta[1]) + Rn[i, 2] * delta[2]) for i in range(3)])
    return np.concatenate([t, log_rotation(Rn)])


def _rt(R, x, t=None):
    """R^T (x - t) per pixel, x a list of three arrays: ((R[0,j] x0 + R[1,j] x1) + R[2,j] x2)"""
    if t is not None:
        x = [x[i] - t[i] for i in range(3)]
    return [(R[0, j] * x[0] + R[1, j] * x[1]) + R[2, j] * x[2] for j in range(3)]


def associate(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, stride=1, max_distance=MAX_DISTANCE,
              intrinsics=None, live_normals=None, cos_max=None):
    """the correspondences of the live pixels (stride * i, stride * j) at twist: (rows, cols, valid, rejected, g, V_w,
    N_w) with g, V_w, N_w lists of three float64 arrays over the strided pixels.  intrinsics: the (fx, fy, cx, cy) the
    live vertices are made with, K's by default; another set makes live_depth one level of a pyramid, which need not
    have the prediction's extents.  cos_max (None: no gate): a pair within max_distance whose live normal
    (live_normals, (h, w, 3)) is zero or has (R^T n) . N_w < cos_max is `rejected`, not valid"""
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    lfx, lfy, lcx, lcy = (fx, fy, cx, cy) if intrinsics is None else intrinsics
    d = scaled_depth(live_depth, ratio)
    pd = np.asarray(pred_depth, np.float32)
    pn = np.asarray(pred_normals, np.float32)
    h, w = pd.shape
    if (intrinsics is None and d.shape != (h, w)) or pn.shape != (h, w, 3):
        raise ValueError("the prediction must be depth of the live extents %s and normals (h, w, 3), got %s and %s"
                         % (d.shape, pd.shape, pn.shape))
    tw = np.asarray(twist, np.float64).reshape(6)
    R, t = rodrigues(tw[3:]), tw[:3]
    Ep = RC.extrinsic(twist_p)
    Rp, tp = Ep[:, :3], Ep[:, 3]
    rows, cols = np.meshgrid(np.arange(0, d.shape[0], stride), np.arange(0, d.shape[1], stride), indexing="ij")
    u, v = cols.astype(np.float64), rows.astype(np.float64)
    dd = d[rows, cols]
    live = dd > 0.0
    vx = [dd * ((u - lcx) / lfx), dd * ((v - lcy) / lfy), dd * 1.0]
    g = _rt(R, vx, t)
    q = [((Rp[i, 0] * g[0] + Rp[i, 1] * g[1]) + Rp[i, 2] * g[2]) + tp[i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ph = np.rint((fx * q[0]) / q[2] + cx)
        pv = np.rint((fy * q[1]) / q[2] + cy)
        valid = live & (q[2] > 0.0) & (ph >= 0.0) & (ph <= float(w - 1)) & (pv >= 0.0) & (pv <= float(h - 1))
    iu = np.where(valid, ph, 0.0).astype(np.int64)
    iv = np.where(valid, pv, 0.0).astype(np.int64)
    D = pd[iv, iu].astype(np.float64)
    Nc = [pn[iv, iu, i].astype(np.float64) for i in range(3)]
    valid &= (D > 0.0) & ((Nc[0] != 0.0) | (Nc[1] != 0.0) | (Nc[2] != 0.0))
    V = [D * ((iu.astype(np.float64) - cx) / fx), D * ((iv.astype(np.float64) - cy) / fy), D * 1.0]
    Vw = _rt(Rp, V, tp)
    Nw = _rt(Rp, Nc)
    diff = [g[i] - Vw[i] for i in range(3)]
    with np.errstate(invalid="ignore"):
        dist = np.sqrt((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2])
        valid &= dist <= float(max_distance)
    rejected = np.zeros_like(valid)
    if cos_max is not None:
        ln = [np.asarray(live_normals, np.float32)[rows, cols, i].astype(np.float64) for i in range(3)]
        m = _rt(R, ln)
        with np.errstate(invalid="ignore"):
            keep = ((ln[0] != 0.0) | (ln[1] != 0.0) | (ln[2] != 0.0)) & \
                (((m[0] * Nw[0] + m[1] * Nw[1]) + m[2] * Nw[2]) >= cos_max)
        rejected = valid & ~keep
        valid &= keep
    return rows, cols, valid, rejected, g, Vw, Nw


def iteration(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, stride=1, max_distance=MAX_DISTANCE,
              intrinsics=None, live_normals=None, cos_max=None):
    """one iteration at twist over associate()'s pairs: (record dict, residual image of live_depth's extents, float32,
    NaN where a pixel has no correspondence, next twist)"""
    rows, cols, valid, rejected, g, Vw, Nw = associate(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p,
                                                       stride, max_distance, intrinsics, live_normals, cos_max)
    diff = [g[i] - Vw[i] for i in range(3)]
    with np.errstate(invalid="ignore"):
        r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2]
        J = [Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
             g[0] * Nw[1] - g[1] * Nw[0]]
    a, a_abs = np.zeros((6, 6)), np.zeros((6, 6))
    b, b_abs = np.zeros(6), np.zeros(6)
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = np.sum((J[i] * J[j])[valid])
            a_abs[i, j] = a_abs[j, i] = np.sum(np.abs(J[i] * J[j])[valid])
        b[i] = -np.sum((J[i] * r)[valid])
        b_abs[i] = np.sum(np.abs(J[i] * r)[valid])
    energy = float(np.sum((r * r)[valid]))
    residuals = np.full(np.shape(live_depth), np.nan, np.float32)
    residuals[rows[valid], cols[valid]] = r[valid].astype(np.float32)
    twist = np.asarray(twist, np.float64).reshape(6)
    skipped = 1 if not np.all(np.isfinite(a)) else _singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        twist = compose(twist, delta)
    # A_abs, b_abs: the sums of the terms' magnitudes, the scale of a sum's rounding in another order
    rec = dict(A=a, b=b, energy=energy, count=int(valid.sum()), delta=delta, twist=twist.copy(), skipped=skipped,
               A_abs=a_abs, b_abs=b_abs, angle_rejected=int(rejected.sum()))
    return rec, residuals, twist


def _singular(a):
    """the rigid trackers' rule: 1 on an exact zero pivot of LU with partial pivoting"""
    m = np.array(a, np.float64)
    for c in range(6):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if m[p, c] == 0.0:
            return 1
        m[[c, p]] = m[[p, c]]
        for r in range(c + 1, 6):
            m[r, c + 1:] = m[r, c + 1:] - (m[r, c] / m[c, c]) * m[c, c + 1:]
    return 0


def icp(live_depth, pred_depth, pred_normals, K, ratio, twist_p, twist=None, iterations=ITERATIONS, strides=STRIDES,
        max_distance=MAX_DISTANCE):
    """the whole pyramid, coarse first: (records, final twist).  Each record carries its level"""
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records = []
    for level, (n, s) in enumerate(zip(iterations, strides)):
        for _ in range(n):
            rec, _, twist = iteration(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, s, max_distance)
            rec["level"] = level
            records.append(rec)
    return records, twist


def sequence(frames, K, ratio, shape, offset, iterations=ITERATIONS, strides=STRIDES, max_distance=MAX_DISTANCE,
             band=20, voxel_size=0.004, initial_twist=None, max_weight=np.inf):
    """SequenceFusion3d(tracking_reference="icp") without a non-rigid step: frame 0 fused under initial_twist; frame
    k >= 1 tracked by ICP from twist_{k-1} against the model ray-cast with normals at twist_{k-1} (no fallback), then
    fused in depth mode.  Returns (tsdf, weight, twists, fusion records, prediction hits, ICP records per frame)."""
    tsdf, weight = F.empty_model(shape)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records, hits, icp_records = [], [], [], []
    for k, depth in enumerate(frames):
        recs, h = [], None
        if k > 0 and sum(iterations) > 0:
            pd, pn, h = RC.raycast(tsdf, weight, K, twist, offset, voxel_size, np.shape(depth), normals=True)
            recs, twist = icp(depth, pd, pn, K, ratio, twist, twist, iterations, strides, max_distance)
        hits.append(h)
        icp_records.append(recs)
        tsdf, weight, rec = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0,
                                         max_weight)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, twists, records, hits, icp_records
