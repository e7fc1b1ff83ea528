"""numpy restatement of the live depth pyramid ("Depth pyramid") and of projective ICP over
it with the normal-angle gate (lsf_icp_run_pyramid), built on tests/icp_restatement.py.  Every step below is one
float64 IEEE operation in the order written; numpy never contracts, and the kernels are built with -ffp-contract=off.
The one step the device may round differently is the filter's float64 exp (the device's and numpy's can differ in
the last bit), so level 0 is compared to 1 float32 ulp and the coarser levels and the normals are restated from the
device's own level 0.  Host numpy only: no package import."""
import math

import numpy as np

import fusion_restatement as F
import icp_restatement as I
import raycast_restatement as RC

__all__ = ["LEVELS", "RADIUS", "SIGMA_SPACE", "SIGMA_RANGE", "DEPTH_GATE", "level_intrinsics", "bilateral",
           "downsample", "normals", "pyramid", "pyramid_from_level0", "iteration", "icp", "sequence"]

LEVELS, RADIUS, SIGMA_SPACE, SIGMA_RANGE, DEPTH_GATE = 3, 3, 3.0, 0.03, 0.03


def level_intrinsics(K, levels):
    """(fx, fy, cx, cy) per level: fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2 from the level above"""
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    out = [(fx, fy, cx, cy)]
    for _ in range(1, levels):
        fx, fy, cx, cy = fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0
        out.append((fx, fy, cx, cy))
    return out


def bilateral(depth, ratio, radius=RADIUS, sigma_space=SIGMA_SPACE, sigma_range=SIGMA_RANGE):
    """level 0: the scaled depth (icp_restatement.scaled_depth) filtered over |du|, |dv| <= radius, clipped to the
    image, valid taps only, in row-major window order: w = exp(-((du du + dv dv) a + ((d_q - c) (d_q - c)) b)),
    float32(sum w d_q / sum w); 0 where the centre is not valid.  radius 0: the scaled depth as float32, 0 where not
    valid."""
    c = I.scaled_depth(depth, ratio)
    valid = c > 0.0
    if radius == 0:
        return np.where(valid, c.astype(np.float32), np.float32(0))
    a = 1.0 / (2.0 * (sigma_space * sigma_space))
    b = 1.0 / (2.0 * (sigma_range * sigma_range))
    h, w = c.shape
    r = int(radius)
    padded = np.zeros((h + 2 * r, w + 2 * r))
    padded[r:r + h, r:r + w] = np.where(valid, c, 0.0)  # NaN and <= 0 are never taps; neither is outside the image
    sw, swd = np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                d = padded[r + dv:r + dv + h, r + du:r + du + w]
                tap = d > 0.0
                e = d - c
                wt = np.exp(-(float(du * du + dv * dv) * a + (e * e) * b))
                sw = np.where(tap, sw + wt, sw)
                swd = np.where(tap, swd + wt * d, swd)
        out = (swd / sw).astype(np.float32)
    return np.where(valid, out, np.float32(0))


def downsample(d, depth_gate=DEPTH_GATE):
    """level l + 1 of level l (float32): c = d(2i, 2j); float32(sum / count) of the valid d among (2i, 2j),
    (2i, 2j + 1), (2i + 1, 2j), (2i + 1, 2j + 1), in that order, with |d - c| <= depth_gate; 0 where c is not valid"""
    d = np.asarray(d, np.float32).astype(np.float64)
    h, w = d.shape[0] >> 1, d.shape[1] >> 1
    q = [d[0:2 * h:2, 0:2 * w:2], d[0:2 * h:2, 1:2 * w:2], d[1:2 * h:2, 0:2 * w:2], d[1:2 * h:2, 1:2 * w:2]]
    c = q[0]
    s, n = np.zeros((h, w)), np.zeros((h, w))
    with np.errstate(invalid="ignore"):
        for x in q:
            m = (x > 0.0) & (np.abs(x - c) <= depth_gate)
            s = np.where(m, s + x, s)
            n = np.where(m, n + 1.0, n)
        out = (s / n).astype(np.float32)
    return np.where(c > 0.0, out, np.float32(0))


def normals(d, intrinsics, depth_gate=DEPTH_GATE):
    """(h, w, 3) float32 normals of one level: V(u, v) = d ((u - cx) / fx, (v - cy) / fy, 1), A = V(u + 1, v) - V(u, v),
    B = V(u, v + 1) - V(u, v), n = B x A / sqrt((n0 n0 + n1 n1) + n2 n2); 0 at the last row and column, where a depth of
    the three is not valid, where either depth difference exceeds depth_gate, or where the norm is not > 0"""
    fx, fy, cx, cy = intrinsics
    d = np.asarray(d, np.float32).astype(np.float64)
    h, w = d.shape
    out = np.zeros((h, w, 3), np.float32)
    if h < 2 or w < 2:
        return out
    d0, d1, d2 = d[:-1, :-1], d[:-1, 1:], d[1:, :-1]
    v, u = np.meshgrid(np.arange(h - 1, dtype=np.float64), np.arange(w - 1, dtype=np.float64), indexing="ij")
    xu, xu1 = (u - cx) / fx, ((u + 1.0) - cx) / fx
    yv, yv1 = (v - cy) / fy, ((v + 1.0) - cy) / fy
    V0 = [d0 * xu, d0 * yv, d0 * 1.0]
    V1 = [d1 * xu1, d1 * yv, d1 * 1.0]
    V2 = [d2 * xu, d2 * yv1, d2 * 1.0]
    A = [V1[c] - V0[c] for c in range(3)]
    B = [V2[c] - V0[c] for c in range(3)]
    n = [B[1] * A[2] - B[2] * A[1], B[2] * A[0] - B[0] * A[2], B[0] * A[1] - B[1] * A[0]]
    norm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    with np.errstate(invalid="ignore"):
        ok = (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0) & ~(np.abs(d1 - d0) > depth_gate) & \
            ~(np.abs(d2 - d0) > depth_gate) & (norm > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(3):
            out[:-1, :-1, c] = np.where(ok, n[c] / norm, 0.0).astype(np.float32)
    return out


def pyramid_from_level0(level0, K, levels=LEVELS, depth_gate=DEPTH_GATE):
    """(depths, normals, intrinsics), one entry per level, from a given level 0"""
    intr = level_intrinsics(K, levels)
    depths = [np.asarray(level0, np.float32)]
    for _ in range(1, levels):
        depths.append(downsample(depths[-1], depth_gate))
    return depths, [normals(d, k, depth_gate) for d, k in zip(depths, intr)], intr


def pyramid(depth, ratio, K, levels=LEVELS, radius=RADIUS, sigma_space=SIGMA_SPACE, sigma_range=SIGMA_RANGE,
            depth_gate=DEPTH_GATE):
    """the whole pyramid of a live depth image: (depths, normals, intrinsics)"""
    return pyramid_from_level0(bilateral(depth, ratio, radius, sigma_space, sigma_range), K, levels, depth_gate)


def iteration(d, n_live, intr, pred_depth, pred_normals, K, twist, twist_p, max_distance=I.MAX_DISTANCE,
              cos_max=None):
    """one iteration on one pyramid level at twist: icp_restatement.iteration over every pixel of the level (float32
    metres), its vertices from the level's intrinsics, with the gate (cos_max None: none).  Returns (record dict with
    angle_rejected, residual image of the level's extents (NaN without a correspondence), next twist)"""
    return I.iteration(np.asarray(d, np.float32), pred_depth, pred_normals, K, 1.0, twist, twist_p, 1, max_distance,
                       intr, n_live, cos_max)


def icp(levels, pred_depth, pred_normals, K, twist_p, twist=None, iterations=I.ITERATIONS,
        max_distance=I.MAX_DISTANCE, cos_max=None):
    """ICP over a pyramid (depths, normals, intrinsics), coarse first: entry k of iterations runs on level
    len(iterations) - 1 - k.  Returns (records, final twist, the last iteration's residual image or None); each record
    carries its entry index as `level`"""
    depths, norms, intr = levels
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records, residuals = [], None
    n = len(iterations)
    for k, count in enumerate(iterations):
        l = n - 1 - k
        for _ in range(count):
            rec, residuals, twist = iteration(depths[l], norms[l], intr[l], pred_depth, pred_normals, K, twist,
                                              twist_p, max_distance, cos_max)
            rec["level"] = k
            records.append(rec)
    return records, twist, residuals


def sequence(frames, K, ratio, shape, offset, iterations=I.ITERATIONS, max_distance=I.MAX_DISTANCE, cos_max=None,
             pyramid_settings=None, band=20, voxel_size=0.004):
    """SequenceFusion3d(tracking_reference="icp", icp_pyramid=...) without a non-rigid step: icp_restatement.sequence
    with each frame k >= 1 tracked over its pyramid (pyramid_settings: keyword arguments of pyramid()); fusion
    integrates the raw depth.  Returns (tsdf, weight, twists, ICP records per frame)."""
    tsdf, weight = F.empty_model(shape)
    twist = np.zeros(6)
    twists, icp_records = [], []
    for k, depth in enumerate(frames):
        recs = []
        if k > 0 and sum(iterations) > 0:
            pd, pn, _ = RC.raycast(tsdf, weight, K, twist, offset, voxel_size, np.shape(depth), normals=True)
            levels = pyramid(depth, ratio, K, **(pyramid_settings or {}))
            recs, twist, _ = icp(levels, pd, pn, K, twist, twist, iterations, max_distance, cos_max)
        icp_records.append(recs)
        tsdf, weight, _ = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0)
        twists.append(np.array(twist, dtype=np.float64))
    return tsdf, weight, twists, icp_records


def cos_of(angle):
    """the gate's cosine, as device_icp.cos_max_angle takes it"""
    return max(-1.0, min(1.0, math.cos(float(angle))))
