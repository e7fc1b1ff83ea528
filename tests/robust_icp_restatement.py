"""numpy restatement of robust ICP ("Robust ICP"): the iteratively reweighted forms of the four
ICP runs -- strided, pyramid, photometric, pyramid photometric -- on top of icp_restatement, depth_pyramid_restatement,
photometric_restatement and pyramid_photometric_restatement, and of SequenceFusion3d(tracking_reference="icp",
icp_robust=).  The HIP kernel (RobustSource in csrc/lsf_icp.hip) must equal the per-pixel arithmetic bit for bit (the
residual images, the weight image, the counts, the outliers); A, b, the energies and the weight sums are sums the device
reduces in a tree, compared with a tolerance.  Every step is one float64 IEEE operation in the order written.  Host numpy
only: no package import."""
from collections import namedtuple

import numpy as np

import depth_pyramid_restatement as DP
import fusion_restatement as F
import icp_restatement as I
import photometric_restatement as PR
import pyramid_photometric_restatement as PP
import raycast_restatement as RC

__all__ = ["Loss", "huber", "tukey", "weight", "iteration", "photometric_iteration", "pyramid_photometric_iteration",
           "icp", "pyramid_icp", "sequence"]

# kind: "huber" or "tukey"; scale: of r, metres; intensity_scale: of the unscaled r_I; np.inf leaves a term least squares
Loss = namedtuple("Loss", ["kind", "scale", "intensity_scale"], defaults=(np.inf,))


def huber(r, s):
    """w = (a <= s) ? 1 : s / a with a = |r|"""
    a = np.abs(np.asarray(r, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a <= s, 1.0, s / a)


def tukey(r, s):
    """t = r / s, u = 1 - t t, w = (a < s) ? u u : 0 with a = |r|"""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    with np.errstate(invalid="ignore", over="ignore"):
        t = r / s
        u = 1.0 - t * t
        return np.where(a < s, u * u, 0.0)


def weight(kind, r, s):
    """(w, outlier) of the residuals r at the scale s: an outlier has a > s (huber) or a >= s (tukey)"""
    with np.errstate(invalid="ignore"):
        a = np.abs(np.asarray(r, np.float64))
        if kind == "huber":
            return huber(r, s), a > s
        if kind == "tukey":
            return tukey(r, s), a >= s
    raise ValueError("kind must be 'huber' or 'tukey', got %r" % (kind,))


def _solve(loss, shape, twist, rows, cols, valid, rejected, g, Vw, Nw, photo=None):
    """the weighted normal equations over associate()'s pairs, solved and composed: per geometric pair
    wJ_i = w J_i, A_ij += wJ_i J_j, b_i -= wJ_i r, energy += (w r) r; per photometric term (photo = (has, r_I, J_I,
    lambda)) the same with w_I of the unscaled r_I on lambda J_I and lambda r_I, and (w_I r_I) r_I into its energy.
    Returns (record, residual image, intensity residual image or None, weight image, next twist)"""
    diff = [g[i] - Vw[i] for i in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2]
        J = [Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
             g[0] * Nw[1] - g[1] * Nw[0]]
        w, outlier = weight(loss.kind, r, float(loss.scale))
        wJ = [w * j for j in J]
        if photo is not None:
            has, rI, JI, lam = photo
            lam = float(lam)
            Jh = [lam * j for j in JI]
            rh = lam * rI
            wI, _ = weight(loss.kind, rI, float(loss.intensity_scale))
            wJh = [wI * j for j in Jh]
    a, a_abs = np.zeros((6, 6)), np.zeros((6, 6))
    b, b_abs = np.zeros(6), np.zeros(6)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(6):
            for j in range(i, 6):
                a[i, j] = np.sum((wJ[i] * J[j])[valid])
                a_abs[i, j] = np.sum(np.abs(wJ[i] * J[j])[valid])
                if photo is not None:
                    a[i, j] = a[i, j] + np.sum((wJh[i] * Jh[j])[has])
                    a_abs[i, j] = a_abs[i, j] + np.sum(np.abs(wJh[i] * Jh[j])[has])
                a[j, i], a_abs[j, i] = a[i, j], a_abs[i, j]
            if photo is None:
                b[i] = -np.sum((wJ[i] * r)[valid])
                b_abs[i] = np.sum(np.abs(wJ[i] * r)[valid])
            else:
                b[i] = -(np.sum((wJ[i] * r)[valid]) + np.sum((wJh[i] * rh)[has]))
                b_abs[i] = np.sum(np.abs(wJ[i] * r)[valid]) + np.sum(np.abs(wJh[i] * rh)[has])
        energy = float(np.sum(((w * r) * r)[valid]))
    residuals = np.full(shape, np.nan, np.float32)
    residuals[rows[valid], cols[valid]] = r[valid].astype(np.float32)
    weights = np.full(shape, np.nan, np.float32)
    weights[rows[valid], cols[valid]] = w[valid].astype(np.float32)
    twist = np.asarray(twist, np.float64).reshape(6)
    skipped = 1 if not np.all(np.isfinite(a)) else I._singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        twist = I.compose(twist, delta)
    rec = dict(A=a, b=b, energy=energy, count=int(valid.sum()), delta=delta, twist=twist.copy(), skipped=skipped,
               A_abs=a_abs, b_abs=b_abs, angle_rejected=int(rejected.sum()), weight_sum=float(np.sum(w[valid])),
               photometric_weight_sum=0.0, outliers=int((outlier & valid).sum()))
    intensity = None
    if photo is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            rec.update(photometric_count=int(has.sum()), photometric_energy=float(np.sum(((wI * rI) * rI)[has])),
                       photometric_weight_sum=float(np.sum(wI[has])))
        intensity = np.full(shape, np.nan, np.float32)
        intensity[rows[has], cols[has]] = rI[has].astype(np.float32)
    return rec, residuals, intensity, weights, twist


def iteration(loss, live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, stride=1,
              max_distance=I.MAX_DISTANCE, intrinsics=None, live_normals=None, cos_max=None):
    """one weighted iteration at twist over icp_restatement.associate's pairs (its arguments: a strided live image,
    or with intrinsics one pyramid level with its normals and gate): (record, residual image, weight image, next
    twist).  The record is icp_restatement.iteration's with the weights inside A, b, energy, A_abs and b_abs, and
    weight_sum, photometric_weight_sum (0) and outliers; the weight image holds float32(w) where the residual image is
    finite.  With loss.scale = inf every w is 1.0 and every product exact: icp_restatement.iteration, array for array"""
    pairs = I.associate(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, stride, max_distance,
                        intrinsics, live_normals, cos_max)
    rec, residuals, _, weights, twist = _solve(loss, np.shape(live_depth), twist, *pairs)
    return rec, residuals, weights, twist


def photometric_iteration(loss, live_depth, live_colour, pred_depth, pred_normals, pred_colour, K, ratio, twist,
                          twist_p, lam, stride=1, max_distance=I.MAX_DISTANCE, max_difference=np.inf):
    """photometric_restatement.iteration weighted: (record, residual image, intensity residual image, weight image,
    next twist); max_difference stays a hard gate in front of w_I"""
    pairs = I.associate(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p, stride, max_distance)
    rows, cols, valid, _, g = pairs[:5]
    has, rI, JI = PR.photometric_terms(live_colour, pred_colour, K, twist_p, rows, cols, valid, g, max_difference)
    return _solve(loss, np.shape(live_depth), twist, *pairs, photo=(has, rI, JI, lam))


def pyramid_photometric_iteration(loss, d, n_live, i_live, i_pred, intr, pred_depth, pred_normals, K, twist, twist_p,
                                  lam, max_distance=I.MAX_DISTANCE, cos_max=None, max_difference=np.inf):
    """pyramid_photometric_restatement.iteration weighted, on one pyramid level: photometric_iteration's five values at
    the level's extents"""
    d = np.asarray(d, np.float32)
    pairs = I.associate(d, pred_depth, pred_normals, K, 1.0, twist, twist_p, 1, max_distance, intr, n_live, cos_max)
    rows, cols, valid, _, g = pairs[:5]
    has, rI, JI = PP.photometric_terms(i_live, i_pred, intr, twist_p, rows, cols, valid, g, max_difference)
    return _solve(loss, d.shape, twist, *pairs, photo=(has, rI, JI, lam))


def icp(loss, live_depth, pred_depth, pred_normals, K, ratio, twist_p, twist=None, iterations=I.ITERATIONS,
        strides=I.STRIDES, max_distance=I.MAX_DISTANCE, live_colour=None, pred_colour=None, lam=None,
        max_difference=np.inf):
    """the whole strided schedule, coarse first, geometric or (with live_colour, pred_colour and lam) joint: (records,
    final twist, the last iteration's residual image, intensity residual image (None without the term) and weight
    image).  Each record carries its level"""
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records, residuals, intensity, weights = [], None, None, None
    for level, (n, s) in enumerate(zip(iterations, strides)):
        for _ in range(n):
            if lam is None:
                rec, residuals, weights, twist = iteration(loss, live_depth, pred_depth, pred_normals, K, ratio, twist,
                                                           twist_p, s, max_distance)
            else:
                rec, residuals, intensity, weights, twist = photometric_iteration(
                    loss, live_depth, live_colour, pred_depth, pred_normals, pred_colour, K, ratio, twist, twist_p,
                    lam, s, max_distance, max_difference)
            rec["level"] = level
            records.append(rec)
    return records, twist, residuals, intensity, weights


def pyramid_icp(loss, levels, pred_depth, pred_normals, K, twist_p, twist=None, iterations=I.ITERATIONS,
                max_distance=I.MAX_DISTANCE, cos_max=None, i_live=None, i_pred=None, lam=None, max_difference=np.inf):
    """the weighted run over a depth pyramid (depths, normals, intrinsics), coarse first, entry k of iterations on level
    len(iterations) - 1 - k; with the two intensity pyramids and lam the joint one.  Returns icp()'s five values, the
    images at the last iteration's level; each record carries its entry index as `level`"""
    depths, norms, intr = levels
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records, residuals, intensity, weights = [], None, None, None
    n = len(iterations)
    for k, count in enumerate(iterations):
        l = n - 1 - k
        for _ in range(count):
            if lam is None:
                rec, residuals, weights, twist = iteration(loss, np.asarray(depths[l], np.float32), pred_depth,
                                                           pred_normals, K, 1.0, twist, twist_p, 1, max_distance,
                                                           intr[l], norms[l], cos_max)
            else:
                rec, residuals, intensity, weights, twist = pyramid_photometric_iteration(
                    loss, depths[l], norms[l], i_live[l], i_pred[l], intr[l], pred_depth, pred_normals, K, twist,
                    twist_p, lam, max_distance, cos_max, max_difference)
            rec["level"] = k
            records.append(rec)
    return records, twist, residuals, intensity, weights


def sequence(loss, frames, K, ratio, shape, offset, iterations=I.ITERATIONS, strides=I.STRIDES,
             max_distance=I.MAX_DISTANCE, band=20, voxel_size=0.004, initial_twist=None, max_weight=np.inf):
    """SequenceFusion3d(tracking_reference="icp", icp_robust=) without a non-rigid step: icp_restatement.sequence with
    every frame k >= 1 tracked by icp() with the loss (None: icp_restatement.icp, least squares).  Returns (tsdf, weight,
    twists, fusion records, prediction hits, ICP records per frame)"""
    tsdf, weight = F.empty_model(shape)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records, hits, icp_records = [], [], [], []
    for k, depth in enumerate(frames):
        recs, h = [], None
        if k > 0 and sum(iterations) > 0:
            pd, pn, h = RC.raycast(tsdf, weight, K, twist, offset, voxel_size, np.shape(depth), normals=True)
            if loss is None:
                recs, twist = I.icp(depth, pd, pn, K, ratio, twist, twist, iterations, strides, max_distance)
            else:
                recs, twist, _, _, _ = icp(loss, depth, pd, pn, K, ratio, twist, twist, iterations, strides,
                                           max_distance)
        hits.append(h)
        icp_records.append(recs)
        tsdf, weight, rec = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0,
                                         max_weight)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, twists, records, hits, icp_records
