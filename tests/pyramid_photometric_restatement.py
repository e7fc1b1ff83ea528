"""numpy restatement of the intensity pyramids ("Intensity pyramid") and of the joint geometric
and photometric ICP over the depth pyramid ("Photometric ICP", the level rule), on top of icp_restatement,
depth_pyramid_restatement and photometric_restatement, and of SequenceFusion3d(colour=True, tracking_reference="icp",
icp_pyramid=, icp_intensity_pyramid=, photometric_weight=).  The HIP kernels (csrc/lsf_intensity_pyramid.hip,
lsf_icp_run_pyramid_photometric in csrc/lsf_icp.hip) must equal the per-pixel arithmetic bit for bit (every pyramid
level, both residual images, the three counts); A, b and the energies are sums, compared with a tolerance.  Every step is
one float64 IEEE operation in the order written.  Host numpy only: no package import."""
import numpy as np

import colour_restatement as C
import depth_pyramid_restatement as DP
import fusion_restatement as F
import icp_restatement as I
import photometric_restatement as PR

__all__ = ["live_level0", "prediction_level0", "downsample", "pyramid_from_level0", "live_pyramid",
           "prediction_pyramid", "photometric_terms", "iteration", "icp", "sequence"]


def live_level0(colour_image):
    """float32(((0.299 R + 0.587 G) + 0.114 B) / 255) of a uint8 (H, W, 3) image: photometric ICP's I_l, rounded"""
    c = np.asarray(colour_image)
    if c.dtype != np.uint8 or c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("a colour image is uint8 (H, W, 3)")
    c = c.astype(np.float64)
    return (((0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]) / 255.0).astype(np.float32)


def prediction_level0(pred_colour):
    """channel 3 of the ray-cast colour image (H, W, 4) float32, copied bit for bit, NaNs included"""
    pc = np.asarray(pred_colour)
    if pc.dtype != np.float32 or pc.ndim != 3 or pc.shape[2] != 4:
        raise ValueError("a prediction colour image is float32 (H, W, 4)")
    return pc[..., 3].view(np.uint32).copy().view(np.float32)


def downsample(level):
    """level l + 1 of level l (float32), extents (h >> 1, w >> 1): float32(((q00 + q10) + (q01 + q11)) / 4) of the
    2 x 2 block q00, q10 (one row), q01, q11 (the next) as doubles, NaN when one of the four is not finite"""
    d = np.asarray(level, np.float32).astype(np.float64)
    h, w = d.shape[0] >> 1, d.shape[1] >> 1
    q00, q10 = d[0:2 * h:2, 0:2 * w:2], d[0:2 * h:2, 1:2 * w:2]
    q01, q11 = d[1:2 * h:2, 0:2 * w:2], d[1:2 * h:2, 1:2 * w:2]
    ok = np.isfinite(q00) & np.isfinite(q10) & np.isfinite(q01) & np.isfinite(q11)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (((q00 + q10) + (q01 + q11)) / 4.0).astype(np.float32)
    return np.where(ok, out, np.float32(np.nan))


def pyramid_from_level0(level0, levels=DP.LEVELS):
    """the levels of an intensity pyramid, level 0 first"""
    out = [np.asarray(level0, np.float32)]
    if (out[0].shape[0] >> (levels - 1)) < 1 or (out[0].shape[1] >> (levels - 1)) < 1:
        raise ValueError("a %d x %d image has no %d-level pyramid" % (out[0].shape + (levels,)))
    for _ in range(1, levels):
        out.append(downsample(out[-1]))
    return out


def live_pyramid(colour_image, levels=DP.LEVELS):
    return pyramid_from_level0(live_level0(colour_image), levels)


def prediction_pyramid(pred_colour, levels=DP.LEVELS):
    return pyramid_from_level0(prediction_level0(pred_colour), levels)


def photometric_terms(i_live, i_pred, intr, twist_p, rows, cols, valid, g, max_difference=np.inf):
    """the intensity term of the pairs of one pyramid level, taken at that level: (has, r_I, J_I) as
    photometric_restatement.photometric_terms gives them, with the level's intrinsics intr = (fx, fy, cx, cy) and
    extents in place of the image's, i_pred (the level of the prediction's pyramid) in place of the colour image's Y,
    and I_l = float64(i_live) at the live pixel.  The interpolation, the derivatives and the Jacobian are that
    function's own: it is called on the level with a black live image, which makes its residual I_p - 0 = I_p"""
    fx, fy, cx, cy = intr
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)
    i_pred = np.asarray(i_pred, np.float32)
    i_live = np.asarray(i_live, np.float32)
    image = np.zeros(i_pred.shape + (4,), np.float32)
    image[..., 3] = i_pred
    black = np.zeros(i_live.shape + (3,), np.uint8)
    has, Ip, J = PR.photometric_terms(black, image, K, twist_p, rows, cols, valid, g)
    with np.errstate(invalid="ignore"):
        rI = Ip - i_live[rows, cols].astype(np.float64)
        has = has & (np.abs(rI) <= float(max_difference))
    return has, rI, J


def iteration(d, n_live, i_live, i_pred, intr, pred_depth, pred_normals, K, twist, twist_p, lam,
              max_distance=I.MAX_DISTANCE, cos_max=None, max_difference=np.inf):
    """one joint iteration on one pyramid level at twist: depth_pyramid_restatement.iteration's pairs (every pixel of
    the level d with its normals n_live and intrinsics intr, the gate with cos_max) and, for every pair,
    photometric_terms on the level's two intensity images.  Returns (record, residual image, intensity residual image,
    next twist), both images of the level's extents; the record is photometric_restatement.iteration's with
    angle_rejected"""
    d = np.asarray(d, np.float32)
    rows, cols, valid, rejected, g, Vw, Nw = I.associate(d, pred_depth, pred_normals, K, 1.0, twist, twist_p, 1,
                                                         max_distance, intr, n_live, cos_max)
    diff = [g[i] - Vw[i] for i in range(3)]
    with np.errstate(invalid="ignore"):
        r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2]
        J = [Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
             g[0] * Nw[1] - g[1] * Nw[0]]
    has, rI, JI = photometric_terms(i_live, i_pred, intr, twist_p, rows, cols, valid, g, max_difference)
    lam = float(lam)
    with np.errstate(invalid="ignore"):
        Jh = [lam * j for j in JI]
        rh = lam * rI
    a, a_abs = np.zeros((6, 6)), np.zeros((6, 6))
    b, b_abs = np.zeros(6), np.zeros(6)
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = np.sum((J[i] * J[j])[valid]) + np.sum((Jh[i] * Jh[j])[has])
            a_abs[i, j] = a_abs[j, i] = np.sum(np.abs(J[i] * J[j])[valid]) + np.sum(np.abs(Jh[i] * Jh[j])[has])
        b[i] = -(np.sum((J[i] * r)[valid]) + np.sum((Jh[i] * rh)[has]))
        b_abs[i] = np.sum(np.abs(J[i] * r)[valid]) + np.sum(np.abs(Jh[i] * rh)[has])
    residuals = np.full(d.shape, np.nan, np.float32)
    residuals[rows[valid], cols[valid]] = r[valid].astype(np.float32)
    intensity = np.full(d.shape, np.nan, np.float32)
    intensity[rows[has], cols[has]] = rI[has].astype(np.float32)
    twist = np.asarray(twist, np.float64).reshape(6)
    skipped = 1 if not np.all(np.isfinite(a)) else I._singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        twist = I.compose(twist, delta)
    rec = dict(A=a, b=b, energy=float(np.sum((r * r)[valid])), count=int(valid.sum()), delta=delta,
               twist=twist.copy(), skipped=skipped, A_abs=a_abs, b_abs=b_abs, angle_rejected=int(rejected.sum()),
               photometric_count=int(has.sum()), photometric_energy=float(np.sum((rI * rI)[has])))
    return rec, residuals, intensity, twist


def icp(levels, i_live, i_pred, pred_depth, pred_normals, K, twist_p, lam, twist=None, iterations=I.ITERATIONS,
        max_distance=I.MAX_DISTANCE, cos_max=None, max_difference=np.inf):
    """the joint run over a depth pyramid (depths, normals, intrinsics) and the two intensity pyramids, coarse first:
    entry k of iterations runs on level len(iterations) - 1 - k.  Returns (records, final twist, the last iteration's
    residual image, its intensity residual image; None for both without an iteration); each record carries its entry
    index as `level`"""
    depths, norms, intr = levels
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records, residuals, intensity = [], None, None
    n = len(iterations)
    for k, count in enumerate(iterations):
        l = n - 1 - k
        for _ in range(count):
            rec, residuals, intensity, twist = iteration(depths[l], norms[l], i_live[l], i_pred[l], intr[l],
                                                         pred_depth, pred_normals, K, twist, twist_p, lam,
                                                         max_distance, cos_max, max_difference)
            rec["level"] = k
            records.append(rec)
    return records, twist, residuals, intensity


def sequence(frames, images, K, ratio, shape, offset, lam, iterations=I.ITERATIONS, max_distance=I.MAX_DISTANCE,
             cos_max=None, max_difference=np.inf, pyramid_settings=None, band=20, voxel_size=0.004, colour_band=1.0):
    """SequenceFusion3d(colour=True, tracking_reference="icp", icp_pyramid=, icp_intensity_pyramid=,
    photometric_weight=lam) without a non-rigid step: photometric_restatement.sequence with each frame k >= 1 tracked
    by icp() over its depth pyramid (pyramid_settings: keyword arguments of depth_pyramid_restatement.pyramid) and
    the intensity pyramids of its colour image and of the prediction; fusion integrates the raw depth and the colour.
    Returns (tsdf, weight, colour, twists, prediction hits, ICP records per frame)."""
    settings = dict(pyramid_settings or {})
    levels = settings.get("levels", DP.LEVELS)
    tsdf, weight = F.empty_model(shape)
    colour = np.zeros(tuple(shape) + (4,), np.float32)
    twist = np.zeros(6)
    twists, hits, icp_records = [], [], []
    for k, (depth, image) in enumerate(zip(frames, images)):
        recs, h = [], None
        if k > 0 and sum(iterations) > 0:
            pd, pn, h, pc = PR.raycast_colour(tsdf, weight, colour, K, twist, offset, voxel_size, np.shape(depth),
                                              normals=True)
            recs, twist, _, _ = icp(DP.pyramid(depth, ratio, K, **settings), live_pyramid(image, levels),
                                    prediction_pyramid(pc, levels), pd, pn, K, twist, lam, twist, iterations,
                                    max_distance, cos_max, max_difference)
        hits.append(h)
        icp_records.append(recs)
        tsdf, weight, colour, _ = C.fuse_depth_colour(tsdf, weight, colour, depth, image, K, ratio, offset, twist,
                                                      band, voxel_size, 1.0, np.inf, colour_band=colour_band)
        twists.append(np.array(twist, dtype=np.float64))
    return tsdf, weight, colour, twists, hits, icp_records
