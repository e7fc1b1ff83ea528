"""numpy restatement of point-to-SDF tracking with a colour term against the colour volume and on the depth pyramid
("Point-to-SDF tracking": "The colour term", "The pyramid source"), and of
SequenceFusion3d(colour=True, tracking_reference="sdf") with such a tracker.  The geometric pair is
point_sdf_restatement's, unchanged; the HIP kernel (csrc/lsf_point_sdf.hip) must equal the per-pixel arithmetic bit for
bit (both residual images, the weight image, the three counts); A, b, the energies and the weight sums are sums, which
the device reduces in a tree, so they are compared with a tolerance.  Every step below is one float64 IEEE operation in
the order written; numpy never contracts, and the kernel is built with -ffp-contract=off.  The depth pyramid is
depth_pyramid_restatement's, the intensity pyramid pyramid_photometric_restatement's, the weights
robust_icp_restatement's, the colour fusion colour_restatement's.  Host numpy only: no package import."""
from collections import namedtuple

import numpy as np

import colour_restatement as C
import depth_pyramid_restatement as DP
import fusion_restatement as F
import icp_restatement as I
import point_sdf_restatement as P
import pyramid_photometric_restatement as PP
import robust_icp_restatement as RR
from rigid_restatement import rodrigues

__all__ = ["Source", "strided_source", "pyramid_source", "luminance", "trilinear_gradient", "terms", "iteration",
           "track", "track_pyramid", "sequence"]

# the pixels of one launch: their depth in metres (float64, a pixel has one when > 0), their coordinates u, v in the
# level's image, the level's (fx, fy, cx, cy), their own intensity I_l (float64; None without a colour input), and where
# they go in the residual images: image[rows, cols] of an image of `shape`
Source = namedtuple("Source", ["depth", "u", "v", "intrinsics", "intensity", "rows", "cols", "shape"])


def luminance(rgb):
    """Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 in float64 of R, G, B (uint8 bytes or float32 records) in 0 .. 255"""
    rgb = np.asarray(rgb).astype(np.float64)
    return ((0.299 * rgb[..., 0] + 0.587 * rgb[..., 1]) + 0.114 * rgb[..., 2]) / 255.0


def strided_source(live_depth, K, ratio, stride=1, live_colour=None):
    """the pixels (stride * i, stride * j) of the live image; I_l is the luminance of the pixel's own bytes,
    unrounded"""
    K = np.asarray(K)
    d = I.scaled_depth(live_depth, ratio)
    rows, cols = np.meshgrid(np.arange(0, d.shape[0], stride), np.arange(0, d.shape[1], stride), indexing="ij")
    intensity = None if live_colour is None else luminance(np.asarray(live_colour)[rows, cols])
    return Source(d[rows, cols], cols.astype(np.float64), rows.astype(np.float64),
                  (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), intensity, rows, cols, d.shape)


def pyramid_source(depth_level, intrinsics, intensity_level=None):
    """every pixel of one level of a depth pyramid (float32 metres) with that level's intrinsics; I_l is the same
    level of the frame's intensity pyramid, float32 widened to double"""
    d = np.asarray(depth_level, np.float32).astype(np.float64)
    rows, cols = np.meshgrid(np.arange(d.shape[0]), np.arange(d.shape[1]), indexing="ij")
    intensity = None if intensity_level is None else np.asarray(intensity_level, np.float32).astype(np.float64)
    return Source(d, cols.astype(np.float64), rows.astype(np.float64), tuple(float(x) for x in intrinsics), intensity,
                  rows, cols, d.shape)


def trilinear_gradient(t, f):
    """(value, [dx, dy, dz]) of the trilinear interpolant of the corner values t0 .. t7 (x fastest, then y, then z) at
    the fractions f = (fx, fy, fz): point_sdf_restatement.sample_gradient's formulas on given corner values"""
    fx, fy, fz = f
    hx, hy, hz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    c00 = t[0] * hx + t[1] * fx
    c01 = t[2] * hx + t[3] * fx
    c10 = t[4] * hx + t[5] * fx
    c11 = t[6] * hx + t[7] * fx
    c0 = c00 * hy + c01 * fy
    c1 = c10 * hy + c11 * fy
    dx = ((t[1] - t[0]) * hy + (t[3] - t[2]) * fy) * hz + ((t[5] - t[4]) * hy + (t[7] - t[6]) * fy) * fz
    dy = (c01 - c00) * hz + (c11 - c10) * fz
    dz = c1 - c0
    return c0 * hz + c1 * fz, [dx, dy, dz]


def terms(tsdf, weight, source, twist, offset, max_distance=P.MAX_DISTANCE, band=20, voxel_size=0.004, colour=None,
          max_difference=np.inf):
    """the per-pixel quantities of one iteration at twist, arrays of the source's shape: dict(live, valid, pair, r, J,
    g, p) and, with a colour volume, (has, r_I, J_I) -- J_I unscaled.  `p` are the voxel coordinates"""
    tsdf = np.asarray(tsdf, np.float32)
    weight = np.asarray(weight, np.float32)
    off = np.asarray(offset, np.float64).reshape(3)
    vs = float(voxel_size)
    mu = float(band) * vs
    fx, fy, cx, cy = source.intrinsics
    tw = np.asarray(twist, np.float64).reshape(6)
    R, t = rodrigues(tw[3:]), tw[:3]
    dd = source.depth
    with np.errstate(invalid="ignore", over="ignore"):
        live = dd > 0.0
        vx = [dd * ((source.u - cx) / fx), dd * ((source.v - cy) / fy), dd * 1.0]
        g = I._rt(R, vx, t)
        p = [g[j] / vs - off[j] for j in range(3)]
        valid, phi, dv = P.sample_gradient(tsdf, weight, p)
        r = mu * phi
        grad = [(mu * dv[j]) / vs for j in range(3)]
        pair = live & valid & (np.abs(r) <= float(max_distance)) & \
            ((grad[0] != 0.0) | (grad[1] != 0.0) | (grad[2] != 0.0))
        J = [grad[0], grad[1], grad[2], g[1] * grad[2] - g[2] * grad[1], g[2] * grad[0] - g[0] * grad[2],
             g[0] * grad[1] - g[1] * grad[0]]
        out = dict(live=live, valid=valid, pair=pair, r=r, J=J, g=g, p=p)
        if colour is None:
            return out
        colour = np.asarray(colour, np.float32)
        i0 = [np.floor(np.where(valid, p[j], 0.0)).astype(np.int64) for j in range(3)]
        f = [np.where(valid, p[j], 0.0) - i0[j].astype(np.float64) for j in range(3)]
        x0, y0, z0 = i0
        has = pair.copy()
        y = []
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    rec = colour[z0 + dz, y0 + dy, x0 + dx]
                    has &= rec[..., 3] > 0
                    y.append(luminance(rec))
        Y, dY = trilinear_gradient(y, f)
        rI = Y - source.intensity
        has &= np.abs(rI) <= float(max_difference)  # NaN fails
        gI = [dY[j] / vs for j in range(3)]
        JI = [gI[0], gI[1], gI[2], g[1] * gI[2] - g[2] * gI[1], g[2] * gI[0] - g[0] * gI[2],
              g[0] * gI[1] - g[1] * gI[0]]
        out.update(has=has, rI=rI, JI=JI)
    return out


def _image(source, mask, values):
    out = np.full(source.shape, np.nan, np.float32)
    out[source.rows[mask], source.cols[mask]] = values[mask].astype(np.float32)
    return out


def iteration(tsdf, weight, source, twist, offset, max_distance=P.MAX_DISTANCE, band=20, voxel_size=0.004, loss=None,
              colour=None, lam=0.0, max_difference=np.inf):
    """one iteration at twist over the source's pixels: (record dict, residual image, intensity residual image (None
    without a colour volume), weight image (None without a loss), next twist).  The images have the source's shape,
    float32, NaN where a pixel has no pair / no colour term.  loss: None or a robust_icp_restatement.Loss; its scale
    weighs r, its intensity_scale the unscaled r_I"""
    q = terms(tsdf, weight, source, twist, offset, max_distance, band, voxel_size, colour, max_difference)
    pair, r, J = q["pair"], q["r"], q["J"]
    tw = np.asarray(twist, np.float64).reshape(6)
    lam = float(lam)
    with np.errstate(invalid="ignore", over="ignore"):
        if loss is None:
            w, outlier, wJ = np.ones_like(r), np.zeros(r.shape, bool), J
        else:
            w, outlier = RR.weight(loss.kind, r, float(loss.scale))
            wJ = [w * j for j in J]
        rows = [(pair, wJ, J, r)]
        energy = float(np.sum((r * r)[pair])) if loss is None else float(np.sum(((w * r) * r)[pair]))
        photo = dict(photometric_count=0, photometric_energy=0.0, photometric_weight_sum=0.0)
        if colour is not None:
            has, rI = q["has"], q["rI"]
            Jh = [lam * j for j in q["JI"]]
            rh = lam * rI
            if loss is None:
                wI, wJh = np.ones_like(rI), Jh
                e_I = float(np.sum((rI * rI)[has]))
            else:
                wI, _ = RR.weight(loss.kind, rI, float(loss.intensity_scale))
                wJh = [wI * j for j in Jh]
                e_I = float(np.sum(((wI * rI) * rI)[has]))
                photo["photometric_weight_sum"] = float(np.sum(wI[has]))
            rows.append((has, wJh, Jh, rh))
            photo.update(photometric_count=int(has.sum()), photometric_energy=e_I)
        a, a_abs = np.zeros((6, 6)), np.zeros((6, 6))
        b, b_abs = np.zeros(6), np.zeros(6)
        for mask, wj, j_, res in rows:
            for i in range(6):
                for j in range(i, 6):
                    a[i, j] += np.sum((wj[i] * j_[j])[mask])
                    a_abs[i, j] += np.sum(np.abs(wj[i] * j_[j])[mask])
                b[i] -= np.sum((wj[i] * res)[mask])
                b_abs[i] += np.sum(np.abs(wj[i] * res)[mask])
        for i in range(6):
            for j in range(i):
                a[i, j], a_abs[i, j] = a[j, i], a_abs[j, i]
    residuals = _image(source, pair, r)
    intensity = None if colour is None else _image(source, q["has"], q["rI"])
    weights = None if loss is None else _image(source, pair, w)
    skipped = 1 if not np.all(np.isfinite(a)) else I._singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        tw = I.compose(tw, delta)
    # A_abs, b_abs: the sums of the terms' magnitudes, the scale of a sum's rounding in another order
    rec = dict(A=a, b=b, energy=energy, count=int(pair.sum()), delta=delta, twist=tw.copy(), skipped=skipped,
               A_abs=a_abs, b_abs=b_abs, no_sample=int((q["live"] & ~q["valid"]).sum()),
               weight_sum=0.0 if loss is None else float(np.sum(w[pair])), outliers=int((outlier & pair).sum()))
    rec.update(photo)
    return rec, residuals, intensity, weights, tw


def _run(tsdf, weight, sources, iterations, twist, offset, max_distance, band, voxel_size, loss, colour, lam,
         max_difference):
    twist = np.asarray(twist, np.float64).reshape(6).copy()
    records, residuals, intensity, weights = [], None, None, None
    for level, (n, source) in enumerate(zip(iterations, sources)):
        for _ in range(n):
            rec, residuals, intensity, weights, twist = iteration(tsdf, weight, source, twist, offset, max_distance,
                                                                  band, voxel_size, loss, colour, lam, max_difference)
            rec["level"] = level
            records.append(rec)
    return records, twist, residuals, intensity, weights


def track(tsdf, weight, live_depth, K, ratio, twist, offset, iterations=P.ITERATIONS, strides=P.STRIDES,
          max_distance=P.MAX_DISTANCE, band=20, voxel_size=0.004, loss=None, colour=None, live_colour=None, lam=0.0,
          max_difference=np.inf):
    """the whole strided run from twist, coarse first: (records, final twist, the last iteration's residual image,
    intensity residual image and weight image).  colour, live_colour and lam go together"""
    sources = [strided_source(live_depth, K, ratio, s, live_colour if colour is not None else None) for s in strides]
    return _run(tsdf, weight, sources, iterations, twist, offset, max_distance, band, voxel_size, loss, colour, lam,
                max_difference)


def track_pyramid(tsdf, weight, depths, intrinsics, twist, offset, iterations=P.ITERATIONS,
                  max_distance=P.MAX_DISTANCE, band=20, voxel_size=0.004, loss=None, colour=None, intensities=None,
                  lam=0.0, max_difference=np.inf):
    """the whole run over a depth pyramid (depths, intrinsics: depth_pyramid_restatement.pyramid's; intensities:
    pyramid_photometric_restatement.live_pyramid's), entry k of iterations on level len(iterations) - 1 - k"""
    n = len(iterations)
    sources = [pyramid_source(depths[n - 1 - k], intrinsics[n - 1 - k],
                              None if colour is None else intensities[n - 1 - k]) for k in range(n)]
    return _run(tsdf, weight, sources, iterations, twist, offset, max_distance, band, voxel_size, loss, colour, lam,
                max_difference)


def sequence(frames, images, K, ratio, shape, offset, lam=None, iterations=P.ITERATIONS, strides=P.STRIDES,
             max_distance=P.MAX_DISTANCE, band=20, voxel_size=0.004, initial_twist=None, colour_band=1.0, loss=None,
             pyramid=None, max_difference=np.inf):
    """SequenceFusion3d(colour=True, tracking_reference="sdf") without a non-rigid step: frame 0 fused with its colour
    under initial_twist; frame k >= 1 tracked from twist_{k-1} against the model (lam None: geometry alone; pyramid:
    None for the strided source, or the keywords of depth_pyramid_restatement.pyramid), then fused with its colour.
    Returns (tsdf, weight, colour volume, twists, tracking records per frame)."""
    tsdf, weight = F.empty_model(shape)
    colour = np.zeros(tuple(shape) + (4,), np.float32)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, sdf_records = [], []
    for k, (depth, image) in enumerate(zip(frames, images)):
        recs = []
        if k > 0 and sum(iterations) > 0:
            joint = dict(colour=colour, lam=lam, max_difference=max_difference) if lam is not None else {}
            if pyramid is None:
                recs, twist = track(tsdf, weight, depth, K, ratio, twist, offset, iterations, strides, max_distance,
                                    band, voxel_size, loss, live_colour=image, **joint)[:2]
            else:
                depths, _, intr = DP.pyramid(depth, ratio, K, **pyramid)
                recs, twist = track_pyramid(tsdf, weight, depths, intr, twist, offset, iterations, max_distance, band,
                                            voxel_size, loss, intensities=PP.live_pyramid(image, len(depths)),
                                            **joint)[:2]
        sdf_records.append(recs)
        tsdf, weight, colour, _ = C.fuse_depth_colour(tsdf, weight, colour, depth, image, K, ratio, offset, twist, band,
                                                      voxel_size, colour_band=colour_band)
        twists.append(np.array(twist, dtype=np.float64))
    return tsdf, weight, colour, twists, sdf_records
