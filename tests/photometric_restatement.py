"""numpy restatement of the ray-cast colour image and of the joint geometric and photometric ICP (INTEGRATION.md
section 3, "Ray-cast colour" and "Photometric ICP"), on top of raycast_restatement and icp_restatement, and of
SequenceFusion3d(colour=True, tracking_reference="icp", photometric_weight=).  The HIP kernels (lsf_raycast_colour in
csrc/lsf_raycast.hip, lsf_icp_run_photometric in csrc/lsf_icp.hip) must equal the per-pixel arithmetic bit for bit (the
colour image, both residual images, both counts); A, b and the energies are sums, compared with a tolerance.  Every step
is one float64 IEEE operation in the order written.  Host numpy only: no package import."""
import numpy as np

import colour_restatement as C
import fusion_restatement as F
import icp_restatement as I
import raycast_restatement as RC

__all__ = ["hit_depth64", "sample_colour", "raycast_colour", "photometric_terms", "iteration", "icp", "sequence"]


def _ray(K, twist, offset, voxel_size, image_shape):
    """raycast_restatement's ray in voxel coordinates, g(s) = a + s b per pixel"""
    h, w = int(image_shape[0]), int(image_shape[1])
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    vs = float(voxel_size)
    E = RC.extrinsic(twist)
    R, t = E[:, :3], E[:, 3]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = [(u - cx) / fx, (v - cy) / fy]
    a, b = [], []
    for j in range(3):
        o = -((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2])
        d = (R[0, j] * dc[0] + R[1, j] * dc[1]) + R[2, j] * 1.0
        a.append(np.full((h, w), o / vs - off[j]))
        b.append(d / vs)
    return a, b


def hit_depth64(tsdf, weight, depth, hit, a, b, voxel_size):
    """the refined float64 depth along the ray of every hit pixel, before raycast_restatement.raycast rounded it to
    `depth`: the crossing (previous sample valid and > 0, own sample valid and <= 0) among the steps around depth whose
    refinement rounds to it.  Steps are searched in marching order, so the first crossing is found"""
    ds = float(voxel_size) / RC.STEPS_PER_VOXEL
    rows, cols = np.nonzero(hit)
    A = [a[j][rows, cols] for j in range(3)]
    B = [b[j][rows, cols] for j in range(3)]
    d32 = depth[rows, cols]
    k = np.floor(d32.astype(np.float64) / ds).astype(np.int64)
    out = np.full(rows.size, np.nan)
    for dm in (-1, 0, 1, 2):
        m = k + dm
        sp, sv = (m - 1).astype(np.float64) * ds, m.astype(np.float64) * ds
        pvalid, p = RC._sample(tsdf, weight, [A[j] + sp * B[j] for j in range(3)])
        valid, val = RC._sample(tsdf, weight, [A[j] + sv * B[j] for j in range(3)])
        with np.errstate(divide="ignore", invalid="ignore"):
            s = sp + ds * (p / (p - val))
        found = np.isnan(out) & pvalid & (p > 0.0) & valid & (val <= 0.0) & (s.astype(np.float32) == d32)
        out[found] = s[found]
    assert not np.isnan(out).any()
    return rows, cols, out


def sample_colour(colour, n, g):
    """(valid, [R, G, B]) of trilinear samples of the colour records at voxel coordinates g: raycast_restatement's
    sample per channel; valid when the 8 corners lie inside the volume and all 8 colour weights are > 0"""
    valid = np.ones(g[0].shape, bool)
    for j in range(3):
        valid &= (g[j] >= 0.0) & (g[j] < float(n[j] - 1))
    i0 = [np.floor(np.where(valid, g[j], 0.0)).astype(np.int64) for j in range(3)]
    f = [np.where(valid, g[j], 0.0) - i0[j].astype(np.float64) for j in range(3)]
    x0, y0, z0 = i0
    with np.errstate(invalid="ignore"):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    valid &= colour[z0 + dz, y0 + dy, x0 + dx, 3] > 0
    fx, fy, fz = f
    gx, gy, gz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    out = []
    for ch in range(3):
        c = {(dz, dy, dx): colour[z0 + dz, y0 + dy, x0 + dx, ch].astype(np.float64)
             for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
        c00 = c[0, 0, 0] * gx + c[0, 0, 1] * fx
        c01 = c[0, 1, 0] * gx + c[0, 1, 1] * fx
        c10 = c[1, 0, 0] * gx + c[1, 0, 1] * fx
        c11 = c[1, 1, 0] * gx + c[1, 1, 1] * fx
        c0 = c00 * gy + c01 * fy
        c1 = c10 * gy + c11 * fy
        out.append(c0 * gz + c1 * fz)
    return valid, out


def raycast_colour(tsdf, weight, colour, K, twist, offset, voxel_size=0.004, image_shape=(480, 640), normals=False,
                   fallback=None, ratio=1.0):
    """raycast_restatement.raycast's (depth, normals, hits) and the colour image (H, W, 4) float32: (R, G, B, Y) at the
    unrounded hit point of every hit pixel with a valid colour sample, four NaNs elsewhere"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.float32)
    colour = np.asarray(colour, dtype=np.float32)
    depth, out_normals, hits = RC.raycast(tsdf, weight, K, twist, offset, voxel_size, image_shape, normals, fallback,
                                          ratio)
    h, w = int(image_shape[0]), int(image_shape[1])
    image = np.full((h, w, 4), np.nan, np.float32)
    if fallback is None:
        bare = depth
    else:
        bare, _, _ = RC.raycast(tsdf, weight, K, twist, offset, voxel_size, image_shape)
    hit = bare > 0
    assert int(hit.sum()) == hits
    if hits:
        a, b = _ray(K, twist, offset, voxel_size, image_shape)
        rows, cols, s = hit_depth64(tsdf, weight, bare, hit, a, b, voxel_size)
        g = [a[j][rows, cols] + s * b[j][rows, cols] for j in range(3)]
        valid, rgb = sample_colour(colour, (tsdf.shape[2], tsdf.shape[1], tsdf.shape[0]), g)
        y = ((0.299 * rgb[0] + 0.587 * rgb[1]) + 0.114 * rgb[2]) / 255.0
        for ch, value in enumerate(rgb + [y]):
            image[rows[valid], cols[valid], ch] = value[valid].astype(np.float32)
    return depth, out_normals, hits, image


def photometric_terms(live_colour, pred_colour, K, twist_p, rows, cols, valid, g, max_difference=np.inf):
    """the intensity term of associate()'s pairs: (has, r_I, J_I) over the strided pixels, J_I a list of six arrays,
    unscaled; `has` marks the pairs with a term"""
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    pc = np.asarray(pred_colour, np.float32)
    h, w = pc.shape[:2]
    Ep = RC.extrinsic(twist_p)
    Rp, tp = Ep[:, :3], Ep[:, 3]
    q = [((Rp[i, 0] * g[0] + Rp[i, 1] * g[1]) + Rp[i, 2] * g[2]) + tp[i] for i in range(3)]
    with np.errstate(all="ignore"):
        pu = (fx * q[0]) / q[2] + cx
        pv = (fy * q[1]) / q[2] + cy
        x0, y0 = np.floor(pu), np.floor(pv)
        has = valid & (0.0 <= x0) & (x0 + 1.0 <= float(w - 1)) & (0.0 <= y0) & (y0 + 1.0 <= float(h - 1))
        ix, iy = np.where(has, x0, 0.0).astype(np.int64), np.where(has, y0, 0.0).astype(np.int64)
        I00 = pc[iy, ix, 3].astype(np.float64)
        I10 = pc[iy, np.minimum(ix + 1, w - 1), 3].astype(np.float64)
        I01 = pc[np.minimum(iy + 1, h - 1), ix, 3].astype(np.float64)
        I11 = pc[np.minimum(iy + 1, h - 1), np.minimum(ix + 1, w - 1), 3].astype(np.float64)
        has &= np.isfinite(I00) & np.isfinite(I10) & np.isfinite(I01) & np.isfinite(I11)
        al, be = pu - x0, pv - y0
        ha, hb = 1.0 - al, 1.0 - be
        Ip = hb * (ha * I00 + al * I10) + be * (ha * I01 + al * I11)
        Iu = hb * (I10 - I00) + be * (I11 - I01)
        Iv = ha * (I01 - I00) + al * (I11 - I10)
        lc = np.asarray(live_colour)[rows, cols].astype(np.float64)
        Il = ((0.299 * lc[..., 0] + 0.587 * lc[..., 1]) + 0.114 * lc[..., 2]) / 255.0
        rI = Ip - Il
        has &= np.abs(rI) <= float(max_difference)
        su, sv = Iu * fx, Iv * fy
        c = [su / q[2], sv / q[2], -((su * q[0] + sv * q[1]) / (q[2] * q[2]))]
        a = [(Rp[0, j] * c[0] + Rp[1, j] * c[1]) + Rp[2, j] * c[2] for j in range(3)]
        J = [a[0], a[1], a[2], g[1] * a[2] - g[2] * a[1], g[2] * a[0] - g[0] * a[2], g[0] * a[1] - g[1] * a[0]]
    return has, rI, J


def iteration(live_depth, live_colour, pred_depth, pred_normals, pred_colour, K, ratio, twist, twist_p, lam, stride=1,
              max_distance=I.MAX_DISTANCE, max_difference=np.inf):
    """one joint iteration at twist: (record, residual image, intensity residual image, next twist).  The geometric
    pairs, r and J are icp_restatement's; a pair with a photometric term adds (lam J_I)(lam J_I)^T and
    -(lam J_I)(lam r_I).  energy and count stay the geometric ones"""
    rows, cols, valid, _, g, Vw, Nw = I.associate(live_depth, pred_depth, pred_normals, K, ratio, twist, twist_p,
                                                  stride, max_distance)
    diff = [g[i] - Vw[i] for i in range(3)]
    with np.errstate(invalid="ignore"):
        r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2]
        J = [Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
             g[0] * Nw[1] - g[1] * Nw[0]]
    has, rI, JI = photometric_terms(live_colour, pred_colour, K, twist_p, rows, cols, valid, g, max_difference)
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
    residuals = np.full(np.shape(live_depth), np.nan, np.float32)
    residuals[rows[valid], cols[valid]] = r[valid].astype(np.float32)
    intensity = np.full(np.shape(live_depth), np.nan, np.float32)
    intensity[rows[has], cols[has]] = rI[has].astype(np.float32)
    twist = np.asarray(twist, np.float64).reshape(6)
    skipped = 1 if not np.all(np.isfinite(a)) else I._singular(a)
    delta = np.zeros(6)
    if skipped == 0:
        delta = np.dot(np.linalg.inv(a), b)
        twist = I.compose(twist, delta)
    rec = dict(A=a, b=b, energy=float(np.sum((r * r)[valid])), count=int(valid.sum()), delta=delta,
               twist=twist.copy(), skipped=skipped, A_abs=a_abs, b_abs=b_abs, angle_rejected=0,
               photometric_count=int(has.sum()), photometric_energy=float(np.sum((rI * rI)[has])))
    return rec, residuals, intensity, twist


def icp(live_depth, live_colour, pred_depth, pred_normals, pred_colour, K, ratio, twist_p, lam, twist=None,
        iterations=I.ITERATIONS, strides=I.STRIDES, max_distance=I.MAX_DISTANCE, max_difference=np.inf):
    """the whole schedule, coarse first: (records, final twist).  Each record carries its level"""
    twist = np.asarray(twist_p if twist is None else twist, np.float64).reshape(6).copy()
    records = []
    for level, (n, s) in enumerate(zip(iterations, strides)):
        for _ in range(n):
            rec, _, _, twist = iteration(live_depth, live_colour, pred_depth, pred_normals, pred_colour, K, ratio,
                                         twist, twist_p, lam, s, max_distance, max_difference)
            rec["level"] = level
            records.append(rec)
    return records, twist


def sequence(frames, images, K, ratio, shape, offset, lam, iterations=I.ITERATIONS, strides=I.STRIDES,
             max_distance=I.MAX_DISTANCE, max_difference=np.inf, band=20, voxel_size=0.004, colour_band=1.0,
             initial_twist=None, max_weight=np.inf):
    """SequenceFusion3d(colour=True, tracking_reference="icp", photometric_weight=lam) without a non-rigid step: frame
    0 fused with its colour under initial_twist; frame k >= 1 tracked by the joint solve from twist_{k-1} against the
    model ray-cast with normals and colour at twist_{k-1}, then fused.  Returns (tsdf, weight, colour, twists, fusion
    records, prediction hits, ICP records per frame)."""
    tsdf, weight = F.empty_model(shape)
    colour = np.zeros(tuple(shape) + (4,), np.float32)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records, hits, icp_records = [], [], [], []
    for k, (depth, image) in enumerate(zip(frames, images)):
        recs, h = [], None
        if k > 0 and sum(iterations) > 0:
            pd, pn, h, pc = raycast_colour(tsdf, weight, colour, K, twist, offset, voxel_size, np.shape(depth),
                                           normals=True)
            recs, twist = icp(depth, image, pd, pn, pc, K, ratio, twist, lam, twist, iterations, strides, max_distance,
                              max_difference)
        hits.append(h)
        icp_records.append(recs)
        tsdf, weight, colour, rec = C.fuse_depth_colour(tsdf, weight, colour, depth, image, K, ratio, offset, twist,
                                                        band, voxel_size, 1.0, max_weight, colour_band=colour_band)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, colour, twists, records, hits, icp_records
