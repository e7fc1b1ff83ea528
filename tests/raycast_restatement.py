"""numpy restatement of ray-casting the canonical TSDF ("Ray-casting") and of
SequenceFusion3d's "raycast" tracking mode.  The HIP kernel (csrc/lsf_raycast.hip) must equal raycast() bit for bit in
depth and in normals, and exactly in the hit count.  Every step below is one float64 IEEE operation in the order
written; numpy never contracts, and the kernel is built with -ffp-contract=off.  Host numpy only: no package import."""
import numpy as np

import fusion_restatement as F
import rigid3d_restatement as R3

__all__ = ["STEPS_PER_VOXEL", "extrinsic", "raycast", "sequence"]

STEPS_PER_VOXEL = 2  # the march advances voxel_size / 2 in camera z per step


def extrinsic(twist):
    """(3, 4) float64: the generator's world -> camera matrix, twist_vector_to_matrix3d of the float32-rounded twist"""
    t32 = np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32)
    return R3.matrix3d(t32)[:3]


def _sample(tsdf, weight, g):
    """(valid, value) of trilinear samples at voxel coordinates g = (gx, gy, gz), each an array of one shape"""
    n = (tsdf.shape[2], tsdf.shape[1], tsdf.shape[0])
    valid = np.ones(g[0].shape, bool)
    for j in range(3):
        valid &= (g[j] >= 0.0) & (g[j] < float(n[j] - 1))
    i0 = [np.floor(np.where(valid, g[j], 0.0)).astype(np.int64) for j in range(3)]
    f = [np.where(valid, g[j], 0.0) - i0[j].astype(np.float64) for j in range(3)]
    x0, y0, z0 = i0
    corners = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = weight[z0 + dz, y0 + dy, x0 + dx]
                valid &= w > 0
                corners[dz, dy, dx] = tsdf[z0 + dz, y0 + dy, x0 + dx].astype(np.float64)
    fx, fy, fz = f
    gx, gy, gz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    c00 = corners[0, 0, 0] * gx + corners[0, 0, 1] * fx
    c01 = corners[0, 1, 0] * gx + corners[0, 1, 1] * fx
    c10 = corners[1, 0, 0] * gx + corners[1, 0, 1] * fx
    c11 = corners[1, 1, 0] * gx + corners[1, 1, 1] * fx
    c0 = c00 * gy + c01 * fy
    c1 = c10 * gy + c11 * fy
    return valid, c0 * gz + c1 * fz


def _fallback(fallback, ratio):
    """the fallback image in metres as float32, scaled as the generators scale depth"""
    d = np.asarray(fallback)
    if d.dtype == np.float32:
        return d * np.float32(ratio)
    if d.dtype in (np.uint16, np.float64):
        return (d.astype(np.float64) * float(ratio)).astype(np.float32)
    raise ValueError("fallback depth must be uint16, float32 or float64")


def raycast(tsdf, weight, K, twist, offset, voxel_size=0.004, image_shape=(480, 640), normals=False, fallback=None,
            ratio=1.0):
    """(depth (H, W) float32, normals (H, W, 3) float32 or None, hits) of the model seen from a camera at twist"""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.float32)
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    h, w = int(image_shape[0]), int(image_shape[1])
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    vs = float(voxel_size)
    ds = vs / STEPS_PER_VOXEL
    E = extrinsic(twist)
    R, t = E[:, :3], E[:, 3]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = [(u - cx) / fx, (v - cy) / fy]
    # the ray in voxel coordinates: g(s) = a + s b, s the camera z.  o = -R^T t, d = R^T (dc, 1)
    a, b = [], []
    for j in range(3):
        o = -((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2])
        d = (R[0, j] * dc[0] + R[1, j] * dc[1]) + R[2, j] * 1.0
        a.append(np.full((h, w), o / vs - off[j]))
        b.append(d / vs)
    # clip to the box of valid sample positions, 0 <= g < n - 1, then pad one step each way
    lo, hi = np.full((h, w), -np.inf), np.full((h, w), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(3):
            top = float(n[j] - 1)
            moving = b[j] != 0.0
            s1 = (0.0 - a[j]) / b[j]
            s2 = (top - a[j]) / b[j]
            lo = np.where(moving, np.maximum(lo, np.minimum(s1, s2)), lo)
            hi = np.where(moving, np.minimum(hi, np.maximum(s1, s2)), hi)
            outside = ~moving & ~((a[j] >= 0.0) & (a[j] < top))
            lo, hi = np.where(outside, np.inf, lo), np.where(outside, -np.inf, hi)
        march = (lo <= hi) & (hi > 0.0) & (hi / ds < 2.0 ** 50)
        k0 = np.where(march, np.maximum(np.floor(np.where(march, lo, 0.0) / ds) - 1.0, 1.0), 1.0).astype(np.int64)
        k1 = np.where(march, np.floor(np.where(march, hi, 0.0) / ds) + 1.0, 0.0).astype(np.int64)
    k1 = np.minimum(k1, k0 + 4 * (nx + ny + nz) + 8)
    k1 = np.where(march, k1, 0)
    depth64 = np.zeros((h, w))
    hit = np.zeros((h, w), bool)
    rows, cols = np.nonzero(march & (k1 >= k0))
    if rows.size:
        A = [a[j][rows, cols] for j in range(3)]
        B = [b[j][rows, cols] for j in range(3)]
        K0, K1 = k0[rows, cols], k1[rows, cols]
        pv, pval = np.zeros(rows.size, bool), np.zeros(rows.size)
        done = np.zeros(rows.size, bool)
        s_hit = np.zeros(rows.size)
        for k in range(int(K0.min()), int(K1.max()) + 1):
            live = ~done & (K0 <= k) & (k <= K1)
            idx = np.nonzero(live)[0]
            if idx.size == 0:
                continue
            s = float(k) * ds
            valid, val = _sample(tsdf, weight, [A[j][idx] + s * B[j][idx] for j in range(3)])
            # a ray's first sample (k == K0) meets pv False: it has no previous sample
            crossing = pv[idx] & (pval[idx] > 0.0) & valid & (val <= 0.0)
            c = idx[crossing]
            p = pval[c]
            s_hit[c] = float(k - 1) * ds + ds * (p / (p - val[crossing]))
            done[c] = True
            pv[idx], pval[idx] = valid, val
        hit[rows, cols] = done
        depth64[rows, cols] = s_hit
    depth = np.where(hit, depth64.astype(np.float32), np.float32(0))
    if fallback is not None:
        fb = _fallback(fallback, ratio)
        if fb.shape != (h, w):
            raise ValueError("fallback depth has shape %s, the image %s" % (fb.shape, (h, w)))
        depth = np.where(hit, depth, fb).astype(np.float32)
    out_normals = None
    if normals:
        out_normals = np.zeros((h, w, 3), np.float32)
        hr, hc = np.nonzero(hit)
        if hr.size:
            s = depth64[hr, hc]
            g = [a[j][hr, hc] + s * b[j][hr, hc] for j in range(3)]
            ok = np.ones(hr.size, bool)
            grad = []
            for j in range(3):
                gp = [g[i] + 1.0 if i == j else g[i] for i in range(3)]
                gm = [g[i] - 1.0 if i == j else g[i] for i in range(3)]
                vp, valp = _sample(tsdf, weight, gp)
                vm, valm = _sample(tsdf, weight, gm)
                ok &= vp & vm
                grad.append(valp - valm)
            nc = [(R[i, 0] * grad[0] + R[i, 1] * grad[1]) + R[i, 2] * grad[2] for i in range(3)]
            len2 = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
            ok &= len2 > 0.0
            norm = np.sqrt(np.where(ok, len2, 1.0))
            for i in range(3):
                out_normals[hr, hc, i] = np.where(ok, nc[i] / norm, 0.0).astype(np.float32)
    return depth.astype(np.float32), out_normals, int(hit.sum())


def sequence(frames, K, ratio, shape, offset, rigid_iterations=60, band=20, voxel_size=0.004, rate=0.5, eta=0.01,
             initial_twist=None, max_weight=np.inf):
    """SequenceFusion3d(tracking_reference="raycast") without a non-rigid step: frame 0 fused under initial_twist; frame
    k >= 1 tracked from twist_{k-1} against the live volume (ratio 1) of the model ray-cast at twist_{k-1}, holes filled
    from frame k-1, then fused in depth mode.  Returns (tsdf, weight, twists, fusion records, prediction hits)."""
    tsdf, weight = F.empty_model(shape)
    twist = np.zeros(6) if initial_twist is None else np.asarray(initial_twist, np.float64).reshape(6)
    twists, records, hits = [], [], []
    for k, depth in enumerate(frames):
        if k > 0 and rigid_iterations > 0:
            previous = frames[k - 1]
            prediction, _, h = raycast(tsdf, weight, K, twist, offset, voxel_size, previous.shape,
                                       fallback=previous, ratio=ratio)
            reference = R3.live_volume(prediction, K, 1.0, shape, offset, twist, band, voxel_size)
            _, twist = R3.optimize(reference, depth, K, ratio, offset, rigid_iterations, band, eta, voxel_size, rate,
                                   twist=twist)
            hits.append(h)
        else:
            hits.append(None)
        tsdf, weight, rec = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size, 1.0,
                                         max_weight)
        twists.append(np.array(twist, dtype=np.float64))
        records.append(rec)
    return tsdf, weight, twists, records, hits
