"""numpy restatement of the rigid tracker's per-voxel arithmetic, in the dtypes the reference's own expressions take
under numpy >= 2 (rigid_opt/sdf_gradient_field.py, rigid_opt/sdf_2_sdf_optimizer2d.py, tsdf/generation.py:130-207 and
:356-437).  The HIP kernels (csrc/lsf_tsdf_typed.h, csrc/lsf_rigid.hip) must equal it bit for bit per voxel; sums over
voxels are compared with a tolerance, since the device reduces in a tree.  Host numpy only: no package import."""
import math

import numpy as np


def matrix2d(twist):
    t = np.asarray(twist, dtype=np.float64).reshape(-1)
    m = np.identity(3)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = math.cos(t[2]), -math.sin(t[2]), math.sin(t[2]), math.cos(t[2])
    m[0, 2], m[1, 2] = t[0], t[1]
    return m


def rodrigues(r):
    dtype = np.float32 if np.asarray(r).dtype == np.float32 else np.float64
    r = np.asarray(r, dtype=np.float64).reshape(3)
    theta = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if theta < np.finfo(np.float64).eps:
        return np.eye(3, dtype=dtype)
    c, s = math.cos(theta), math.sin(theta)
    u = r * (1.0 / theta)
    cross = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return ((c * np.eye(3) + (1.0 - c) * np.outer(u, u)) + s * cross).astype(dtype)


def matrix3d(twist):
    t = np.asarray(twist)
    t = (t if t.dtype == np.float32 else t.astype(np.float64)).reshape(6)
    m = np.zeros((4, 4))
    m[0:3, 0:3] = rodrigues(t[3:6])
    m[0:3, 3] = t[0:3]
    m[3, 3] = 1.0
    return m


def _coords(n, offset, voxel_size):
    return ((np.arange(n, dtype=np.float64) + float(offset)) * voxel_size).astype(np.float32)


def _trunc_index(v):
    ok = np.isfinite(v) & (v > -2147483000.0) & (v < 2147483000.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0)), -1).astype(np.int64)


def tsdf_nearest(depth, K, ratio, shape, offset, E=None, band=20, voxel_size=0.004, row=None, default=1.0):
    """(H, W) slice (row given) or (Z, Y, X) volume, nearest pixel, float32"""
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    E = np.eye(4, dtype=np.float32) if E is None else np.asarray(E)
    et = np.float32 if E.dtype == np.float32 else np.float64
    E = E.astype(et)
    K = np.asarray(K)
    pt = np.float32 if K.dtype == np.float32 else np.float64
    qt = np.result_type(et, pt).type
    half = band / 2 * voxel_size
    if row is not None:
        h, w = shape
        x = np.broadcast_to(_coords(w, offset[0], voxel_size)[None, :], (h, w))
        y = np.zeros((h, w), np.float32)
        z = np.broadcast_to(_coords(h, offset[2], voxel_size)[:, None], (h, w))
    else:
        nz, ny, nx = shape
        x = np.broadcast_to(_coords(nx, offset[0], voxel_size)[None, None, :], shape)
        y = np.broadcast_to(_coords(ny, offset[1], voxel_size)[None, :, None], shape)
        z = np.broadcast_to(_coords(nz, offset[2], voxel_size)[:, None, None], shape)
    x, y, z = x.astype(et), y.astype(et), z.astype(et)
    pc = [((E[k, 0] * x + E[k, 1] * y) + E[k, 2] * z) + E[k, 3] * et(1) for k in range(3)]
    with np.errstate(all="ignore"):
        front = pc[2] > 0
        ix = _trunc_index(((qt(pt(K[0, 0])) * pc[0].astype(qt)) / pc[2].astype(qt) + qt(pt(K[0, 2]))) + qt(0.5))
        if row is None:
            iy = _trunc_index(((qt(pt(K[1, 1])) * pc[1].astype(qt)) / pc[2].astype(qt) + qt(pt(K[1, 2]))) + qt(0.5))
        else:
            iy = np.full(ix.shape, int(row), np.int64)
        inside = front & (ix >= 0) & (ix < depth.shape[1]) & (iy >= 0) & (iy < depth.shape[0])
        raw = depth[np.where(inside, iy, 0), np.where(inside, ix, 0)]
        if depth.dtype == np.float32:
            d = raw * np.float32(ratio)
        else:
            d = raw.astype(np.float64) * float(ratio)
        st = np.result_type(d.dtype, et).type
        sd = d.astype(st) - pc[2].astype(st)
        hs = st(half)
        val = np.where(sd < -hs, st(-1), np.where(sd > hs, st(1), sd / hs)).astype(np.float32)
        return np.where(inside & ~(d <= 0), val, np.float32(default)).astype(np.float32)


def gradient_wrt_twist(live, twist, offset, voxel_size=0.004):
    """calculate_gradient_wrt_twist, (H, W, 3) float32"""
    live = np.asarray(live, dtype=np.float32)
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    gy, gx = np.gradient(live)
    m = matrix2d(-np.asarray(twist, dtype=np.float64).reshape(3))
    h, w = live.shape
    x = np.broadcast_to(_coords(w, offset[0], voxel_size)[None, :], (h, w)).astype(np.float64)
    z = np.broadcast_to(_coords(h, offset[2], voxel_size)[:, None], (h, w)).astype(np.float64)
    t0 = (m[0, 0] * x + m[0, 1] * z) + m[0, 2] * 1.0
    t1 = (m[1, 0] * x + m[1, 1] * z) + m[1, 2] * 1.0
    fx, fy = gx.astype(np.float64), gy.astype(np.float64)
    vs = np.float32(voxel_size)
    g = np.stack([(fx * 1.0 + fy * 0.0).astype(np.float32) / vs, (fx * 0.0 + fy * 1.0).astype(np.float32) / vs,
                  (fx * t1 + fy * -t0).astype(np.float32) / vs], axis=-1)
    return g


def iteration_sums(canonical, live, g, twist, eta):
    """A (3x3), b (3,), energy of one iteration, float64 (products of A in float32)"""
    g = g.reshape(-1, 3)
    c, l = canonical.reshape(-1), live.reshape(-1)
    a = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            a[i, j] = np.sum((g[:, i] * g[:, j]).astype(np.float64))
    t = np.asarray(twist, dtype=np.float64).reshape(3)
    gd = g.astype(np.float64)
    r = (c - l).astype(np.float64) + ((gd[:, 0] * t[0] + gd[:, 1] * t[1]) + gd[:, 2] * t[2])
    b = np.array([np.sum(r * gd[:, i]) for i in range(3)])
    ne = np.float32(-eta)
    d = c.astype(np.float64) * (c > ne) - l.astype(np.float64) * (l > ne)
    return a, b, 0.5 * np.sum(d * d)


def singular_class(a):
    """the device's rule: 1 = skip (a non-finite entry, or an exact zero pivot in LU with partial pivoting), 0 = invert"""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return 1
    m = a.copy()
    for c in range(3):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if m[p, c] == 0.0:
            return 1
        m[[c, p]] = m[[p, c]]
        for r in range(c + 1, 3):
            f = m[r, c] / m[c, c]
            m[r, c + 1:] = m[r, c + 1:] - f * m[c, c + 1:]
    return 0


def optimize(canonical, live_depth, K, ratio, row, offset, iterations, band, eta=0.01, voxel_size=0.004, rate=0.5):
    """the reference's loop on the restatement: list of per-iteration dicts and the final (3,) twist"""
    twist = np.zeros(3)
    records = []
    for _ in range(iterations):
        t3 = np.array([twist[0], 0.0, twist[1], 0.0, twist[2], 0.0], dtype=np.float32)
        live = tsdf_nearest(live_depth, K, ratio, canonical.shape, offset, matrix3d(t3), band, 0.004, row)
        g = gradient_wrt_twist(live, twist, offset, voxel_size)
        a, b, energy = iteration_sums(canonical, live, g, twist, eta)
        skipped = singular_class(a)
        ts = np.zeros(3)
        if skipped == 0:
            ts = np.dot(np.linalg.inv(a), b)
            twist = twist + rate * (ts - twist)
        records.append(dict(A=a, b=b, energy=energy, twist_star=ts, twist=twist.copy(), skipped=skipped, live=live,
                            gradient=g))
    return records, twist
