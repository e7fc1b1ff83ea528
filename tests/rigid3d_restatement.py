"""numpy restatement of the 6-DoF SDF-2-SDF rigid tracker's per-voxel arithmetic ("The rigid
tracker"): the reference's 2-D algorithm (rigid_opt/sdf_gradient_field.py, rigid_opt/sdf_2_sdf_optimizer2d.py) lifted
to 3-D with the 2-D kernel's dtype choices.  The HIP kernel (csrc/lsf_rigid3d.hip) must equal it bit for bit per voxel;
sums over voxels are compared with a tolerance, since the device reduces in a tree.  Host numpy only: no package
import."""
import numpy as np

from rigid_restatement import _coords, matrix3d, tsdf_nearest

__all__ = ["matrix3d", "tsdf_nearest", "live_volume", "gradient_wrt_twist_3d", "iteration_sums", "singular_class",
           "optimize"]


def live_volume(depth, K, ratio, shape, offset, twist, band=20, voxel_size=0.004, default=1.0):
    """the live (Z, Y, X) volume under twist: twist_vector_to_matrix3d of the float32-rounded twist, float64 product"""
    t32 = np.asarray(twist, dtype=np.float64).reshape(6).astype(np.float32)
    return tsdf_nearest(depth, K, ratio, shape, offset, matrix3d(t32), band, voxel_size, None, default)


def gradient_wrt_twist_3d(live, twist, offset, voxel_size=0.004):
    """(Z, Y, X, 6) float32: [grad ; p x grad] / voxel_size, p = twist_vector_to_matrix3d(-twist) . (point, 1)"""
    live = np.asarray(live, dtype=np.float32)
    offset = np.asarray(offset, dtype=np.float64).reshape(3)
    gz, gy, gx = np.gradient(live)
    m = matrix3d(-np.asarray(twist, dtype=np.float64).reshape(6))
    nz, ny, nx = live.shape
    x = np.broadcast_to(_coords(nx, offset[0], voxel_size)[None, None, :], live.shape).astype(np.float64)
    y = np.broadcast_to(_coords(ny, offset[1], voxel_size)[None, :, None], live.shape).astype(np.float64)
    z = np.broadcast_to(_coords(nz, offset[2], voxel_size)[:, None, None], live.shape).astype(np.float64)
    px, py, pz = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] * 1.0 for k in range(3)]
    fx, fy, fz = gx.astype(np.float64), gy.astype(np.float64), gz.astype(np.float64)
    vs = np.float32(voxel_size)
    channels = [fx, fy, fz, py * fz - pz * fy, pz * fx - px * fz, px * fy - py * fx]
    return np.stack([c.astype(np.float32) / vs for c in channels], axis=-1)


def iteration_sums(canonical, live, g, twist, eta):
    """A (6x6), b (6,), energy of one iteration, float64 (products of A in float32)"""
    g = g.reshape(-1, 6)
    c, l = canonical.reshape(-1), live.reshape(-1)
    a = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = np.sum((g[:, i] * g[:, j]).astype(np.float64))
    t = np.asarray(twist, dtype=np.float64).reshape(6)
    gd = g.astype(np.float64)
    dot = gd[:, 0] * t[0]
    for i in range(1, 6):
        dot = dot + gd[:, i] * t[i]
    r = (c - l).astype(np.float64) + dot
    b = np.array([np.sum(r * gd[:, i]) for i in range(6)])
    ne = np.float32(-eta)
    d = c.astype(np.float64) * (c > ne) - l.astype(np.float64) * (l > ne)
    return a, b, 0.5 * np.sum(d * d)


def singular_class(a):
    """the device's rule: 1 = skip (a non-finite entry, or an exact zero pivot in LU with partial pivoting), 0 = invert"""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return 1
    m = a.copy()
    n = m.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if m[p, c] == 0.0:
            return 1
        m[[c, p]] = m[[p, c]]
        for r in range(c + 1, n):
            f = m[r, c] / m[c, c]
            m[r, c + 1:] = m[r, c + 1:] - f * m[c, c + 1:]
    return 0


def step(canonical, live_depth, K, ratio, offset, twist, band, eta=0.01, voxel_size=0.004, rate=0.5):
    """one iteration at twist: (record dict, next twist)"""
    twist = np.asarray(twist, dtype=np.float64).reshape(6)
    live = live_volume(live_depth, K, ratio, canonical.shape, offset, twist, band, 0.004)
    g = gradient_wrt_twist_3d(live, twist, offset, voxel_size)
    a, b, energy = iteration_sums(canonical, live, g, twist, eta)
    skipped = singular_class(a)
    ts = np.zeros(6)
    if skipped == 0:
        ts = np.dot(np.linalg.inv(a), b)
        twist = twist + rate * (ts - twist)
    return dict(A=a, b=b, energy=energy, twist_star=ts, twist=twist.copy(), skipped=skipped), twist


def optimize(canonical, live_depth, K, ratio, offset, iterations, band, eta=0.01, voxel_size=0.004, rate=0.5,
             twist=None):
    """the 2-D reference's loop in 3-D on the restatement: list of per-iteration dicts and the final (6,) twist"""
    twist = np.zeros(6) if twist is None else np.asarray(twist, dtype=np.float64).reshape(6)
    records = []
    for _ in range(iterations):
        rec, twist = step(canonical, live_depth, K, ratio, offset, twist, band, eta, voxel_size, rate)
        records.append(rec)
    return records, twist
