"""numpy restatement of the RGB-D sensor front end ("RGB-D sensor"; include/lsf_hip.h,
lsf_rgbd_ray_table / _register_depth / _rectify_colour), which the HIP kernels of csrc/lsf_rgbd.hip must equal bit for
bit, the record's eight counts included.  Every float step is float64, one operation each in the order the contract
writes them; numpy never contracts a multiply and an add, and the kernels are built with -ffp-contract=off.  The z-buffer
is np.minimum.at on the bit patterns of float32(q_z): an unsigned minimum gives the same result in any order.  Written
from the contract: whole-image array expressions, a loop only over the footprint's max_footprint^2 places.  Host numpy
only: no package import."""
import numpy as np

ITERATIONS = 10
MAX_FOOTPRINT = 16
EMPTY = np.uint32(0x7f800000)
LIMIT = 2147483000.0
RECORD_FIELDS = ("valid", "behind", "outside", "empty", "clipped", "written", "filled", "masked")
BARREL = (-0.25, 0.08, 0.001, -0.0005)  # the lens of the tests: k1, k2, p1, p2


def coefficients(k):
    """the eight coefficients (k1, k2, p1, p2, k3, k4, k5, k6) as float64: 0, 4, 5 or 8 given in any shape, zero-padded"""
    k = np.zeros(0) if k is None else np.asarray(k, dtype=np.float64).reshape(-1)
    assert k.size in (0, 4, 5, 8), k.size
    return np.concatenate([k, np.zeros(8 - k.size)])


def _radial(x, y, k):
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in k)
    r2 = x * x + y * y
    num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return num, den, dx, dy


def distort(x, y, k):
    """(xd, yd) of normalised (x, y) under OpenCV's rational model"""
    with np.errstate(all="ignore"):
        num, den, dx, dy = _radial(x, y, coefficients(k))
        s = num / den
        return x * s + dx, y * s + dy


def undistort(xd, yd, k, iterations=ITERATIONS):
    """the fixed-point inverse: `iterations` steps from (xd, yd), none at all when every coefficient is 0"""
    k = coefficients(k)
    x, y = np.array(xd, dtype=np.float64), np.array(yd, dtype=np.float64)
    if not np.any(k != 0):
        return x, y
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            num, den, dx, dy = _radial(x, y, k)
            x, y = (xd - dx) * den / num, (yd - dy) * den / num
    return x, y


def intrinsics(K):
    """(fx, fy, cx, cy) as Python floats of a 3 x 3 matrix"""
    K = np.asarray(K)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def ray_table(height, width, K, k=None):
    """(corner_rays (H + 1, W + 1, 2), centre_rays (H, W, 2)) float64: the undistorted normalised coordinates at
    (u - 0.5, v - 0.5) and at (u, v)"""
    fx, fy, cx, cy = intrinsics(K)

    def rays(us, vs):
        v, u = np.meshgrid(vs, us, indexing="ij")
        with np.errstate(all="ignore"):
            x, y = undistort((u - cx) / fx, (v - cy) / fy, k)
        return np.stack([x, y], axis=-1)

    corner = rays(np.arange(width + 1, dtype=np.float64) - 0.5, np.arange(height + 1, dtype=np.float64) - 0.5)
    centre = rays(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    return corner, centre


def scaled_depth(depth, ratio):
    """the depth in metres as float64, scaled as the TSDF generators scale it"""
    depth = np.asarray(depth)
    with np.errstate(all="ignore"):
        if depth.dtype == np.uint16:
            return depth.astype(np.float64) * float(ratio)
        if depth.dtype == np.float32:
            return (depth * np.float32(ratio)).astype(np.float64)
        assert depth.dtype == np.float64, depth.dtype
        return depth * float(ratio)


def _move(R, t, p0, p1, p2):
    return [((R[i, 0] * p0 + R[i, 1] * p1) + R[i, 2] * p2) + t[i] for i in range(3)]


def register_depth(depth, ratio, corner_rays, centre_rays, depth_to_output, K_out, out_shape, max_footprint=8,
                   colour_valid=None):
    """(out_depth float32 (Ho, Wo), record dict) of one call.  depth_to_output: 4 x 4, q = R p + t"""
    depth = np.asarray(depth)
    H, W = depth.shape
    Ho, Wo = (int(v) for v in out_shape)
    assert corner_rays.shape == (H + 1, W + 1, 2) and centre_rays.shape == (H, W, 2)
    assert 1 <= max_footprint <= MAX_FOOTPRINT
    T = np.asarray(depth_to_output, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy = intrinsics(K_out)
    rec = dict.fromkeys(RECORD_FIELDS, 0)
    with np.errstate(all="ignore"):
        z = scaled_depth(depth, ratio)
        live = np.isfinite(z) & (z > 0)
        rec["valid"] = int(live.sum())
        q = _move(R, t, centre_rays[..., 0] * z, centre_rays[..., 1] * z, z)
        zf = q[2].astype(np.float32)
        front = (q[2] > 0) & np.isfinite(zf)
        corners = [corner_rays[:-1, :-1], corner_rays[:-1, 1:], corner_rays[1:, :-1], corner_rays[1:, 1:]]
        U, V = [], []
        back = np.zeros((H, W), bool)
        for c in corners:
            qc = _move(R, t, c[..., 0] * z, c[..., 1] * z, z)
            back |= qc[2] <= 0
            U.append(fx * (qc[0] / qc[2]) + cx)
            V.append(fy * (qc[1] / qc[2]) + cy)
        U, V = np.stack(U), np.stack(V)
        behind = live & (~front | back)
        rec["behind"] = int(behind.sum())
        go = live & ~behind
        bounds = [np.ceil(U.min(axis=0)), np.ceil(U.max(axis=0)), np.ceil(V.min(axis=0)), np.ceil(V.max(axis=0))]
        wild = ~np.all(np.isfinite(U) & np.isfinite(V), axis=0)
        for b in bounds:
            wild |= ~np.isfinite(b) | (b < -LIMIT) | (b > LIMIT)
        outside = go & wild
        go &= ~wild
        u0, u1, v0, v1 = (np.where(go, b, 0.0).astype(np.int64) for b in bounds)
        clipped = go & ((u1 - u0 > max_footprint) | (v1 - v0 > max_footprint))
        rec["clipped"] = int(clipped.sum())
        u1, v1 = np.minimum(u1, u0 + max_footprint), np.minimum(v1, v0 + max_footprint)
        empty = go & ((u0 >= u1) | (v0 >= v1))
        rec["empty"] = int(empty.sum())
        go &= ~empty
        off = go & ((u1 <= 0) | (v1 <= 0) | (u0 >= Wo) | (v0 >= Ho))
        rec["outside"] = int(outside.sum() + off.sum())
        go &= ~off
        rec["written"] = int(go.sum())
    zbuffer = np.full(Ho * Wo, EMPTY, np.uint32)
    bits = zf.view(np.uint32)
    for dj in range(max_footprint):
        for di in range(max_footprint):
            i, j = u0 + di, v0 + dj
            m = go & (i < u1) & (j < v1) & (i >= 0) & (i < Wo) & (j >= 0) & (j < Ho)
            np.minimum.at(zbuffer, (j[m] * Wo + i[m]), bits[m])
    zbuffer = zbuffer.reshape(Ho, Wo)
    filled = zbuffer != EMPTY
    rec["filled"] = int(filled.sum())
    keep = filled
    if colour_valid is not None:
        colour_valid = np.asarray(colour_valid)
        assert colour_valid.dtype == np.uint8 and colour_valid.shape == (Ho, Wo)
        rec["masked"] = int((filled & (colour_valid == 0)).sum())
        keep = filled & (colour_valid != 0)
    out = np.where(keep, zbuffer.view(np.float32), np.float32(0)).astype(np.float32)
    return out, rec


def rectify_colour(src, K_src, k_src, K_out, out_shape):
    """(dst uint8 (Ho, Wo, 3), valid uint8 (Ho, Wo)): the raw image resampled into the ideal camera K_out"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    Hs, Ws = src.shape[:2]
    Ho, Wo = (int(v) for v in out_shape)
    fxs, fys, cxs, cys = intrinsics(K_src)
    fxo, fyo, cxo, cyo = intrinsics(K_out)
    v, u = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        xd, yd = distort((u - cxo) / fxo, (v - cyo) / fyo, k_src)
        us, vs = fxs * xd + cxs, fys * yd + cys
        ok = np.isfinite(us) & np.isfinite(vs) & (us >= 0) & (us <= Ws - 1) & (vs >= 0) & (vs <= Hs - 1)
    us, vs = np.where(ok, us, 0.0), np.where(ok, vs, 0.0)
    fu, fv = np.floor(us), np.floor(vs)
    a, b = (us - fu)[..., None], (vs - fv)[..., None]
    u0, v0 = fu.astype(np.int64), fv.astype(np.int64)
    u1, v1 = np.minimum(u0 + 1, Ws - 1), np.minimum(v0 + 1, Hs - 1)
    s = src.astype(np.float64)
    top = s[v0, u0] * (1.0 - a) + s[v0, u1] * a
    bottom = s[v1, u0] * (1.0 - a) + s[v1, u1] * a
    value = np.floor((top * (1.0 - b) + bottom * b) + 0.5).astype(np.uint8)
    dst = np.where(ok[..., None], value, np.uint8(0)).astype(np.uint8)
    return dst, ok.astype(np.uint8)


def rotation(rotvec):
    """Rodrigues' matrix of a rotation vector, float64"""
    r = np.asarray(rotvec, dtype=np.float64)
    theta = float(np.linalg.norm(r))
    if theta == 0:
        return np.eye(3)
    n = r / theta
    N = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(n, n) + np.sin(theta) * N


def transform(rotvec=(0, 0, 0), t=(0, 0, 0)):
    """the 4 x 4 of q = R p + t"""
    T = np.eye(4)
    T[:3, :3] = rotation(rotvec)
    T[:3, 3] = np.asarray(t, dtype=np.float64)
    return T
