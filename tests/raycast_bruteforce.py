"""An unclipped ray march through the canonical TSDF, written from the "Ray-casting" bullets of INTEGRATION.md section 3
and from nothing else: the independent reference for the depth image and the hit count of csrc/lsf_raycast.hip.  The
kernel and tests/raycast_restatement.py clip every ray to the volume's box (lo, hi, a first and a last step, a step cap)
and the contract promises that "the clip only decides where a lane starts and stops".  Here there is no clip: every pixel
visits every sample m = 1 .. M, M taken from the farthest corner of the box, and applies the validity test, the
trilinear value and the hit rule as the contract words them.  Every step is one float64 IEEE operation in the order
the contract writes it.  The camera matrix is raycast_restatement.extrinsic, pinned separately against
rigid3d_restatement.  Host numpy only: no package import."""
import math

import numpy as np

from raycast_restatement import extrinsic

__all__ = ["STEP_DIVISOR", "ray", "steps", "sample", "trace", "march"]

STEP_DIVISOR = 2  # step = voxel_size / 2


def ray(K, twist, offset, voxel_size, image_shape):
    """(a, b, R): per axis j (x, y, z) the (H, W) float64 arrays of g(s) = a + s b, and the camera's rotation"""
    h, w = int(image_shape[0]), int(image_shape[1])
    K = np.asarray(K)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    off = np.asarray(offset, np.float64).reshape(3)
    vs = float(voxel_size)
    E = extrinsic(twist)
    R, t = E[:, :3], E[:, 3]
    u = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    v = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    dc0, dc1 = (u - cx) / fx, (v - cy) / fy
    a, b = [], []
    for j in range(3):
        o = -((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2])
        d = (R[0, j] * dc0 + R[1, j] * dc1) + R[2, j] * 1.0
        a.append(np.full((h, w), o / vs - off[j]))
        b.append(d / vs)
    return a, b, R


def steps(shape, twist, offset, voxel_size):
    """M: ceil(z_max / step) + 3 for the largest camera z of the box's eight corners, 1 when that is not positive.
    No valid sample lies beyond z_max, the samples being at camera z = m * step"""
    nz, ny, nx = shape
    E = extrinsic(twist)
    off = np.asarray(offset, np.float64).reshape(3)
    vs = float(voxel_size)
    z_max = -math.inf
    for cx in (0.0, float(nx - 1)):
        for cy in (0.0, float(ny - 1)):
            for cz in (0.0, float(nz - 1)):
                world = [(cx + off[0]) * vs, (cy + off[1]) * vs, (cz + off[2]) * vs]
                z_max = max(z_max, E[2, 0] * world[0] + E[2, 1] * world[1] + E[2, 2] * world[2] + E[2, 3])
    return int(math.ceil(z_max / (vs / STEP_DIVISOR))) + 3 if z_max > 0.0 else 1


def sample(tsdf, weight, g):
    """(inside, valid, value) at voxel coordinates g = [gx, gy, gz], arrays of one shape.  inside: 0 <= g_j < n_j - 1 on
    every axis; valid: inside and all 8 corner weights > 0; value: the trilinear value where inside, along x for the
    four (z, y) pairs, then y, then z"""
    nz, ny, nx = tsdf.shape
    gx, gy, gz = g
    with np.errstate(invalid="ignore"):
        inside = (gx >= 0.0) & (gx < float(nx - 1)) & (gy >= 0.0) & (gy < float(ny - 1)) & (gz >= 0.0) & \
            (gz < float(nz - 1))
    gx, gy, gz = np.where(inside, gx, 0.0), np.where(inside, gy, 0.0), np.where(inside, gz, 0.0)
    x0, y0, z0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64), np.floor(gz).astype(np.int64)
    fx, fy, fz = gx - x0, gy - y0, gz - z0
    hx, hy, hz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    valid = inside.copy()
    with np.errstate(invalid="ignore"):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    valid &= weight[z0 + dz, y0 + dy, x0 + dx] > 0
    t = tsdf.astype(np.float64)
    with np.errstate(invalid="ignore"):
        c00 = t[z0, y0, x0] * hx + t[z0, y0, x0 + 1] * fx
        c01 = t[z0, y0 + 1, x0] * hx + t[z0, y0 + 1, x0 + 1] * fx
        c10 = t[z0 + 1, y0, x0] * hx + t[z0 + 1, y0, x0 + 1] * fx
        c11 = t[z0 + 1, y0 + 1, x0] * hx + t[z0 + 1, y0 + 1, x0 + 1] * fx
        c0 = c00 * hy + c01 * fy
        c1 = c10 * hy + c11 * fy
        value = c0 * hz + c1 * fz
    return inside, valid, value


def trace(tsdf, weight, K, twist, offset, voxel_size, image_shape):
    """every sample of every pixel: (inside, valid, value), each (M + 1, H, W) with row m the sample at s = m * step.
    Row 0 is no sample (the march starts at m = 1) and is all False / 0"""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    a, b, _ = ray(K, twist, offset, voxel_size, image_shape)
    M = steps(tsdf.shape, twist, offset, voxel_size)
    step = float(voxel_size) / STEP_DIVISOR
    h, w = a[0].shape
    inside, valid, value = np.zeros((M + 1, h, w), bool), np.zeros((M + 1, h, w), bool), np.zeros((M + 1, h, w))
    for m in range(1, M + 1):
        s = float(m) * step
        inside[m], valid[m], value[m] = sample(tsdf, weight, [a[j] + s * b[j] for j in range(3)])
    return inside, valid, value


def march(tsdf, weight, K, twist, offset, voxel_size, image_shape):
    """(depth (H, W) float32, hit (H, W) bool, s_hit (H, W) float64, index (H, W) int64): the depth is 0 and s_hit NaN
    where a pixel has no hit; index is the m of a pixel's hit, else of its last valid sample, else 0"""
    _, valid, value = trace(tsdf, weight, K, twist, offset, voxel_size, image_shape)
    step = float(voxel_size) / STEP_DIVISOR
    shape = valid.shape[1:]
    hit = np.zeros(shape, bool)
    s_hit = np.full(shape, np.nan)
    index = np.zeros(shape, np.int64)
    for m in range(1, valid.shape[0]):
        p, c = value[m - 1], value[m]
        with np.errstate(invalid="ignore", divide="ignore"):
            crossing = ~hit & valid[m - 1] & (p > 0.0) & valid[m] & (c <= 0.0)
            s = float(m - 1) * step + step * (p / (p - c))
        s_hit[crossing] = s[crossing]
        index[~hit & valid[m]] = m
        hit |= crossing
    depth = np.where(hit, s_hit, 0.0).astype(np.float32)
    return depth, hit, s_hit, index
