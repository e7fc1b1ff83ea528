"""An analytic depth scene for the fusion tests: three spheres in front of a back plane, ray-cast exactly into float32
depth images in metres for a camera at a given twist.  The curved surfaces constrain all six degrees of freedom, which
a single flat wall does not (t_x, t_y and r_z leave A singular).

Pose convention, the generator's: the live volume of a frame taken at twist xi is generated
under E = twist_vector_to_matrix3d(xi), which maps a point X of the canonical (world) frame to camera coordinates
R X + t.  The camera of frame k therefore sees the world sphere (c, r) as the sphere (R c + t, r) and the world plane
z = PLANE_Z as the plane through R (0, 0, PLANE_Z) + t with normal R (0, 0, 1).  A pixel (u, v) is the ray
s ((u - cx) / fx, (v - cy) / fy, 1), and its depth is the z of the nearest hit, s.  Host numpy only."""
import numpy as np

import rigid_restatement as R

K = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
WIDTH, HEIGHT = 640, 480
PLANE_Z = 0.62
SPHERES = (((0.0, 0.0, 0.55), 0.05), ((-0.06, 0.045, 0.50), 0.035), ((0.055, -0.05, 0.52), 0.04))
# per frame: about one 4 mm voxel of translation and one degree of rotation
STEP = np.array([0.003, -0.002, 0.002, 0.01, -0.012, 0.008])


def offset(n):
    """array offset (voxels) of an n^3 volume of 4 mm voxels around the spheres and the plane"""
    return np.array([-n / 2, -n / 2, 0.43 / 0.004 + (64 - n) / 4], dtype=np.float64)


def true_twist(k):
    return k * STEP


def render(twist, width=WIDTH, height=HEIGHT, K_=K):
    """(height, width) float32 depth in metres of the scene seen from a camera at twist; 0 where nothing is hit"""
    m = R.matrix3d(np.asarray(twist, dtype=np.float64))
    rot, t = m[:3, :3], m[:3, 3]
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    d = np.stack([(u - float(K_[0, 2])) / float(K_[0, 0]), (v - float(K_[1, 2])) / float(K_[1, 1]),
                  np.ones_like(u)], axis=-1)
    best = np.full(u.shape, np.inf)
    normal = rot @ np.array([0.0, 0.0, 1.0])
    p0 = rot @ np.array([0.0, 0.0, PLANE_Z]) + t
    denom = d @ normal
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(np.abs(denom) > 1e-12, (p0 @ normal) / denom, np.inf)
    best = np.where(s > 0, np.minimum(best, s), best)
    for c, r in SPHERES:
        cc = rot @ np.asarray(c) + t
        a = np.sum(d * d, axis=-1)
        b = d @ cc
        disc = b * b - a * (cc @ cc - r * r)
        with np.errstate(invalid="ignore"):
            s = (b - np.sqrt(disc)) / a
        hit = (disc >= 0) & (s > 0)
        best = np.where(hit, np.minimum(best, s), best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def frames(count, **kw):
    return [render(true_twist(k), **kw) for k in range(count)]
