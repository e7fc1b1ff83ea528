"""The analytic scene of tests/fusion_scene.py at a reduced image size, with one extra "ghost" sphere that a first
frame sees and a second does not: the transient object free-space carving removes from the model.  Host numpy only."""
import numpy as np

import fusion_scene as S
import rigid_restatement as R

SCALE = 4  # the images are 160 x 120
WIDTH, HEIGHT = S.WIDTH // SCALE, S.HEIGHT // SCALE
# the intrinsics of the image binned SCALE x SCALE: f / SCALE, (c + 0.5) / SCALE - 0.5
K = np.array([[S.K[0, 0] / SCALE, 0, (S.K[0, 2] + 0.5) / SCALE - 0.5],
              [0, S.K[1, 1] / SCALE, (S.K[1, 2] + 0.5) / SCALE - 0.5], [0, 0, 1]], dtype=np.float32)
GHOST_CENTRE, GHOST_RADIUS = np.array([0.06, 0.055, 0.50]), 0.025
N = 64  # the volume the ghost is placed in: N^3 at fusion_scene.offset(N)


def _rays():
    v, u = np.meshgrid(np.arange(HEIGHT, dtype=np.float64), np.arange(WIDTH, dtype=np.float64), indexing="ij")
    return np.stack([(u - float(K[0, 2])) / float(K[0, 0]), (v - float(K[1, 2])) / float(K[1, 1]),
                     np.ones_like(u)], axis=-1)


def sphere_depth(centre, radius, twist=None):
    """(HEIGHT, WIDTH) float64 depth of one world sphere seen from a camera at twist; inf where its ray misses"""
    m = R.matrix3d(np.zeros(6) if twist is None else np.asarray(twist, dtype=np.float64))
    cc = m[:3, :3] @ np.asarray(centre, dtype=np.float64) + m[:3, 3]
    d = _rays()
    a, b = np.sum(d * d, axis=-1), d @ cc
    disc = b * b - a * (cc @ cc - radius * radius)
    with np.errstate(invalid="ignore"):
        s = (b - np.sqrt(disc)) / a
    return np.where((disc >= 0) & (s > 0), s, np.inf)


def plain(twist=None):
    """frame B: the scene without the ghost, float32 metres"""
    return S.render(np.zeros(6) if twist is None else twist, width=WIDTH, height=HEIGHT, K_=K)


def with_ghost(twist=None):
    """frame A: the ghost composed into the scene by a per-pixel minimum, float32 metres"""
    base = plain(twist).astype(np.float64)
    ghost = sphere_depth(GHOST_CENTRE, GHOST_RADIUS, twist)
    return np.where(np.isfinite(ghost), np.minimum(np.where(base > 0, base, np.inf), ghost), base).astype(np.float32)


def voxel_points(n=N, voxel_size=0.004):
    """(n, n, n, 3) world (x, y, z) of the voxels of the n^3 volume at fusion_scene.offset(n)"""
    off = S.offset(n)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([(i + off[0]) * voxel_size, (j + off[1]) * voxel_size, (k + off[2]) * voxel_size], axis=-1)


def in_ghost(n=N, voxel_size=0.004):
    """the voxels strictly inside the ghost's ball"""
    return np.linalg.norm(voxel_points(n, voxel_size) - GHOST_CENTRE, axis=-1) < GHOST_RADIUS
