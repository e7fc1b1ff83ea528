"""A deforming analytic depth scene for the non-rigid fusion tests: one sphere in front of fusion_scene's back plane that
grows by 1.5 voxels of radius from frame 0 to frame 1, seen by fusion_scene's camera at the zero twist.  No rigid motion
explains the change, so a model that fuses frame 1 rigidly is pulled half-way to the larger sphere, and one that fuses
it through the warp field of a non-rigid registration is not.  Host numpy only."""
import functools

import numpy as np

import fusion_scene as S

K = S.K
WIDTH, HEIGHT = S.WIDTH, S.HEIGHT
CENTRE = (0.0, 0.0, 0.52)
RADII = (0.030, 0.036)  # metres, frame 0 and frame 1: 1.5 voxels apart
PLANE_Z = S.PLANE_Z
N = 32
VOXEL = 0.004
OFFSET = np.array([-16.0, -16.0, 112.0])
BAND = 10  # narrow_band_width_voxels
TWIST = np.zeros(6)
# HierarchicalOptimizer3d / oracle.HierarchicalOracle.  tikhonov_strength: the default 0.2 diverges in 3-D (the
# recursion g <- data - s laplace(g) has gain 12 s), 0.05 is tests/test_gpu_tsdf.py's
OPTIMIZER = dict(tikhonov_term_enabled=True, gradient_kernel_enabled=False, maximum_chunk_size=8, rate=0.3,
                 maximum_iteration_count=100, maximum_warp_update_threshold=0.001, tikhonov_strength=0.05)
COLOUR = (200, 90, 30)  # the constant colour image of the coloured run


def render(radius):
    """(HEIGHT, WIDTH) float32 depth in metres of the sphere of that radius and the plane, camera at the origin"""
    v, u = np.meshgrid(np.arange(HEIGHT, dtype=np.float64), np.arange(WIDTH, dtype=np.float64), indexing="ij")
    d = np.stack([(u - float(K[0, 2])) / float(K[0, 0]), (v - float(K[1, 2])) / float(K[1, 1]), np.ones_like(u)],
                 axis=-1)
    best = np.full(u.shape, PLANE_Z)  # the ray's z component is 1: the plane z = PLANE_Z is hit at s = PLANE_Z
    c = np.asarray(CENTRE)
    a = np.sum(d * d, axis=-1)
    b = d @ c
    disc = b * b - a * (c @ c - radius * radius)
    with np.errstate(invalid="ignore"):
        s = (b - np.sqrt(disc)) / a
    hit = (disc >= 0) & (s > 0)
    return np.where(hit, np.minimum(best, s), best).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frames():
    """the two depth images, read-only"""
    out = tuple(render(r) for r in RADII)
    for a in out:
        a.setflags(write=False)
    return out


def colour_image():
    return np.broadcast_to(np.array(COLOUR, np.uint8), (HEIGHT, WIDTH, 3)).copy()


def model_change(tsdf0, tsdf1):
    """the measure of the end-to-end test: the mean |tsdf after frame 1 - tsdf after frame 0| over the voxels whose
    frame-0 value has magnitude < 0.5"""
    t0, t1 = np.asarray(tsdf0, np.float64), np.asarray(tsdf1, np.float64)
    near = np.abs(t0) < 0.5
    assert np.count_nonzero(near) > 100
    return float(np.mean(np.abs(t1 - t0)[near]))
