"""The analytic scene of tests/fusion_scene.py as a depth sensor would see it: seeded axial noise of standard deviation
sigma(z) = 0.0012 + 0.0019 (z - 0.4)^2 metres (a structured-light sensor's axial model), then quantised to uint16
millimetres (depth_unit_ratio 0.001).  Pixels without a hit stay 0.  Generated from a seed: no fixture is stored.
Host numpy only."""
import numpy as np

import fusion_scene as S

RATIO = 0.001


def sigma(z):
    return 0.0012 + 0.0019 * (z - 0.4) ** 2


def render(twist, seed, **kw):
    """(height, width) uint16 depth in millimetres of the scene from a camera at twist"""
    z = S.render(twist, **kw).astype(np.float64)
    rng = np.random.default_rng(seed)
    noisy = z + rng.standard_normal(z.shape) * sigma(z)
    return np.where(z > 0, np.clip(np.rint(noisy / RATIO), 1, 65535), 0).astype(np.uint16)


def frames(count, step=S.STEP, seed=0, **kw):
    """frames 0 .. count - 1 at the true twists k * step, frame k seeded with seed + k"""
    return [render(k * np.asarray(step), seed + k, **kw) for k in range(count)]
