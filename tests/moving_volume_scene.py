"""An analytic depth scene for the moving-volume tests, in the manner of tests/fusion_scene.py: a back plane and a row of
spheres along x that is longer than one window, seen by a camera that translates along x with a little y and a small
rotation.  With the window and the policy below the anchor crosses the threshold several times, and the camera ends
where it sees nothing of the window's first position.  Pose convention: fusion_scene's.  Host numpy only."""
import numpy as np

import rigid_restatement as R

WIDTH, HEIGHT = 160, 120
K = np.array([[400.0, 0, 80], [0, 400.0, 60], [0, 0, 1]], dtype=np.float32)
PLANE_Z = 0.62
# centres 9 cm apart from x = -0.10 to 0.53 m, alternating in y and z so that no translation maps the row onto itself
SPHERES = tuple(((-0.10 + 0.09 * i, 0.025 * (-1) ** i, 0.54 + 0.015 * ((i % 3) - 1)), 0.035) for i in range(8))
# per frame: the camera moves 6 mm (1.5 voxels) along +x and 1 mm along +y (t = -R c) and turns a little
STEP = np.array([-0.006, -0.001, 0.0, 0.0004, 0.001, 0.0003])
FRAMES = 45

VOXEL = 0.004
BAND = 5                 # narrow band, voxels
WINDOW = 48              # the window: 48^3 voxels, a 19.2 cm cube
ANCHOR = (0.0, 0.0, 0.56)
THRESHOLD = 6.0
WINDOW_OFFSET = np.array([-WINDOW / 2, -WINDOW / 2, ANCHOR[2] / VOXEL - WINDOW / 2], dtype=np.float64)


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


def paint(depth, twist, K_=K):
    """a uint8 (H, W, 3) colour image registered to `depth`: stripes in the WORLD x, y and z of each pixel's point, so
    the colour belongs to the surface and not to the camera; black where the depth is 0"""
    m = R.matrix3d(np.asarray(twist, dtype=np.float64))
    rot, t = m[:3, :3], m[:3, 3]
    h, w = depth.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = depth.astype(np.float64)
    cam = np.stack([(u - float(K_[0, 2])) / float(K_[0, 0]) * z, (v - float(K_[1, 2])) / float(K_[1, 1]) * z, z], -1)
    world = (cam - t) @ rot  # R^T (X - t)
    image = np.stack([127.5 + 127.5 * np.sin(world[..., j] * f) for j, f in enumerate((90.0, 70.0, 50.0))], -1)
    return np.where((z > 0)[..., None], np.floor(image), 0).astype(np.uint8)


def frames(count=FRAMES):
    return [render(true_twist(k)) for k in range(count)]
