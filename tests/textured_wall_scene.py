"""An analytic textured wall for the photometric tracking tests: the world plane z = PLANE_Z painted by world position
with three smooth channels.  Its geometry constrains t_z, r_x and r_y only (t_x, t_y and r_z leave the point-to-plane A
singular); the texture constrains the rest.

Pose convention, fusion_scene's: a camera at twist xi sees the world point X at R X + t, (R, t) =
twist_vector_to_matrix3d(xi).  Pixel (u, v) is the ray s ((u - cx) / fx, (v - cy) / fy, 1) and its depth the s of the
hit.  The colour of a pixel is the paint at its hit point, rint(255 c) per channel as uint8.  Host numpy only."""
import numpy as np

import rigid_restatement as R

PLANE_Z = 0.6
# the camera of the kernel tests: 152 x 120 pixels, both a multiple of 8 and neither of 16
K_SMALL = np.array([[175.0, 0, 76], [0, 175.0, 60], [0, 0, 1]], dtype=np.float32)
SHAPE_SMALL = (120, 152)
# the live frame of the kernel tests, seen against the prediction at the zero twist
MOTION = np.array([0.003, -0.002, 0.002, 0.01, -0.012, 0.008])


def paint(X, Y):
    """(..., 3) float64 in 0..1: the wall's R, G, B at the world position (X, Y)"""
    tau = 2.0 * np.pi
    r = 0.5 + 0.25 * np.sin(tau * X / 0.08) + 0.2 * np.sin(tau * Y / 0.06 + 1.0)
    g = 0.5 + 0.25 * np.sin(tau * (X + Y) / 0.07 + 0.5) + 0.2 * np.cos(tau * (X - Y) / 0.09)
    b = 0.5 + 0.3 * np.sin(tau * X / 0.05 + 2.0) * np.sin(tau * Y / 0.065)
    return np.stack([r, g, b], axis=-1)


def render(twist, K, shape):
    """(depth float32 (H, W) in metres, colour uint8 (H, W, 3), normal float64 (3,)) of the wall seen from a camera at
    twist.  The normal is the plane's in camera coordinates, towards the camera, as the ray-caster's normals point"""
    m = R.matrix3d(np.asarray(twist, dtype=np.float64))
    rot, t = m[:3, :3], m[:3, 3]
    h, w = int(shape[0]), int(shape[1])
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(u - float(K[0, 2])) / float(K[0, 0]), (v - float(K[1, 2])) / float(K[1, 1]), np.ones_like(u)],
                 axis=-1)
    normal = rot @ np.array([0.0, 0.0, 1.0])
    p0 = rot @ np.array([0.0, 0.0, PLANE_Z]) + t
    s = (p0 @ normal) / (d @ normal)
    assert np.all(s > 0)  # the tests' cameras face the wall
    world = (s[..., None] * d - t) @ rot  # R^T (s d - t)
    image = np.rint(255.0 * paint(world[..., 0], world[..., 1])).astype(np.uint8)
    return s.astype(np.float32), np.ascontiguousarray(image), -normal


def luminance(rgb):
    """Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 in float64 of R, G, B in units of the 8-bit image"""
    rgb = np.asarray(rgb, dtype=np.float64)
    return ((0.299 * rgb[..., 0] + 0.587 * rgb[..., 1]) + 0.114 * rgb[..., 2]) / 255.0


def prediction(twist, K, shape):
    """the analytic prediction at twist, in the ray-caster's formats: (depth (H, W), normals (H, W, 3), colour
    (H, W, 4)) float32, the colour (R, G, B, Y) of the render's own bytes"""
    depth, image, normal = render(twist, K, shape)
    normals = np.broadcast_to(normal.astype(np.float32), depth.shape + (3,)).copy()
    colour = np.empty(depth.shape + (4,), np.float32)
    colour[..., :3] = image
    colour[..., 3] = luminance(image).astype(np.float32)
    return depth, normals, colour


def live_depth(depth, dtype):
    """a float32 metre depth image in a live dtype, and its depth_unit_ratio"""
    if dtype == np.uint16:
        return np.round(depth * 5000).astype(np.uint16), 1.0 / 5000
    if dtype == np.float32:
        return depth * np.float32(2), 0.5
    return depth.astype(np.float64), 1.0
