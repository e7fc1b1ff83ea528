"""colour_scene's painted spheres and plane seen by an RGB-D rig: a colour camera with fusion_scene's matrix at 640 x 480
behind a lens with distortion, following fusion_scene.true_twist(k), and a depth camera of 512 x 384 with a barrel lens,
3 cm to its side and turned by 0.02 rad.  Both RAW images are rendered analytically along the distorted pixels' rays (the
undistortion for that is iterated to convergence here, far beyond the kernels' ten steps).  Also what the CPU and the GPU
tests share: the frames registered and rectified by rgbd_restatement, and the four of them fused by the existing
restatements into colour_scene's 64^3 volume.  Host numpy only."""
import functools

import numpy as np

import colour_restatement as C
import colour_scene as CS
import fusion_restatement as F
import fusion_scene as S
import mesh_restatement as M
import rgbd_restatement as G
import rigid_restatement as R

COLOUR_K = S.K
COLOUR_SHAPE = (S.HEIGHT, S.WIDTH)
COLOUR_COEFFS = (0.12, -0.2, 0.0008, -0.0006, 0.05)
DEPTH_K = np.array([[560.0, 0, 255.5], [0, 560.0, 191.5], [0, 0, 1]])
DEPTH_SHAPE = (384, 512)
DEPTH_COEFFS = G.BARREL
DEPTH_TO_COLOUR = G.transform((0.0, 0.02, 0.0), (0.03, 0.0, 0.002))
MAX_FOOTPRINT = 8


class Camera:
    """the least a camera of fusion.RgbdSensor carries"""

    class Intrinsics:
        def __init__(self, matrix, coeffs):
            self.intrinsic_matrix = matrix
            if coeffs is not None:
                self.distortion_coeffs = np.asarray(coeffs, dtype=np.float64)

    def __init__(self, matrix, coeffs=None, depth_unit_ratio=None):
        self.intrinsics = Camera.Intrinsics(matrix, coeffs)
        if depth_unit_ratio is not None:
            self.depth_unit_ratio = depth_unit_ratio


def cameras():
    """(depth camera, colour camera) of the rig; the raw depth is float32 in metres"""
    return Camera(DEPTH_K, DEPTH_COEFFS, 1.0), Camera(COLOUR_K, COLOUR_COEFFS)


def pixel_rays(shape, K, k):
    """(x, y) float64 (H, W): the undistorted normalised coordinates of the raw pixels, to convergence"""
    fx, fy, cx, cy = G.intrinsics(K)
    v, u = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    return G.undistort((u - cx) / fx, (v - cy) / fy, k, iterations=60)


def render_rays(pose, x, y):
    """(depth float32 in metres, surface int8) along the rays (x, y, 1) of a camera whose world-to-camera matrix is
    pose: colour_scene.render's expressions with the rays given"""
    rot, t = pose[:3, :3], pose[:3, 3]
    d = np.stack([x, y, np.ones_like(x)], axis=-1)
    best = np.full(x.shape, np.inf)
    surface = np.full(x.shape, -1, np.int8)
    normal = rot @ np.array([0.0, 0.0, 1.0])
    p0 = rot @ np.array([0.0, 0.0, S.PLANE_Z]) + t
    denom = d @ normal
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(np.abs(denom) > 1e-12, (p0 @ normal) / denom, np.inf)
    nearer = (s > 0) & (s < best)
    best, surface = np.where(nearer, s, best), np.where(nearer, np.int8(CS.PLANE), surface)
    for j, (c, r) in enumerate(S.SPHERES):
        cc = rot @ np.asarray(c) + t
        a = np.sum(d * d, axis=-1)
        b = d @ cc
        disc = b * b - a * (cc @ cc - r * r)
        with np.errstate(invalid="ignore"):
            s = (b - np.sqrt(disc)) / a
        nearer = (disc >= 0) & (s > 0) & (s < best)
        best, surface = np.where(nearer, s, best), np.where(nearer, np.int8(j), surface)
    hit = np.isfinite(best)
    return np.where(hit, best, 0.0).astype(np.float32), np.where(hit, surface, np.int8(-1))


@functools.lru_cache(maxsize=None)
def raw_frames():
    """FRAMES x (raw depth float32 (384, 512) in metres, raw colour uint8 (480, 640, 3)); nothing modifies them"""
    xd, yd = pixel_rays(DEPTH_SHAPE, DEPTH_K, DEPTH_COEFFS)
    xc, yc = pixel_rays(COLOUR_SHAPE, COLOUR_K, COLOUR_COEFFS)
    out = []
    for k in range(CS.FRAMES):
        colour_pose = R.matrix3d(np.asarray(S.true_twist(k), dtype=np.float64))
        depth_pose = np.linalg.inv(DEPTH_TO_COLOUR) @ colour_pose
        depth, _ = render_rays(depth_pose, xd, yd)
        _, surface = render_rays(colour_pose, xc, yc)
        image = np.where((surface >= 0)[..., None], CS.COLOURS[np.maximum(surface, 0)], CS.BACKGROUND).astype(np.uint8)
        pair = (depth, np.ascontiguousarray(image))
        for a in pair:
            a.setflags(write=False)
        out.append(pair)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ray_tables():
    """the depth camera's (corner_rays, centre_rays), restated"""
    tables = G.ray_table(*DEPTH_SHAPE, DEPTH_K, DEPTH_COEFFS)
    for a in tables:
        a.setflags(write=False)
    return tables


@functools.lru_cache(maxsize=None)
def restated_registration():
    """FRAMES x (depth_m float32 (480, 640), colour uint8 (480, 640, 3), colour_valid uint8, record): the raw pairs
    registered into the rectified colour camera by rgbd_restatement"""
    corner, centre = ray_tables()
    out = []
    for depth, image in raw_frames():
        colour, valid = G.rectify_colour(image, COLOUR_K, COLOUR_COEFFS, COLOUR_K, COLOUR_SHAPE)
        depth_m, record = G.register_depth(depth, 1.0, corner, centre, DEPTH_TO_COLOUR, COLOUR_K, COLOUR_SHAPE,
                                           MAX_FOOTPRINT, valid)
        for a in (depth_m, colour, valid):
            a.setflags(write=False)
        out.append((depth_m, colour, valid, record))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def restated_model():
    """(tsdf, weight, colour, (vertices, faces, vertex colours)) of the registered frames fused at their true twists
    into colour_scene's empty 64^3 volume with COLOUR_BAND, all by the existing restatements"""
    off = CS.offset()
    t, w = F.empty_model((CS.N,) * 3)
    c = np.zeros((CS.N,) * 3 + (4,), np.float32)
    for k, (depth_m, colour, _, _) in enumerate(restated_registration()):
        t, w, c, _ = C.fuse_depth_colour(t, w, c, depth_m, colour, COLOUR_K, 1.0, off, S.true_twist(k),
                                         colour_band=CS.COLOUR_BAND)
    verts, faces = M.extract(t, w, off, CS.VOXEL)[:2]
    colours = C.vertex_colours(t, w, c)
    for a in (t, w, c, verts, faces, colours):
        a.setflags(write=False)
    return t, w, c, (verts, faces, colours)
