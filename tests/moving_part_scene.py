"""The scene of the robust ICP tests: tests/fusion_scene.py's spheres and plane at tests/ghost_scene.py's 160 x 120 image
size, with one part that moves against the rest between the prediction and the live frame.  The prediction is the scene
at the zero twist with finite-difference normals (depth_pyramid_restatement.normals); the live frame is taken at half a
fusion_scene.STEP with SPHERES[1] displaced by MOVE.  The moved sphere's pairs sit inside ICP's 2 cm distance gate and
drag a least-squares pose; robust weights take them out.  Host numpy only."""
import functools

import numpy as np

import depth_pyramid_restatement as DP
import fusion_scene as S
import ghost_scene as G

K, WIDTH, HEIGHT = G.K, G.WIDTH, G.HEIGHT
SHAPE = (HEIGHT, WIDTH)
MOVED = 1  # the index of the sphere that moves
MOVE = np.array([0.008, 0.0, -0.008])  # its displacement in world coordinates, metres
TRUE_TWIST = 0.5 * S.STEP  # the live camera against the prediction's
ITERATIONS, STRIDES = (4, 4, 6), (4, 2, 1)
# the scales of the tests, metres: Huber's k and Tukey's c
HUBER_SCALE, TUKEY_SCALE = 0.001, 0.003


def intrinsics():
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def render(twist, moved=True, width=WIDTH, height=HEIGHT, K_=K):
    """(height, width) float32 depth in metres of the scene seen from a camera at twist, with the moved sphere displaced
    by MOVE (moved=True) or in place: fusion_scene.render of the changed sphere list"""
    spheres = list(S.SPHERES)
    if moved:
        c, r = spheres[MOVED]
        spheres[MOVED] = (tuple(np.asarray(c) + MOVE), r)
    keep = S.SPHERES
    S.SPHERES = tuple(spheres)
    try:
        return S.render(twist, width=width, height=height, K_=K_)
    finally:
        S.SPHERES = keep


@functools.lru_cache(maxsize=None)
def prediction():
    """(depth (H, W), normals (H, W, 3)) float32 of the undisturbed scene at the zero twist, in the ray-caster's
    formats: the normals are the forward differences of the depth, 0 at the last row and column and across a depth
    step.  Nothing modifies them"""
    depth = render(np.zeros(6), moved=False)
    normals = DP.normals(depth, intrinsics())
    depth.setflags(write=False)
    normals.setflags(write=False)
    return depth, normals


@functools.lru_cache(maxsize=None)
def live(moved=True):
    """the live frame at TRUE_TWIST, float32 metres"""
    depth = render(TRUE_TWIST, moved=moved)
    depth.setflags(write=False)
    return depth


def changed_pixels():
    """the pixels of the live frame that the moved sphere changes"""
    return int((live(True) != live(False)).sum())


def sequence_frames(count=3, width=WIDTH, height=HEIGHT, K_=K):
    """frame k at fusion_scene.true_twist(k); frame 0 undisturbed, every later frame with the sphere displaced"""
    return [render(S.true_twist(k), moved=k > 0, width=width, height=height, K_=K_) for k in range(count)]


def pose_error(twist, truth=None):
    """(translation error in metres, rotation error in radians) of a twist against the true one: the norms of the two
    halves of the difference"""
    d = np.asarray(twist, np.float64).reshape(6) - (TRUE_TWIST if truth is None else np.asarray(truth, np.float64))
    return float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:]))
