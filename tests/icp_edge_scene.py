"""A ragged, adversarial pair for the strided ICP (csrc/lsf_icp.hip: lsf_icp_run).  The image is 73 x 101: both extents
prime, so no stride above 1 and no 16 x 16 tile divides them, and StridedSource::store clips its NaN cell at the right
and at the bottom edge.  The prediction is the restated ray-cast of raycast_edge_scene's ball, with a floor and a wall
added (model_tsdf), under its `holes` weights, misses filled from a constant fallback: it carries "depth > 0 with a
zero normal" both at the filled pixels and at hits next to a hole.  The live frame is the same model with weights of
one, seen from a slightly different camera, with exact zeros, negative, NaN and +inf depths scattered into it.  ICP
starts from a third twist, so that live pixels project off themselves and some leave the image.  rejection_classes() sorts the live pixels into the
reasons a pair is refused without calling icp_restatement.associate.  Host numpy only."""
import numpy as np

import raycast_edge_scene as ES
import raycast_restatement as RC
from rigid_restatement import rodrigues

IMAGE = (73, 101)
K = np.array([[95.0, 0, 50.0], [0, 95.0, 36.0], [0, 0, 1]], np.float32)  # the ball camera's view, scaled to fill 73 x 101
CAMERA = "rx"
FALLBACK = 1.25          # metres: the constant the prediction's misses are filled from
DELTA = np.array([-0.004, 0.003, 0.002, -0.004, -0.006, -0.003])  # live twist minus prediction twist (m, rad)
# the estimate ICP starts from, minus the prediction twist: most of the way to the live twist, so that a live pixel
# projects about 0.8 pixel to the right of itself and the last columns leave the image
START = 0.8 * DELTA + np.array([0.0005, -0.0004, 0.0003, -0.0003, 0.0004, 0.0002])
# 0.12 voxel.  The surface is the zero level of a trilinear field on 0.25 m voxels and the two cameras cut it along
# different rays, so true pairs lie up to a few centimetres apart; at 0.03 m most pair and the rest are refused
MAX_DISTANCE = 0.03
STRIDES = (1, 2, 3, 4, 5, 7)
PYRAMID = ((2, 2, 3), (4, 2, 1))  # iterations and strides of the whole-pass case
LIVE_TYPES = ("float32", "float64", "uint16")
_CACHE = {}


def model_tsdf():
    """the ball of raycast_edge_scene with a floor (y > 4.7) and a wall (x > 9.2) added.  A sphere alone leaves the
    rotation about its centre free: A is then singular up to the volume's discretisation (condition number 1e6 and
    steps of 0.5 m were measured), and sums in another order move the twist by more than the tolerance"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in ES.BALL_SHAPE), indexing="ij")
    r = np.sqrt((x - 5.3) ** 2 + (y - 3.1) ** 2 + (z - 4.2) ** 2) - 2.4
    return np.clip(np.minimum(np.minimum(r, 4.7 - y), 9.2 - x) / 2.0, -1.0, 1.0).astype(np.float32)


def twist_p():
    return ES.ball_twist(CAMERA)


def start_twist():
    return twist_p() + START


def prediction():
    """(depth, normals) float32: restated ray-cast of ball / holes with normals, misses filled with FALLBACK"""
    if "prediction" not in _CACHE:
        fb = np.full(IMAGE, FALLBACK, np.float32)
        d, n, hits = RC.raycast(model_tsdf(), ES.ball_weight("holes"), K, twist_p(), ES.BALL_OFFSET, ES.VOXEL, IMAGE,
                                normals=True, fallback=fb)
        _CACHE["prediction"] = (d, n, hits)
    return _CACHE["prediction"][:2]


def prediction_hits():
    prediction()
    return _CACHE["prediction"][2]


def clean_live():
    """float32 metres: ball with weights of one from twist_p + DELTA, 0 where a ray misses"""
    if "clean" not in _CACHE:
        _CACHE["clean"] = RC.raycast(model_tsdf(), ES.ball_weight("ones"), K, twist_p() + DELTA, ES.BALL_OFFSET,
                                     ES.VOXEL, IMAGE)[0]
    return _CACHE["clean"]


def live(kind):
    """(image, ratio).  float32 (ratio 0.5) and float64 (ratio 1) carry 40 each of exact 0, negative, NaN and +inf at
    pixels that had a depth, the last row and column among them; uint16 (ratio 0.001) carries the zeros"""
    if kind not in _CACHE:
        clean = clean_live()
        rng = np.random.default_rng(5)
        rows, cols = np.nonzero(clean > 0)
        pick = rng.permutation(rows.size)[:160]
        bad = [0.0, -0.75, np.nan, np.inf]
        if kind == "uint16":
            image = np.round(clean.astype(np.float64) * 1000).astype(np.uint16)
            image[rows[pick[:40]], cols[pick[:40]]] = 0
            ratio = 0.001
        elif kind in ("float32", "float64"):
            image = (clean * np.float32(2)).astype(kind) if kind == "float32" else clean.astype(np.float64)
            for q, value in enumerate(bad):
                image[rows[pick[40 * q:40 * q + 40]], cols[pick[40 * q:40 * q + 40]]] = value
            image[-1, -1], image[-1, -2], image[-2, -1], image[0, -1], image[-1, 0] = np.nan, np.inf, -1.0, 0.0, np.inf
            ratio = 0.5 if kind == "float32" else 1.0
        else:
            raise ValueError(kind)
        _CACHE[kind] = (image, ratio)
    return _CACHE[kind]


def rejection_classes(image, ratio, twist, stride=1):
    """the live pixels (stride i, stride j) sorted by the first test of the contract they fail at `twist`: a dict of
    counts for "not_positive" (live depth not > 0, NaN counted), "behind" (q_z not > 0), "outside" (the projection
    leaves the image, or is NaN), "unusable_hole" (predicted depth not > 0), "zero_normal" (predicted depth > 0 with
    a zero normal), "far" (beyond MAX_DISTANCE, or a NaN distance) and "paired".  Written with matrices per pixel in a
    plain loop, not from icp_restatement.associate; it is a census, not a bit-exact restatement"""
    pd, pn = prediction()
    h, w = IMAGE
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    d = np.asarray(image)
    d = (d * np.float32(ratio)).astype(np.float64) if d.dtype == np.float32 else d.astype(np.float64) * float(ratio)
    tw = np.asarray(twist, np.float64)
    R, t = rodrigues(tw[3:]), tw[:3]
    Ep = RC.extrinsic(twist_p())
    Rp, tp = Ep[:, :3], Ep[:, 3]
    counts = dict.fromkeys(("not_positive", "behind", "outside", "unusable_hole", "zero_normal", "far", "paired"), 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for v in range(0, h, stride):
            for u in range(0, w, stride):
                depth = d[v, u]
                if not depth > 0.0:
                    counts["not_positive"] += 1
                    continue
                vertex = depth * np.array([(u - cx) / fx, (v - cy) / fy, 1.0])
                g = R.T @ (vertex - t)
                q = Rp @ g + tp
                if not q[2] > 0.0:
                    counts["behind"] += 1
                    continue
                pu, pv = np.rint(fx * q[0] / q[2] + cx), np.rint(fy * q[1] / q[2] + cy)
                if not (0.0 <= pu <= w - 1 and 0.0 <= pv <= h - 1):
                    counts["outside"] += 1
                    continue
                iu, iv = int(pu), int(pv)
                if not pd[iv, iu] > 0:
                    counts["unusable_hole"] += 1
                    continue
                if not pn[iv, iu].any():
                    counts["zero_normal"] += 1
                    continue
                D = float(pd[iv, iu])
                Vw = Rp.T @ (D * np.array([(iu - cx) / fx, (iv - cy) / fy, 1.0]) - tp)
                if not np.linalg.norm(g - Vw) <= MAX_DISTANCE:
                    counts["far"] += 1
                    continue
                counts["paired"] += 1
    return counts


def restated_iteration(kind, stride):
    """icp_restatement.iteration of live(kind) at start_twist(): (record, residual image, next twist), computed once"""
    import icp_restatement as I
    key = ("iteration", kind, stride)
    if key not in _CACHE:
        image, ratio = live(kind)
        pd, pn = prediction()
        with np.errstate(invalid="ignore"):  # the infinite depths
            _CACHE[key] = I.iteration(image, pd, pn, K, ratio, start_twist(), twist_p(), stride, MAX_DISTANCE)
    return _CACHE[key]


def restated_pass(kind):
    """icp_restatement.icp over PYRAMID from start_twist(): (records, final twist), computed once"""
    import icp_restatement as I
    key = ("pass", kind)
    if key not in _CACHE:
        image, ratio = live(kind)
        pd, pn = prediction()
        with np.errstate(invalid="ignore"):
            _CACHE[key] = I.icp(image, pd, pn, K, ratio, twist_p(), start_twist(), PYRAMID[0], PYRAMID[1],
                                MAX_DISTANCE)
    return _CACHE[key]
