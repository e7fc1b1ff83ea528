"""CPU checks of robust ICP: the restatement's own properties (tests/robust_icp_restatement.py) -- the weights at their
edges, an infinite scale against icp_restatement, the pose it recovers on tests/moving_part_scene.py --, the ctypes
layout of the two parameter structs, the header's macros, the exports, and the refusal of bad arguments by both C entry
points and by the Python interfaces."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import depth_pyramid_restatement as DP
import icp_restatement as I
import moving_part_scene as M
import robust_icp_restatement as RR
import test_pyramid_photometric_host as PH
from conftest import ROOT

HUBER, TUKEY = RR.Loss("huber", M.HUBER_SCALE), RR.Loss("tukey", M.TUKEY_SCALE)
# the least factors by which a loss must shrink least squares' pose error on the moving-part scene, in translation and
# in rotation.  The restatement reaches 76 and 37 (tukey), 5.3 and 3.7 (huber); profiles/robust_icp_cost.md has the table
TUKEY_FACTOR, HUBER_FACTOR = 10.0, 3.0


@functools.lru_cache(maxsize=None)
def restated_errors():
    """{name: (translation error, rotation error)} of the final pose of the whole run (iterations (4, 4, 6), strides
    (4, 2, 1)) on the moving-part scene, for least squares and both losses, and for least squares without the move"""
    pd, pn = M.prediction()
    out = {}
    for name, loss, moved in (("least squares", None, True), ("huber", HUBER, True), ("tukey", TUKEY, True),
                              ("undisturbed", None, False)):
        if loss is None:
            _, twist = I.icp(M.live(moved), pd, pn, M.K, 1.0, np.zeros(6), None, M.ITERATIONS, M.STRIDES)
        else:
            _, twist, _, _, _ = RR.icp(loss, M.live(moved), pd, pn, M.K, 1.0, np.zeros(6), None, M.ITERATIONS, M.STRIDES)
        out[name] = M.pose_error(twist)
    return out


def test_weights_at_their_edges():
    s = 0.003
    below, above = np.nextafter(s, 0.0), np.nextafter(s, 1.0)
    r = np.array([0.0, below, -below, s, -s, above, -above, 2 * s])
    w, out = RR.weight("huber", r, s)
    assert np.array_equal(w[:5], np.ones(5)) and np.array_equal(w[5:], [s / above, s / above, s / (2 * s)])
    assert list(out) == [False] * 5 + [True] * 3
    w, out = RR.weight("tukey", r, s)
    u = 1.0 - (below / s) * (below / s)
    assert w[0] == 1.0 and w[1] == w[2] == u * u and np.array_equal(w[3:], np.zeros(5))
    assert list(out) == [False] * 3 + [True] * 5
    for kind in ("huber", "tukey"):  # an infinite scale: exactly 1.0, never an outlier
        w, out = RR.weight(kind, np.array([0.0, 1e-300, -0.02, 1e300]), np.inf)
        assert np.array_equal(w, np.ones(4)) and not out.any()
    with pytest.raises(ValueError):
        RR.weight("cauchy", r, s)


@pytest.mark.parametrize("kind", ["huber", "tukey"])
def test_an_infinite_scale_is_the_plain_iteration(kind):
    """array for array: the strided form at stride 2, and one gated pyramid level"""
    pd, pn = M.prediction()
    start = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015])
    loss = RR.Loss(kind, np.inf)
    levels = DP.pyramid(M.live(), 1.0, M.K, levels=2)
    cases = (((M.live(), pd, pn, M.K, 1.0, start, np.zeros(6), 2), {}),
             ((levels[0][1], pd, pn, M.K, 1.0, start, np.zeros(6), 1, I.MAX_DISTANCE, levels[2][1], levels[1][1],
               DP.cos_of(math.radians(20.0))), {}))
    for args, kw in cases:
        want, want_res, want_twist = I.iteration(*args, **kw)
        got, res, weights, twist = RR.iteration(loss, *args, **kw)
        for key, value in want.items():
            assert np.array_equal(got[key], value), key
        assert want["count"] > 1000 and got["weight_sum"] == want["count"] and got["outliers"] == 0
        assert np.array_equal(res.view(np.uint32), want_res.view(np.uint32)) and np.array_equal(twist, want_twist)
        assert np.array_equal(weights[np.isfinite(res)], np.ones(want["count"], np.float32))
        assert np.isnan(weights[~np.isfinite(res)]).all()
    assert got["angle_rejected"] > 0


def test_a_pair_with_weight_zero_still_counts():
    pd, pn = M.prediction()
    plain, _, _ = I.iteration(M.live(), pd, pn, M.K, 1.0, np.zeros(6), np.zeros(6))
    got, res, weights, twist = RR.iteration(RR.Loss("tukey", 1e-9), M.live(), pd, pn, M.K, 1.0, np.zeros(6),
                                            np.zeros(6))
    assert got["count"] == plain["count"] and np.isfinite(res).sum() == plain["count"]
    assert got["outliers"] > 0.99 * got["count"] and got["weight_sum"] < 0.01 * got["count"]
    assert got["skipped"] == 1 and np.array_equal(twist, np.zeros(6))


def test_the_losses_recover_the_pose_of_the_moving_part_scene(capsys):
    """547 of 19200 pixels move; least squares loses 3 mm and 2 degrees to them.  Tukey at 3 mm must cut both errors
    to a tenth at the most, Huber at 1 mm to a third"""
    err = restated_errors()
    with capsys.disabled():
        print("\nmoving-part scene, |t error| (m) and |r error| (rad):", {k: (float("%.3g" % a), float("%.3g" % b))
                                                                         for k, (a, b) in err.items()})
    assert M.changed_pixels() == 547
    ls = err["least squares"]
    assert ls[0] > 2e-3 and ls[1] > 2e-2  # the problem is there
    for name, factor in (("tukey", TUKEY_FACTOR), ("huber", HUBER_FACTOR)):
        assert err[name][0] * factor <= ls[0] and err[name][1] * factor <= ls[1], (name, err[name], ls)
    assert err["tukey"][0] <= 2 * err["undisturbed"][0]


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p, q = lib.IcpRobustParams, lib.IcpPyramidRobustParams
    assert [f[0] for f in p._fields_] == [f[0] for f in lib.IcpPhotometricParams._fields_] + \
        ["loss", "scale", "intensity_scale"]
    assert [f[0] for f in q._fields_] == [f[0] for f in lib.IcpPyramidPhotometricParams._fields_] + \
        ["loss", "scale", "intensity_scale"]
    assert ctypes.sizeof(lib.IcpPhotometricParams) == 160 and ctypes.sizeof(p) == 184
    assert (p.loss.offset, p.scale.offset, p.intensity_scale.offset) == (160, 168, 176)
    assert ctypes.sizeof(lib.IcpPyramidPhotometricParams) == 152 and ctypes.sizeof(q) == 176
    assert (q.loss.offset, q.scale.offset, q.intensity_scale.offset) == (152, 160, 168)
    for name, _ in lib.IcpPhotometricParams._fields_:
        assert getattr(p, name).offset == getattr(lib.IcpPhotometricParams, name).offset
    for name, _ in lib.IcpPyramidPhotometricParams._fields_:
        assert getattr(q, name).offset == getattr(lib.IcpPyramidPhotometricParams, name).offset
    assert (lib.ICP_LOSS_HUBER, lib.ICP_LOSS_TUKEY) == (1, 2)
    assert lib.ICP_ROBUST_SCRATCH_BYTES == 2 * 256 * 34 * 8 and lib.ICP_PYRAMID_ROBUST_SCRATCH_BYTES == 2 * 256 * 35 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for text in ("#define LSF_ICP_LOSS_HUBER 1", "#define LSF_ICP_LOSS_TUKEY 2", "#define LSF_ICP_RECORD_DOUBLES 64",
                 "#define LSF_ICP_ROBUST_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 34 * 8)",
                 "#define LSF_ICP_PYRAMID_ROBUST_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 35 * 8)",
                 "#define LSF_ABI_VERSION 4", "} lsf_icp_robust_params;", "} lsf_icp_pyramid_robust_params;"):
        assert text in header, text
    assert lib.ABI_VERSION == 4 and lib.lib.lsf_abi_version() == 4 and lib.ICP_RECORD_DOUBLES == 64
    for name, pointers in (("lsf_icp_run_robust", 13), ("lsf_icp_run_pyramid_robust", 14)):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None and name + "(" in header
        assert len(lib.PROTOTYPES[name][1]) == pointers


def _robust_cases(entry, names, sizes, outs, optional, params):
    """the refusals the two entry points share; optional: the two photometric inputs"""
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}  # 1 MiB apart: nothing aliases
    images = ("residuals", "intensity_residuals", "weights")

    def case(want=-1, p=None, no_params=False, **moved):
        at = dict(base, **{name: None for name in images})
        at.update(moved)
        return dict(entry=entry, passes=want is None, want=want, pointers=[at[name] for name in names],
                    params=None if no_params else bytes(p or params()).hex())

    geometric = {optional[0]: None, optional[1]: None}
    cases = {"no params": case(no_params=True)}
    required = [n for n in names if n not in optional + images]
    for name in required:
        cases["no %s" % name] = case(**{name: None})
    for field, value in (("loss", 0), ("loss", 3), ("loss", -1), ("scale", 0.0), ("scale", -0.001),
                         ("scale", math.nan), ("intensity_scale", 0.0), ("intensity_scale", -1.0),
                         ("intensity_scale", math.nan), ("photometric_weight", 0.0), ("photometric_weight", -0.1),
                         ("photometric_weight", math.nan), ("photometric_weight", math.inf),
                         ("max_intensity_difference", 0.0), ("max_intensity_difference", math.nan), ("height", 0),
                         ("width", -1), ("fx", 0.0), ("fy", math.nan), ("max_distance", 0.0), ("levels", 0)):
        cases["%s %r" % (field, value)] = case(p=params(**{field: value}))
    cases["a negative iteration count"] = case(p=params(iterations=(2, -1, 3)))
    # the photometric inputs go together, with lambda, and the intensity residual image with them
    cases["one image without the other"] = case(**{optional[0]: None})
    cases["the other image without the one"] = case(**{optional[1]: None})
    cases["a weight without images"] = case(**geometric)
    cases["an intensity residual image without images"] = case(p=params(photometric_weight=0.0),
                                                               intensity_residuals=base["intensity_residuals"],
                                                               **geometric)
    cases["an unknown loss without images"] = case(p=params(photometric_weight=0.0, loss=7), **geometric)
    for out, n in outs.items():
        for name, size in sizes.items():
            cases["%s in the last byte of %s" % (out, name)] = case(**{out: base[name] + size - 1})
            cases["%s over the first byte of %s" % (out, name)] = case(**{out: base[name] - n + 1})
    cases["the weights alias the residuals"] = case(residuals=base["residuals"], weights=base["residuals"])
    cases["the weights alias the intensity residuals"] = case(intensity_residuals=base["weights"],
                                                              weights=base["weights"])
    cases["the weights alias the scratch"] = case(weights=base["scratch"])
    cases["the weights alias the twist"] = case(weights=base["twist"])
    cases["the plain call"] = case(want=None)
    cases["every image"] = case(want=None, **{name: base[name] for name in images})
    cases["tukey"] = case(want=None, p=params(loss=2))
    cases["infinite scales"] = case(want=None, p=params(scale=math.inf, intensity_scale=math.inf))
    cases["the geometric solve"] = case(want=None, p=params(photometric_weight=0.0), weights=base["weights"],
                                        residuals=base["residuals"], **geometric)
    cases["the geometric solve does not read the gate"] = case(
        want=None, p=params(photometric_weight=0.0, max_intensity_difference=0.0), **geometric)
    cases["nothing to launch"] = case(want=0, p=params(iterations=(0, 0, 0)), records=None,
                                      **{name: base[name] for name in images})
    return cases


def test_the_strided_entry_point_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    h, w = 48, 64
    names = ("live_depth", "live_colour", "pred_depth", "pred_normals", "pred_colour", "twist", "records", "scratch",
             "residuals", "intensity_residuals", "weights")
    sizes = dict(live_depth=2 * h * w, live_colour=3 * h * w, pred_depth=4 * h * w, pred_normals=12 * h * w,
                 pred_colour=16 * h * w)
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.ICP_ROBUST_SCRATCH_BYTES, residuals=4 * h * w,
                intensity_residuals=4 * h * w, weights=4 * h * w)

    def params(iterations=(2, 0, 3), **fields):
        p = lib.IcpRobustParams()
        p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance = 70.0, 70.0, 32.0, 24.0, 0.001, 0.02
        p.photometric_weight, p.max_intensity_difference = 0.1, math.inf
        p.height, p.width, p.depth_dtype, p.levels = h, w, lib.DEPTH_U16, len(iterations)
        p.iterations[:len(iterations)] = list(iterations)
        p.strides[:3] = [4, 2, 1]
        p.loss, p.scale, p.intensity_scale = lib.ICP_LOSS_HUBER, 0.001, 0.05
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    cases = _robust_cases("lsf_icp_run_robust", names, sizes, outs, ("live_colour", "pred_colour"), params)
    cases["a stride of 0"] = dict(cases["the plain call"], passes=False, want=-1,
                                  params=bytes(params(strides=(ctypes.c_int32 * 4)(4, 0, 1, 0))).hex())
    cases["an unknown depth dtype"] = dict(cases["the plain call"], passes=False, want=-1,
                                           params=bytes(params(depth_dtype=9)).hex())
    PH._check(cases)


def test_the_pyramid_entry_point_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    h, w, levels = 48, 64, 3
    pyramid = sum((h >> l) * (w >> l) for l in range(levels))
    names = ("live_depth", "live_normals", "live_intensity", "pred_depth", "pred_normals", "pred_intensity", "twist",
             "records", "scratch", "residuals", "intensity_residuals", "weights")
    sizes = dict(live_depth=4 * pyramid, live_normals=12 * pyramid, live_intensity=4 * pyramid, pred_depth=4 * h * w,
                 pred_normals=12 * h * w, pred_intensity=4 * pyramid)
    # the last iteration runs on level 0 (entry 2): the three images are 48 x 64
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.ICP_PYRAMID_ROBUST_SCRATCH_BYTES, residuals=4 * h * w,
                intensity_residuals=4 * h * w, weights=4 * h * w)

    def params(iterations=(2, 0, 3), **fields):
        p = lib.IcpPyramidRobustParams()
        p.fx, p.fy, p.cx, p.cy, p.max_distance, p.cos_max_angle = 70.0, 70.0, 32.0, 24.0, 0.02, 0.9
        p.photometric_weight, p.max_intensity_difference = 0.1, math.inf
        p.height, p.width, p.pyramid_levels, p.levels, p.angle_gate = h, w, levels, len(iterations), 1
        p.iterations[:len(iterations)] = list(iterations)
        p.loss, p.scale, p.intensity_scale = lib.ICP_LOSS_TUKEY, 0.003, math.inf
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    cases = _robust_cases("lsf_icp_run_pyramid_robust", names, sizes, outs, ("live_intensity", "pred_intensity"), params)
    plain = cases["the plain call"]
    for field, value in (("cos_max_angle", 1.5), ("pyramid_levels", 0), ("pyramid_levels", 5), ("levels", 4)):
        cases["%s %r" % (field, value)] = dict(plain, passes=False, want=-1,
                                               params=bytes(params(**{field: value})).hex())
    # with the last iteration on level 2 the weight image is 12 x 16: right behind an input passes, one float into it
    # is refused
    coarse = bytes(params(iterations=(2, 0, 0))).hex()
    at = dict(zip(names, plain["pointers"]))
    behind = at["pred_intensity"] + 4 * pyramid
    cases["coarse weights right behind an input"] = dict(plain, params=coarse,
                                                         pointers=plain["pointers"][:-1] + [behind])
    cases["coarse weights one float early"] = dict(plain, passes=False, want=-1, params=coarse,
                                                   pointers=plain["pointers"][:-1] + [behind - 4])
    cases["no gate"] = dict(plain, params=bytes(params(angle_gate=0)).hex())
    PH._check(cases)


def test_python_argument_checks():
    from levelsetfusion_python_amd import device_icp, fusion, rigid_opt
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, ProjectiveIcp3d, RobustLoss
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    import fusion_scene as S
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    loss = RobustLoss("tukey", 0.003)
    assert (loss.kind, loss.code, loss.scale, loss.intensity_scale) == ("tukey", 2, 0.003, math.inf)
    assert RobustLoss("huber", 1, 0.05).code == 1 and RobustLoss(kind="huber", scale=math.inf).scale == math.inf
    assert "no value is right across sensors" in " ".join(RobustLoss.__init__.__doc__.split())
    with pytest.raises(TypeError):
        RobustLoss("huber")  # no default scale
    for bad in (("cauchy", 0.003), ("tukey", 0.0), ("tukey", -1.0), ("tukey", math.nan), ("huber", 0.001, 0.0),
                ("huber", 0.001, math.nan)):
        with pytest.raises(ValueError):
            RobustLoss(*bad)

    p = device_icp.robust_params(cam, (480, 640), np.arange(6) * 0.01, 1, loss, iterations=(2, 5), strides=(2, 1))
    assert (p.loss, p.scale, p.intensity_scale, p.photometric_weight, p.max_intensity_difference) == \
        (2, 0.003, math.inf, 0.0, math.inf)
    assert (p.height, p.width, p.levels, list(p.iterations), list(p.strides), p.depth_dtype, p.depth_unit_ratio) == \
        (480, 640, 2, [2, 5, 0, 0], [2, 1, 0, 0], 1, 0.001)
    p = device_icp.robust_params(cam, (48, 64), np.zeros(6), 0, RobustLoss("huber", 0.001, 0.05), 0.25, 0.5)
    assert (p.loss, p.scale, p.intensity_scale, p.photometric_weight, p.max_intensity_difference) == \
        (1, 0.001, 0.05, 0.25, 0.5)
    q = device_icp.pyramid_robust_params(cam, (480, 640), 3, np.zeros(6), loss, 0.1, 0.125, (2, 5), 0.03, 0.3)
    assert (q.loss, q.scale, q.photometric_weight, q.max_intensity_difference, q.pyramid_levels, q.levels,
            list(q.iterations), q.angle_gate, q.cos_max_angle, q.max_distance) == \
        (2, 0.003, 0.1, 0.125, 3, 2, [2, 5, 0, 0], 1, math.cos(0.3), 0.03)
    for bad in (None, "tukey", 0.003, RR.Loss("tukey", 0.003)):
        with pytest.raises(ValueError, match="RobustLoss"):
            device_icp.robust_params(cam, (48, 64), np.zeros(6), 0, bad)
        with pytest.raises(ValueError, match="RobustLoss"):
            device_icp.pyramid_robust_params(cam, (48, 64), 3, np.zeros(6), bad)
        if bad is not None:
            with pytest.raises(ValueError, match="RobustLoss"):
                ProjectiveIcp3d(cam, robust=bad)
    with pytest.raises(ValueError):
        device_icp.robust_params(cam, (48, 64), np.zeros(6), 0, loss, photometric_weight=0.0)
    record = np.arange(64, dtype=np.float64)
    r = device_icp.unpack_record(record)
    assert (r["weight_sum"], r["photometric_weight_sum"], r["outliers"]) == (61.0, 62.0, 63)
    assert (r["count"], r["angle_rejected"], r["photometric_count"], r["photometric_energy"]) == (56, 58, 59, 60.0)

    # every configuration takes one
    for kw in (dict(), dict(pyramid=DepthPyramid(), max_normal_angle=0.3), dict(photometric_weight=0.1),
               dict(pyramid=DepthPyramid(), intensity_pyramid=IntensityPyramid(), photometric_weight=0.1)):
        t = ProjectiveIcp3d(cam, robust=loss, **kw)
        assert t.robust is loss and t.last_weights is None
    assert ProjectiveIcp3d(cam).robust is None
    t = ProjectiveIcp3d(cam, robust=loss, photometric_weight=0.1)
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        t.track(None, 0, None, None, np.zeros(6), np.zeros(6))

    kw = dict(camera=cam, field_shape=8, array_offset=[0, 0, 100])
    for mode in ("model", "raycast"):
        with pytest.raises(ValueError, match="icp_robust needs"):
            fusion.SequenceFusion3d(**kw, tracking_reference=mode, icp_robust=loss)
    with pytest.raises(ValueError, match="RobustLoss"):
        fusion.SequenceFusion3d(**kw, tracking_reference="icp", icp_robust="tukey")
    assert "icp_robust" in fusion.__doc__ and "Robust ICP" in fusion.__doc__
    not_covered = fusion.__doc__[fusion.__doc__.index("Not covered:"):]
    assert "Huber / Tukey" not in not_covered
    for text in ("a scale estimated from the residuals", "`pixel_weight` in fusion", "SDF-2-SDF trackers"):
        assert text in " ".join(not_covered.split()), text
    assert rigid_opt.RobustLoss is RobustLoss
    assert callable(device_icp.icp_run_robust) and callable(device_icp.icp_run_pyramid_robust)
