"""CPU checks of point-to-SDF tracking: the restatement's own properties (tests/point_sdf_restatement.py) -- the pose it
recovers on tests/fusion_scene.py, the restated "sdf" sequence, Tukey weights on tests/moving_part_scene.py --, the ctypes
layout of lsf_point_sdf_params, the header's macros, the exports, the tracking-mode tuples, and the refusal of bad
arguments by the C entry point and by the Python interfaces."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import fusion_restatement as F
import fusion_scene as S
import moving_part_scene as M
import point_sdf_restatement as P
import robust_icp_restatement as RR
import test_pyramid_photometric_host as PH
from conftest import ROOT

# the restated "sdf" sequence, 48^3, four frames, iterations (4, 4, 6) at strides (4, 2, 1), 2 cm gate, measured: the
# largest translation error of a frame 0.250, 0.346 and 0.389 mm, the largest rotation error 4.16e-4, 5.77e-4 and
# 6.81e-4 rad (frames 1-3).  The bounds are twice the worst frame.
SEQUENCE_WORST_T, SEQUENCE_WORST_R = 3.89e-4, 6.81e-4
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 2 * SEQUENCE_WORST_T, 2 * SEQUENCE_WORST_R
# the moving-part scene against a 48^3 model of the undisturbed scene, measured (|t error| m, |r error| rad): least
# squares (2.20e-2, 5.12e-2), Huber at 1 mm (1.08e-3, 5.86e-3), Tukey at 3 mm (3.19e-4, 3.16e-3), least squares without
# the move (5.64e-4, 9.15e-4); profiles/point_sdf_cost.md has the table.  The bound is twice Tukey's error.
TUKEY_ERROR_T, TUKEY_ERROR_R = 3.19e-4, 3.16e-3


@functools.lru_cache(maxsize=None)
def model(shape=(48, 48, 48), offset=None):
    """frames 0 and 1 of the fusion scene fused at their true twists (restated): (tsdf, weight), read only"""
    off = S.offset(shape[0]) if offset is None else np.array(offset)
    t, w = F.empty_model(shape)
    for k, depth in enumerate(S.frames(2)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


@functools.lru_cache(maxsize=None)
def restated_sequence(count=4, n=48):
    """point_sdf_restatement.sequence of the scene's first frames at n^3; nothing modifies it"""
    return P.sequence(S.frames(count), S.K, 1.0, (n,) * 3, S.offset(n))


@pytest.mark.parametrize("n", [48, 64])
def test_the_restatement_converges(n):
    """from frame 1's twist onto frame 2: within 1e-3 of the true twist in every component (measured 4.0e-4 at 48^3,
    4.2e-4 at 64^3), every iteration with at least 1000 pairs (measured minimum 2417 and 4272)"""
    t, w = model((n,) * 3)
    records, twist, _, _ = P.track(t, w, S.render(S.true_twist(2)), S.K, 1.0, S.true_twist(1), S.offset(n))
    assert len(records) == 14 and [r["level"] for r in records] == [0] * 4 + [1] * 4 + [2] * 6
    assert np.abs(twist - S.true_twist(2)).max() <= 1e-3, twist - S.true_twist(2)
    assert min(r["count"] for r in records) >= 1000
    assert all(r["skipped"] == 0 and r["no_sample"] > 0 for r in records)
    assert np.linalg.cond(records[-1]["A"]) < 1e4  # measured 8e2 and 1.3e3


def test_restated_sdf_sequence():
    _, _, twists, fusion, records = restated_sequence()
    err = np.abs(np.array(twists) - np.array([S.true_twist(k) for k in range(4)]))
    assert records[0] == [] and all(len(r) == 14 for r in records[1:])
    assert np.array_equal(twists[0], np.zeros(6))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err
    np.testing.assert_allclose(err[1:, :3].max(), SEQUENCE_WORST_T, rtol=0.02)
    np.testing.assert_allclose(err[1:, 3:].max(), SEQUENCE_WORST_R, rtol=0.02)
    assert all(f["fused"] > 0 for f in fusion)


@functools.lru_cache(maxsize=None)
def moving_part_model(n=48):
    t, w = F.empty_model((n,) * 3)
    t, w, _ = F.fuse_depth(t, w, M.render(np.zeros(6), moved=False), M.K, 1.0, S.offset(n), np.zeros(6))
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def test_tukey_keeps_the_pose_where_least_squares_is_dragged(capsys):
    t, w = moving_part_model()
    err = {}
    for name, loss in (("least squares", None), ("tukey", RR.Loss("tukey", M.TUKEY_SCALE))):
        _, twist, _, _ = P.track(t, w, M.live(True), M.K, 1.0, np.zeros(6), S.offset(48), M.ITERATIONS, M.STRIDES,
                                 loss=loss)
        err[name] = M.pose_error(twist)
    with capsys.disabled():
        print("\npoint-to-SDF on the moving-part scene, |t error| (m) and |r error| (rad):", err)
    assert err["tukey"][0] <= 2 * TUKEY_ERROR_T and err["tukey"][1] <= 2 * TUKEY_ERROR_R, err
    assert err["least squares"][0] > 1e-2 and err["least squares"][1] > 2e-2, err  # the problem is there


def test_an_infinite_scale_is_the_plain_iteration():
    t, w = model()
    start = S.true_twist(1) + np.array([0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
    live = S.render(S.true_twist(2))
    want, want_res, none, want_twist = P.iteration(t, w, live, S.K, 1.0, start, S.offset(48), 2)
    assert none is None and want["weight_sum"] == 0.0 and want["count"] > 1000
    for kind in ("huber", "tukey"):
        got, res, weights, twist = P.iteration(t, w, live, S.K, 1.0, start, S.offset(48), 2,
                                               loss=RR.Loss(kind, np.inf))
        for key in ("A", "b", "energy", "count", "delta", "twist", "skipped", "no_sample", "outliers"):
            assert np.array_equal(got[key], want[key]), key
        assert got["weight_sum"] == want["count"] and np.array_equal(twist, want_twist)
        assert np.array_equal(res.view(np.uint32), want_res.view(np.uint32))
        assert np.array_equal(weights[np.isfinite(res)], np.ones(want["count"], np.float32))


def test_the_gradient_of_a_linear_field_is_exact():
    """phi = a x + b y + c z + e in float32-exact numbers: the sample is the field and the gradient (a, b, c)"""
    z, y, x = np.meshgrid(np.arange(5.0), np.arange(6.0), np.arange(7.0), indexing="ij")
    tsdf = (0.25 * x - 0.5 * y + 0.125 * z + 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    p = [np.array([0.0, 2.5, 5.75, 6.0, -0.25]), np.array([0.0, 1.25, 4.5, 1.0, 1.0]), np.array([0.0, 3.0, 3.5, 1.0, 1.0])]
    valid, phi, d = P.sample_gradient(tsdf, weight, p)
    assert list(valid) == [True, True, True, False, False]  # p_x = n_x - 1 has no sample
    assert np.array_equal(phi[:3], (0.25 * p[0] - 0.5 * p[1] + 0.125 * p[2] + 1.0)[:3])
    assert np.array_equal(np.array(d)[:, :3], np.array([[0.25] * 3, [-0.5] * 3, [0.125] * 3]))
    weight[3, 1, 2] = 0.0
    assert list(P.sample_gradient(tsdf, weight, p)[0]) == [True, False, True, False, False]


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.PointSdfParams
    assert ctypes.sizeof(p) == 160
    doubles = ("fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance", "voxel_size", "offset_x", "offset_y",
               "offset_z", "narrow_band_width_voxels", "scale")
    assert [f[0] for f in p._fields_] == list(doubles) + ["depth", "height", "width", "image_height", "image_width",
                                                          "depth_dtype", "levels", "iterations", "strides", "loss"]
    assert [getattr(p, n).offset for n in doubles] == list(range(0, 96, 8))
    assert (p.depth.offset, p.height.offset, p.width.offset, p.image_height.offset, p.image_width.offset,
            p.depth_dtype.offset, p.levels.offset, p.iterations.offset, p.strides.offset, p.loss.offset) == \
        (96, 100, 104, 108, 112, 116, 120, 124, 140, 156)
    assert lib.POINT_SDF_LOSS_NONE == 0 and lib.POINT_SDF_SCRATCH_BYTES == 2 * 256 * 33 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for text in ("#define LSF_POINT_SDF_LOSS_NONE 0", "#define LSF_ICP_RECORD_DOUBLES 64",
                 "#define LSF_POINT_SDF_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 33 * 8)", "#define LSF_ABI_VERSION 4",
                 "} lsf_point_sdf_params;", "lsf_point_sdf_run("):
        assert text in header, text
    assert lib.ABI_VERSION == 4 and lib.lib.lsf_abi_version() == 4 and lib.ICP_RECORD_DOUBLES == 64
    assert len(lib.PROTOTYPES["lsf_point_sdf_run"][1]) == 10 and lib.lib.lsf_point_sdf_run is not None
    from levelsetfusion_python_amd import _build
    assert "lsf_point_sdf.hip" in _build.SOURCES
    assert "lsf_icp_shared.h" in _build.HEADERS and "lsf_tsdf_sample.h" in _build.HEADERS


def test_the_entry_point_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    h, w, n = 48, 64, (8, 10, 12)
    names = ("tsdf", "weight", "live_depth", "twist", "records", "scratch", "residuals", "weights")
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}  # 1 MiB apart: nothing aliases
    voxels = 4 * n[0] * n[1] * n[2]
    sizes = dict(tsdf=voxels, weight=voxels, live_depth=2 * h * w)
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.POINT_SDF_SCRATCH_BYTES, residuals=4 * h * w,
                weights=4 * h * w)

    def params(iterations=(2, 0, 3), strides=(4, 2, 1), **fields):
        p = lib.PointSdfParams()
        p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance = 70.0, 70.0, 32.0, 24.0, 0.001, 0.02
        p.voxel_size, p.narrow_band_width_voxels, p.scale = 0.004, 20.0, 0.003
        p.offset_x, p.offset_y, p.offset_z = -6.0, -5.0, 100.0
        p.depth, p.height, p.width = n
        p.image_height, p.image_width, p.depth_dtype, p.levels = h, w, lib.DEPTH_U16, len(iterations)
        p.iterations[:len(iterations)] = list(iterations)
        p.strides[:len(strides)] = list(strides)
        p.loss = lib.ICP_LOSS_TUKEY
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def case(want=-1, p=None, no_params=False, **moved):
        at = dict(base, residuals=None, weights=None)
        at.update(moved)
        return dict(entry="lsf_point_sdf_run", passes=want is None, want=want, pointers=[at[name] for name in names],
                    params=None if no_params else bytes(p or params()).hex())

    cases = {"no params": case(no_params=True), "tsdf is weight": case(weight=base["tsdf"])}
    for name in ("tsdf", "weight", "live_depth", "twist", "records", "scratch"):
        cases["no %s" % name] = case(**{name: None})
    for field, value in (("image_height", 0), ("image_width", -1), ("depth", 1), ("height", 1), ("width", 1),
                         ("fx", 0.0), ("fy", math.nan), ("cx", math.inf), ("depth_unit_ratio", math.nan),
                         ("max_distance", 0.0), ("max_distance", math.nan), ("voxel_size", 0.0),
                         ("voxel_size", -0.004), ("voxel_size", math.nan), ("voxel_size", math.inf),
                         ("narrow_band_width_voxels", 0.0), ("narrow_band_width_voxels", -1.0),
                         ("narrow_band_width_voxels", math.nan), ("narrow_band_width_voxels", math.inf),
                         ("offset_x", math.nan), ("offset_z", math.inf), ("depth_dtype", 9), ("levels", 0),
                         ("levels", 5), ("loss", 3), ("loss", -1), ("scale", 0.0), ("scale", -0.001),
                         ("scale", math.nan)):
        cases["%s %r" % (field, value)] = case(p=params(**{field: value}))
    cases["a negative iteration count"] = case(p=params(iterations=(2, -1, 3)))
    cases["a stride of 0"] = case(p=params(strides=(4, 0, 1)))
    cases["too many pixels"] = case(p=params(image_height=1 << 16, image_width=1 << 15))
    cases["a weight image without a loss"] = case(p=params(loss=0), weights=base["weights"])
    for out, size in outs.items():
        for name, bytes_ in sizes.items():
            cases["%s in the last byte of %s" % (out, name)] = case(**{out: base[name] + bytes_ - 1})
            cases["%s over the first byte of %s" % (out, name)] = case(**{out: base[name] - size + 1})
    cases["the weights alias the residuals"] = case(residuals=base["residuals"], weights=base["residuals"])
    cases["the residuals alias the scratch"] = case(residuals=base["scratch"])
    cases["the weights alias the twist"] = case(weights=base["twist"])
    cases["the plain call"] = case(want=None)
    cases["both images"] = case(want=None, residuals=base["residuals"], weights=base["weights"])
    cases["no loss"] = case(want=None, p=params(loss=0, scale=math.nan), residuals=base["residuals"])
    cases["huber at an infinite scale"] = case(want=None, p=params(loss=1, scale=math.inf))
    cases["an infinite gate"] = case(want=None, p=params(max_distance=math.inf))
    cases["the smallest volume"] = case(want=None, p=params(depth=2, height=2, width=2))
    cases["residuals right behind the depth image"] = case(want=None, residuals=base["live_depth"] + 2 * h * w)
    cases["nothing to launch"] = case(want=0, p=params(iterations=(0, 0, 0)), records=None,
                                      residuals=base["residuals"], weights=base["weights"])
    PH._check(cases)


def test_python_argument_checks():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_point_sdf, fusion, rigid_opt
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, PointToSdf3d, RobustLoss
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    loss = RobustLoss("tukey", 0.003)
    p = device_point_sdf.params((40, 36, 52), cam, (480, 640), 0, [-26.25, -18.0, 112.5], 0.005, 16, (2, 5), (2, 1),
                                0.03)
    assert (p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance) == (700.0, 700.0, 320.0, 240.0, 0.001, 0.03)
    assert (p.voxel_size, p.narrow_band_width_voxels, p.offset_x, p.offset_y, p.offset_z) == \
        (0.005, 16.0, -26.25, -18.0, 112.5)
    assert (p.depth, p.height, p.width, p.image_height, p.image_width, p.depth_dtype, p.levels) == \
        (40, 36, 52, 480, 640, 0, 2)
    assert (list(p.iterations), list(p.strides), p.loss) == ([2, 5, 0, 0], [2, 1, 0, 0], 0)
    p = device_point_sdf.params((48,) * 3, cam, (48, 64), 2, S.offset(48), robust=loss)
    assert (p.loss, p.scale, p.voxel_size, p.narrow_band_width_voxels, p.max_distance) == (2, 0.003, 0.004, 20.0, 0.02)
    assert (list(p.iterations), list(p.strides)) == ([4, 4, 6, 0], [4, 2, 1, 0])
    for kw in (dict(shape=(48, 48)), dict(shape=(48, 1, 48)), dict(image_shape=(0, 64)), dict(depth_code=3),
               dict(voxel_size=0.0), dict(voxel_size=math.nan), dict(voxel_size=math.inf),
               dict(narrow_band_width_voxels=0), dict(narrow_band_width_voxels=math.inf), dict(max_distance=0.0),
               dict(max_distance=math.nan), dict(array_offset=[0.0, math.nan, 1.0]), dict(iterations=(1, 2)),
               dict(iterations=(-1, 1, 1)), dict(strides=(4, 0, 1)), dict(iterations=(1,) * 5, strides=(1,) * 5),
               dict(robust="tukey"), dict(robust=RR.Loss("tukey", 0.003))):
        args = dict(shape=(48,) * 3, camera=cam, image_shape=(48, 64), depth_code=0, array_offset=S.offset(48))
        args.update(kw)
        with pytest.raises(ValueError):
            device_point_sdf.params(**args)

    t = PointToSdf3d(cam)
    assert (t.iterations, t.strides, t.max_distance, t.robust) == ((4, 4, 6), (4, 2, 1), 0.02, None)
    assert t.last_records == [] and t.last_residuals is None and t.last_weights is None
    assert PointToSdf3d(cam, (2, 3), (2, 1), 0.05, loss).robust is loss
    for bad in (dict(iterations=(1, 2)), dict(strides=(0, 1, 1)), dict(max_distance=0.0), dict(robust="tukey")):
        with pytest.raises(ValueError):
            PointToSdf3d(cam, **bad)
    assert lsf.PointToSdf3d is rigid_opt.PointToSdf3d is PointToSdf3d and "PointToSdf3d" in lsf.__all__
    assert callable(device_point_sdf.point_sdf_run)

    # the mode tuples: the two old ones keep their values
    assert fusion.DIRECT_TRACKING_MODES == ("sdf",) and "DIRECT_TRACKING_MODES" in fusion.__all__
    assert fusion.TRACKING_REFERENCES == ("model", "raycast") and fusion.TRACKING_MODES == ("model", "raycast", "icp")
    kw = dict(camera=cam, field_shape=8, array_offset=[0, 0, 100])
    with pytest.raises(ValueError, match="tracking_reference must be one of"):
        fusion.SequenceFusion3d(**kw, tracking_reference="tsdf")
    for name, value in (("photometric_weight", 0.1), ("icp_robust", loss), ("icp_pyramid", DepthPyramid()),
                        ("icp_max_normal_angle", 0.3), ("icp_intensity_pyramid", IntensityPyramid())):
        with pytest.raises(ValueError, match="%s belongs to the \"icp\" tracker" % name):
            fusion.SequenceFusion3d(**kw, tracking_reference="sdf", colour=name == "photometric_weight",
                                    **{name: value})
    with pytest.raises(ValueError, match="PointToSdf3d"):
        fusion.SequenceFusion3d(**kw, tracking_reference="sdf", sdf_tracker=lsf.ProjectiveIcp3d(cam))
    for mode in ("model", "raycast", "icp"):
        with pytest.raises(ValueError, match="sdf_tracker needs"):
            fusion.SequenceFusion3d(**kw, tracking_reference=mode, sdf_tracker=t)
    doc = " ".join(fusion.__doc__.split())
    assert "\"sdf\"" in doc and "Point-to-SDF tracking" in doc
    not_covered = doc[doc.index("Not covered:"):]
    for text in ("a depth pyramid or filtered depth as the point source", "a colour term against the colour volume",
                 "a minimum-weight gate", "a per-voxel weight on the pairs"):
        assert text in not_covered, text
