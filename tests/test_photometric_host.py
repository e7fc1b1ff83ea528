"""CPU checks of the ray-cast colour image and of the joint geometric and photometric ICP: the restated Jacobian against
finite differences, the conditions the GPU tests' scenes must meet (tests/textured_wall_scene.py,
tests/photometric_restatement.py), the accuracy bounds the GPU tests import, the ctypes layout of
lsf_icp_photometric_params, the header's macros, the exports, and the refusal of bad arguments by both C entry points
and by the Python interfaces."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import colour_scene as CS
import fusion_scene as S
import icp_restatement as I
import photometric_restatement as PR
import textured_wall_scene as W
from conftest import ROOT

LAMBDA = 0.1
RUN_ITERATIONS, RUN_STRIDES = (4, 5, 10), (4, 2, 1)

# The accuracy bounds of the GPU tests: twice the restatement's own error on the same inputs, measured here on the
# CPU (test_restated_run_meets_its_bound, test_restated_sequence_meets_its_bound pin the measurements to 2 %).
# The whole run on the 152 x 120 wall (analytic prediction at 0, live frame at textured_wall_scene.MOTION, lambda 0.1,
# iterations (4, 5, 10) at strides (4, 2, 1)): the final twist errs by 2.0815e-6 m and 8.9645e-6 rad.
RUN_ERROR_T, RUN_ERROR_R = 2.0815e-6, 8.9645e-6
RUN_ATOL_T, RUN_ATOL_R = 2 * RUN_ERROR_T, 2 * RUN_ERROR_R
# The restated three-frame sequence of the wall (fusion_scene's K, 640 x 480 and STEP, 64^3, colour_band 0.25, lambda
# 0.1, the default schedule): the worst frame errs by 2.2155e-5 m and 5.7768e-5 rad.  The geometric-only sequence
# (icp_restatement.sequence) on the same frames errs in the plane by 3 mm (frame 1, whose every iteration is skipped)
# and by 5.3 mm in t_x, 14 mm in t_y and 2.1e-2 rad in r_z (frame 2, against the model's uneven normals).
SEQUENCE_ERROR_T, SEQUENCE_ERROR_R = 2.2155e-5, 5.7768e-5
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 2 * SEQUENCE_ERROR_T, 2 * SEQUENCE_ERROR_R
SEQUENCE_N, SEQUENCE_FRAMES, SEQUENCE_COLOUR_BAND = 64, 3, 0.25

# test 1 of the GPU file: colour_scene's model seen at frame 1's twist with K / 8 into 88 x 56 pixels
CAST_K = (S.K / 8).astype(np.float32)
CAST_SHAPE = (56, 88)


@functools.lru_cache(maxsize=None)
def wall_inputs():
    """the kernel tests' wall: (prediction depth, normals, colour at the zero twist; live depth float32, colour)"""
    out = W.prediction(np.zeros(6), W.K_SMALL, W.SHAPE_SMALL) + W.render(W.MOTION, W.K_SMALL, W.SHAPE_SMALL)[:2]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_run():
    """(records, final twist) of the whole joint run on the wall"""
    pd, pn, pc, depth, image = wall_inputs()
    return PR.icp(depth, image, pd, pn, pc, W.K_SMALL, 1.0, np.zeros(6), LAMBDA, None, RUN_ITERATIONS, RUN_STRIDES)


@functools.lru_cache(maxsize=None)
def sequence_frames():
    out = tuple(W.render(S.true_twist(k), S.K, (S.HEIGHT, S.WIDTH))[:2] for k in range(SEQUENCE_FRAMES))
    for f in out:
        for a in f:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_sequence():
    """photometric_restatement.sequence of the wall's three frames; nothing modifies it"""
    frames = sequence_frames()
    n = SEQUENCE_N
    return PR.sequence([f[0] for f in frames], [f[1] for f in frames], S.K, 1.0, (n,) * 3, S.offset(n), LAMBDA,
                       colour_band=SEQUENCE_COLOUR_BAND)


def test_restated_jacobian_against_finite_differences():
    """J_I against central differences of r_I under the left perturbation g <- g + tau + omega x g
    (icp_restatement.compose), at the wall's pixels whose projection stays in one cell of the prediction, where the
    interpolant is smooth.  Step h = 1e-6 per component.  Rounding: r_I is a few operations on values below 1, in
    error by about 1e-15, over 2 h: 5e-10.  Truncation: h^2 / 6 times the third derivative of r_I along the step; r_I
    is bilinear in (pu, pv), its gradient at most 0.3 per pixel here, and pu's third derivative in a translation is
    6 fx / q_z^4 < 1e4 per m^3 (rotations: times |g|^3 < 1): below 1e-12 * 0.3 * 1e4 / 6 = 5e-10.  The bound, 1e-7,
    is a hundred times their sum and 1e-8 of the Jacobian's entries, which reach 10 to 100."""
    h, bound = 1e-6, 1e-7
    pd, pn, pc, depth, image = wall_inputs()
    twist, twist_p = W.MOTION + np.array([4e-4, -3e-4, 2e-4, 1e-3, -2e-3, 1.5e-3]), np.zeros(6)

    def terms(tw):
        rows, cols, valid, _, g, _, _ = I.associate(depth, pd, pn, W.K_SMALL, 1.0, tw, twist_p)
        has, rI, J = PR.photometric_terms(image, pc, W.K_SMALL, twist_p, rows, cols, valid, g)
        fxq = [((float(W.K_SMALL[0, 0]) * g[0]) / g[2]) + float(W.K_SMALL[0, 2]),
               ((float(W.K_SMALL[1, 1]) * g[1]) / g[2]) + float(W.K_SMALL[1, 2])]  # twist_p = 0: q = g
        return has, rI, J, np.floor(fxq[0]), np.floor(fxq[1])

    has, _, J, cx, cy = terms(twist)
    assert has.sum() > 10000
    checked = 0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        hp, rp, _, xp, yp = terms(I.compose(twist, d))
        hm, rm, _, xm, ym = terms(I.compose(twist, -d))
        same = has & hp & hm & (xp == cx) & (xm == cx) & (yp == cy) & (ym == cy)
        assert same.sum() > 0.9 * has.sum()
        fd = (rp[same] - rm[same]) / (2 * h)
        assert np.abs(J[k][same]).max() > 1.0
        assert np.abs(fd - J[k][same]).max() <= bound, (k, np.abs(fd - J[k][same]).max())
        checked += int(same.sum())
    assert checked > 60000


def test_geometry_alone_skips_every_iteration_on_the_wall():
    pd, pn, _, depth, _ = wall_inputs()
    records, twist = I.icp(depth, pd, pn, W.K_SMALL, 1.0, np.zeros(6), None, RUN_ITERATIONS, RUN_STRIDES)
    assert len(records) == 19 and all(r["skipped"] == 1 and r["count"] > 1000 for r in records)
    assert np.array_equal(twist, np.zeros(6))


def test_restated_run_meets_its_bound():
    """the joint run updates in every iteration, most geometric pairs carry a photometric term, and the final twist's
    error is the recorded one: the GPU test's bound is twice it"""
    records, twist = restated_run()
    assert [r["level"] for r in records] == [0] * 4 + [1] * 5 + [2] * 10
    assert all(r["skipped"] == 0 for r in records)
    for r in records:
        assert r["count"] > 1000 and 2 * (r["count"] - r["photometric_count"]) < r["count"]
    err = np.abs(twist - W.MOTION)
    np.testing.assert_allclose([err[:3].max(), err[3:].max()], [RUN_ERROR_T, RUN_ERROR_R], rtol=0.02)
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R


def test_ray_cast_colour_covers_the_hits():
    """at least half of the hit pixels of the GPU file's first test carry a colour, and the others are NaN"""
    t, w, c, _, _ = CS.restated_model()
    _, _, hits, image = PR.raycast_colour(t, w, c, CAST_K, S.true_twist(1), CS.offset(), CS.VOXEL, CAST_SHAPE)
    coloured = np.isfinite(image).all(axis=2)
    assert hits > 500 and 2 * int(coloured.sum()) >= hits
    assert np.isnan(image[~coloured]).all()
    lit = image[coloured]
    np.testing.assert_allclose(lit[:, 3], W.luminance(lit[:, :3]), rtol=1e-6)


def test_restated_sequence_meets_its_bound():
    """the restated photometric sequence tracks the wall within the recorded error; the geometric-only sequence on the
    same frames errs in the plane (t_x, t_y, r_z) by more than the GPU test's bound"""
    _, _, _, twists, _, hits, icp = restated_sequence()
    truth = np.array([S.true_twist(k) for k in range(SEQUENCE_FRAMES)])
    err = np.abs(np.array(twists) - truth)
    assert hits[0] is None and min(hits[1:]) > 40000
    assert all(r["skipped"] == 0 and 2 * r["photometric_count"] > r["count"] for recs in icp[1:] for r in recs)
    np.testing.assert_allclose([err[1:, :3].max(), err[1:, 3:].max()], [SEQUENCE_ERROR_T, SEQUENCE_ERROR_R], rtol=0.02)
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R
    frames = [f[0] for f in sequence_frames()]
    n = SEQUENCE_N
    _, _, geometric, _, _, _ = I.sequence(frames, S.K, 1.0, (n,) * 3, S.offset(n))
    print("geometric-only |twist - truth|, frames 1-2:\n", np.abs(np.array(geometric) - truth)[1:])
    plane = np.abs(np.array(geometric) - truth)[1:][:, [0, 1, 5]]
    assert plane[:, :2].max() > SEQUENCE_ATOL_T and plane[:, 2].max() > SEQUENCE_ATOL_R


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.IcpPhotometricParams
    assert [f[0] for f in p._fields_] == ["fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance",
                                          "photometric_weight", "max_intensity_difference", "twist_p", "height",
                                          "width", "depth_dtype", "levels", "iterations", "strides"]
    assert ctypes.sizeof(p) == 14 * 8 + 4 * 4 + 2 * 4 * 4 and p.twist_p.offset == 64 and p.height.offset == 112
    assert p.strides.offset == 144
    assert lib.ICP_PHOTOMETRIC_SCRATCH_BYTES == 2 * 256 * 31 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    assert "#define LSF_ICP_PHOTOMETRIC_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 31 * 8)" in header
    assert "#define LSF_ABI_VERSION 4" in header and lib.ABI_VERSION == 4 and lib.lib.lsf_abi_version() == 4
    for name in ("lsf_raycast_colour", "lsf_icp_run_photometric"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None and name + "(" in header
    assert len(lib.PROTOTYPES["lsf_raycast_colour"][1]) == 10
    assert len(lib.PROTOTYPES["lsf_icp_run_photometric"][1]) == 12


def _good_params():
    import levelsetfusion_python_amd._lib as lib
    p = lib.IcpPhotometricParams()
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance = 70.0, 70.0, 32.0, 24.0, 0.001, 0.02
    p.photometric_weight, p.max_intensity_difference = 0.1, math.inf
    p.height, p.width, p.depth_dtype, p.levels = 48, 64, lib.DEPTH_U16, 2
    p.iterations[:2] = [2, 3]
    p.strides[:2] = [2, 1]
    return p


def test_the_photometric_entry_point_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    f = lib.lib.lsf_icp_run_photometric
    p = _good_params()
    # never dereferenced: every call below is refused on the host.  The fake buffers are 1 MiB apart, so only the
    # cases built to alias do.
    live, lc, pd, pn, pc, tw, rec, sc, res, ires = (ctypes.c_void_p((1 << 20) * k) for k in range(1, 11))
    good = [live, lc, pd, pn, pc, tw, rec, sc, None, None]
    for field, value in (("photometric_weight", 0.0), ("photometric_weight", -0.1), ("photometric_weight", math.nan),
                         ("photometric_weight", math.inf), ("max_intensity_difference", 0.0),
                         ("max_intensity_difference", -1.0), ("max_intensity_difference", math.nan),
                         ("height", 0), ("width", -1), ("fx", 0.0), ("fy", math.nan), ("cx", math.inf),
                         ("depth_unit_ratio", math.nan), ("max_distance", 0.0), ("max_distance", math.nan),
                         ("depth_dtype", 3), ("levels", 0), ("levels", 5)):
        q = lib.IcpPhotometricParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert f(*good, ctypes.byref(q), None) == -1, (field, value)
    for edit in (lambda q: q.strides.__setitem__(1, 0), lambda q: q.iterations.__setitem__(0, -1),
                 lambda q: q.twist_p.__setitem__(4, math.nan)):
        q = lib.IcpPhotometricParams.from_buffer_copy(p)
        edit(q)
        assert f(*good, ctypes.byref(q), None) == -1
    P = ctypes.byref(p)
    for k in range(8):  # every required pointer
        args = list(good)
        args[k] = None
        assert f(*args, P, None) == -1, k
    assert f(*good, None, None) == -1
    for k, other in ((5, lc),    # the twist aliases the live colour
                     (6, pc),    # records alias the prediction's colour
                     (7, rec),   # scratch aliases the records
                     (8, pc),    # residuals alias the prediction's colour
                     (9, lc),    # intensity residuals alias the live colour
                     (9, sc)):   # intensity residuals alias the scratch
        args = list(good)
        args[k] = other
        assert f(*args, P, None) == -1, k
    args = list(good)
    args[8] = args[9] = res      # the two residual images alias each other
    assert f(*args, P, None) == -1
    args = list(good)
    args[9] = ctypes.c_void_p((1 << 20) * 5 + 16 * 48 * 64 - 4)  # the last float of the prediction's colour
    assert f(*args, P, None) == -1
    args = list(good)
    args[8], args[9] = res, ires
    q = lib.IcpPhotometricParams.from_buffer_copy(p)
    q.iterations[0] = q.iterations[1] = 0
    args[6] = None
    assert f(*args, ctypes.byref(q), None) == 0  # nothing to launch


def test_the_colour_ray_cast_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    f = lib.lib.lsf_raycast_colour
    p = lib.RaycastParams()
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.voxel_size = 70.0, 70.0, 32.0, 24.0, 0.001, 0.004
    p.depth, p.height, p.width, p.image_height, p.image_width = 8, 8, 8, 48, 64
    # 8^3 voxels: 2 KiB per scalar volume, 8 KiB of colour; the images 12, 36 and 48 KiB; buffers 1 MiB apart
    t, w, c, fb, d, n, co, hc = (ctypes.c_void_p((1 << 20) * k) for k in range(1, 9))
    good = [t, w, c, None, d, n, co, hc]
    P = ctypes.byref(p)
    for k in (0, 1, 2, 4, 6):  # tsdf, weight, colour, depth_out and colour_out are required
        args = list(good)
        args[k] = None
        assert f(*args, P, None) == -1, k
    assert f(*good, None, None) == -1
    for k, other in ((6, c),                                     # the colour image aliases the colour volume
                     (6, ctypes.c_void_p(c.value + 8 * 1024 - 4)),  # ... its last float
                     (6, t), (6, d), (6, n), (6, hc),
                     (4, c), (5, c), (7, c),
                     (4, ctypes.c_void_p(co.value + 16 * 48 * 64 - 4))):  # depth_out in the colour image's last float
        args = list(good)
        args[k] = other
        assert f(*args, P, None) == -1, (k, other)
    args = list(good)
    args[3] = co  # the fallback image aliases the colour image
    assert f(*args, P, None) == -1
    for field, value in (("voxel_size", 0.0), ("fx", 0.0), ("image_height", 0), ("depth", 1), ("t_x", math.nan)):
        q = lib.RaycastParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert f(*good, ctypes.byref(q), None) == -1, (field, value)


def test_python_argument_checks():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_icp, fusion
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    p = device_icp.photometric_params(cam, (480, 640), np.arange(6) * 0.01, 0, 0.25, 0.125)
    assert (p.height, p.width, p.levels, list(p.iterations), list(p.strides)) == (480, 640, 3, [4, 4, 6, 0],
                                                                                   [4, 2, 1, 0])
    assert (p.fx, p.depth_unit_ratio, p.max_distance, p.photometric_weight, p.max_intensity_difference,
            p.twist_p[5]) == (700.0, 0.001, 0.02, 0.25, 0.125, 0.05)
    assert device_icp.photometric_params(cam, (4, 4), np.zeros(6), 0, 1.0).max_intensity_difference == math.inf
    for weight, gate in ((0.0, 1.0), (-1.0, 1.0), (math.nan, 1.0), (math.inf, 1.0), (0.1, 0.0), (0.1, -0.5),
                         (0.1, math.nan)):
        with pytest.raises(ValueError):
            device_icp.photometric_params(cam, (48, 64), np.zeros(6), 0, weight, gate)
        with pytest.raises(ValueError):
            lsf.ProjectiveIcp3d(cam, photometric_weight=weight, max_intensity_difference=gate)
    with pytest.raises(ValueError, match="intensity pyramid"):
        lsf.ProjectiveIcp3d(cam, iterations=(1,), pyramid=DepthPyramid(levels=1), photometric_weight=0.1)
    t = lsf.ProjectiveIcp3d(cam, photometric_weight=0.1, max_intensity_difference=0.5)
    assert (t.photometric_weight, t.max_intensity_difference, t.last_intensity_residuals) == (0.1, 0.5, None)
    assert lsf.ProjectiveIcp3d(cam).photometric_weight is None
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        t.track(None, 0, None, None, np.zeros(6), np.zeros(6))
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        lsf.ProjectiveIcp3d(cam).track(None, 0, None, None, np.zeros(6), np.zeros(6), colour_image=0,
                                       prediction_colour=0)
    kw = dict(camera=cam, field_shape=8, array_offset=[0, 0, 100])
    for bad in (dict(photometric_weight=0.1, tracking_reference="icp"),                  # no colour volume
                dict(photometric_weight=0.1, colour=True),                               # "model" tracking
                dict(photometric_weight=0.1, colour=True, tracking_reference="raycast"),
                dict(photometric_weight=0.1, colour=True, tracking_reference="icp", icp_iterations=(1,),
                     icp_pyramid=DepthPyramid(levels=1)),
                dict(photometric_weight=-0.1, colour=True, tracking_reference="icp"),
                dict(photometric_weight=0.1, colour=True, tracking_reference="icp",
                     icp_max_intensity_difference=0.0)):
        with pytest.raises(ValueError):
            fusion.SequenceFusion3d(**kw, **bad)
    assert "photometric_weight" in fusion.__doc__ and "photometric (colour) tracking" not in fusion.__doc__
    assert "an intensity pyramid" in fusion.__doc__
    assert callable(device_icp.icp_run_photometric)
    r = device_icp.unpack_record(np.arange(64, dtype=np.float64))
    assert (r["photometric_count"], r["photometric_energy"], r["count"], r["energy"]) == (59, 60.0, 56, 12.0)
