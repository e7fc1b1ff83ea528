"""CPU checks of the live depth pyramid and of ICP over it: the ctypes layouts of lsf_depth_pyramid_params and
lsf_icp_pyramid_params, the header's macros, the exports, the refusal of bad arguments by both C entry points and by the
Python wrappers, properties of the numpy restatement (tests/depth_pyramid_restatement.py), and the restated accuracy of
pyramid tracking against today's strided tracking on the noisy scene (tests/noisy_scene.py)."""
import ctypes
import math
import os

import numpy as np
import pytest

import depth_pyramid_restatement as P
import fusion_scene as S
import icp_restatement as I
import noisy_scene as N
from conftest import ROOT

# the restated noisy "icp" sequence, 48^3, five frames of tests/noisy_scene.py (seed 0), iterations (4, 4, 6), 2 cm
# distance gate: the largest translation and rotation error of frames 1-4 against the true twists.  Strided tracking
# (strides (4, 2, 1)) on the raw frames, and pyramid tracking with the default DepthPyramid (3 levels, radius 3,
# sigma_space 3 px, sigma_range 3 cm, depth gate 3 cm) and a 20 degree normal-angle gate.
STRIDE_WORST_T, STRIDE_WORST_R = 3.414e-4, 1.9535e-3
PYRAMID_WORST_T, PYRAMID_WORST_R = 3.131e-4, 1.2684e-3
MAX_NORMAL_ANGLE = math.radians(20.0)


def _lib():
    import levelsetfusion_python_amd._lib as lib
    return lib


def test_params_layouts_and_macros():
    lib = _lib()
    d = lib.DepthPyramidParams
    assert [f[0] for f in d._fields_] == ["fx", "fy", "cx", "cy", "depth_unit_ratio", "sigma_space", "sigma_range",
                                          "depth_gate", "height", "width", "depth_dtype", "levels", "radius"]
    assert ctypes.sizeof(d) == 8 * 8 + 5 * 4 + 4 and d.height.offset == 64 and d.radius.offset == 80
    q = lib.IcpPyramidParams
    assert [f[0] for f in q._fields_] == ["fx", "fy", "cx", "cy", "max_distance", "cos_max_angle", "twist_p", "height",
                                          "width", "pyramid_levels", "levels", "angle_gate", "iterations"]
    assert ctypes.sizeof(q) == 12 * 8 + 9 * 4 + 4 and q.height.offset == 96 and q.iterations.offset == 116
    assert lib.PYRAMID_MAX_RADIUS == 8 and lib.ICP_PYRAMID_SCRATCH_BYTES == 2 * 256 * 30 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    assert "#define LSF_PYRAMID_MAX_RADIUS 8" in header
    assert "#define LSF_ICP_PYRAMID_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 30 * 8)" in header
    assert "#define LSF_ABI_VERSION 4" in header and lib.ABI_VERSION == 4
    for name in ("lsf_depth_pyramid", "lsf_icp_run_pyramid"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None


def _pyramid_params():
    lib = _lib()
    p = lib.DepthPyramidParams()
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio = 70.0, 70.0, 32.0, 24.0, 0.001
    p.sigma_space, p.sigma_range, p.depth_gate = 3.0, 0.03, 0.03
    p.height, p.width, p.depth_dtype, p.levels, p.radius = 48, 64, lib.DEPTH_U16, 3, 3
    return p


def test_the_pyramid_c_abi_refuses_bad_arguments_before_launching():
    lib = _lib()
    f = lib.lib.lsf_depth_pyramid
    p = _pyramid_params()
    # never dereferenced: every call below is refused on the host.  The fake buffers are 1 MiB apart.
    depth, out_d, out_n = (ctypes.c_void_p((1 << 20) * k) for k in (1, 2, 3))
    for field, value in (("height", 0), ("width", -1), ("height", 1 << 16), ("fx", 0.0), ("fy", math.nan),
                         ("cx", math.inf), ("cy", math.nan), ("depth_unit_ratio", math.nan), ("depth_gate", 0.0),
                         ("depth_gate", -0.01), ("depth_gate", math.nan), ("depth_dtype", 3), ("depth_dtype", -1),
                         ("radius", -1), ("radius", 9), ("sigma_space", 0.0), ("sigma_space", math.inf),
                         ("sigma_range", -1.0), ("sigma_range", math.nan), ("levels", 0), ("levels", 5),
                         ("height", 3), ("width", 2)):
        q = lib.DepthPyramidParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "height" and value == 1 << 16:
            q.width = 1 << 16  # 2^32 pixels
        assert f(depth, out_d, out_n, ctypes.byref(q), None) == -1, (field, value)
    P_ = ctypes.byref(p)
    for args in ((None, out_d, out_n), (depth, None, out_n), (depth, out_d, None),
                 (depth, depth, out_n),   # the depth output is the input
                 (depth, out_d, out_d),   # the normals overlap the depth output
                 (depth, out_d, ctypes.c_void_p((1 << 20) * 1 + 48 * 64 * 2 - 2))):  # the input's last pixel
        assert f(*args, P_, None) == -1, args
    assert f(depth, out_d, out_n, None, None) == -1
    near = ctypes.c_void_p((1 << 20) * 2 + 4 * (48 * 64 + 24 * 32 + 12 * 16) - 4)  # the depth output's last float
    assert f(depth, out_d, near, P_, None) == -1


def _icp_params():
    lib = _lib()
    p = lib.IcpPyramidParams()
    p.fx, p.fy, p.cx, p.cy, p.max_distance, p.cos_max_angle = 70.0, 70.0, 32.0, 24.0, 0.02, 0.9
    p.height, p.width, p.pyramid_levels, p.levels, p.angle_gate = 48, 64, 3, 2, 1
    p.iterations[:2] = [2, 3]
    return p


def test_the_pyramid_icp_c_abi_refuses_bad_arguments_before_launching():
    lib = _lib()
    f = lib.lib.lsf_icp_run_pyramid
    p = _icp_params()
    ld, ln, pd, pn, tw, rec, sc, res = (ctypes.c_void_p((1 << 20) * k) for k in range(1, 9))
    for field, value in (("height", 0), ("width", -1), ("height", 1 << 16), ("fx", 0.0), ("fy", math.nan),
                         ("cx", math.inf), ("max_distance", 0.0), ("max_distance", math.nan),
                         ("cos_max_angle", 1.5), ("cos_max_angle", -1.01), ("cos_max_angle", math.nan),
                         ("pyramid_levels", 0), ("pyramid_levels", 5), ("levels", 0), ("levels", 4),
                         ("height", 3)):
        q = lib.IcpPyramidParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "height" and value == 1 << 16:
            q.width = 1 << 16
        assert f(ld, ln, pd, pn, tw, rec, sc, None, ctypes.byref(q), None) == -1, (field, value)
    for edit in (lambda q: q.iterations.__setitem__(1, -1), lambda q: q.twist_p.__setitem__(2, math.inf)):
        q = lib.IcpPyramidParams.from_buffer_copy(p)
        edit(q)
        assert f(ld, ln, pd, pn, tw, rec, sc, None, ctypes.byref(q), None) == -1
    P_ = ctypes.byref(p)
    for args in ((None, ln, pd, pn, tw, rec, sc, None), (ld, None, pd, pn, tw, rec, sc, None),
                 (ld, ln, None, pn, tw, rec, sc, None), (ld, ln, pd, None, tw, rec, sc, None),
                 (ld, ln, pd, pn, None, rec, sc, None), (ld, ln, pd, pn, tw, None, sc, None),
                 (ld, ln, pd, pn, tw, rec, None, None),
                 (ld, ln, pd, pn, ld, rec, sc, None),       # the twist aliases the live depth
                 (ld, ln, pd, pn, tw, ln, sc, None),        # records alias the live normals
                 (ld, ln, pd, pn, tw, rec, pn, None),       # scratch aliases the prediction's normals
                 (ld, ln, pd, pn, tw, rec, rec, None),      # scratch aliases the records
                 (ld, ln, pd, pn, tw, rec, sc, pd),         # residuals alias the prediction
                 (ld, ln, pd, pn, tw, rec, sc, tw)):        # residuals alias the twist
        assert f(*args, P_, None) == -1, args
    assert f(ld, ln, pd, pn, tw, rec, sc, None, None, None) == -1
    near = ctypes.c_void_p((1 << 20) * 1 + 4 * (48 * 64 + 24 * 32 + 12 * 16) - 4)  # the live depth's last float
    assert f(ld, ln, pd, pn, tw, rec, sc, near, P_, None) == -1
    q = lib.IcpPyramidParams.from_buffer_copy(p)
    q.iterations[0] = q.iterations[1] = 0
    assert f(ld, ln, pd, pn, tw, None, sc, None, ctypes.byref(q), None) == 0  # nothing to launch


def _camera(ratio=0.001):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=ratio)


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_depth_pyramid as D, device_icp
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, ProjectiveIcp3d
    p = D.params(_camera(), (480, 640), 0)
    assert (p.levels, p.radius, p.sigma_space, p.sigma_range, p.depth_gate) == (3, 3, 3.0, 0.03, 0.03)
    assert (p.height, p.width, p.fx, p.cx, p.depth_unit_ratio) == (480, 640, 700.0, 320.0, 0.001)
    assert D.level_shapes((480, 640), 3) == [(480, 640), (240, 320), (120, 160)]
    assert D.level_intrinsics(_camera(), 3) == P.level_intrinsics(S.K, 3)
    for bad in (dict(levels=0), dict(levels=5), dict(radius=-1), dict(radius=9), dict(sigma_space=0.0),
                dict(sigma_range=math.nan), dict(sigma_space=math.inf), dict(depth_gate=0.0),
                dict(depth_gate=math.nan), dict(image_shape=(3, 640)), dict(image_shape=(0, 4))):
        kw = dict(camera=_camera(), image_shape=(48, 64), depth_code=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.params(**kw)
        if "image_shape" not in bad:
            with pytest.raises(ValueError):
                DepthPyramid(**bad)
    q = device_icp.pyramid_params(_camera(), (480, 640), 3, np.arange(6) * 0.01, (4, 4, 6), 0.02, 0.5)
    assert (q.pyramid_levels, q.levels, list(q.iterations), q.angle_gate) == (3, 3, [4, 4, 6, 0], 1)
    assert q.cos_max_angle == math.cos(0.5) and q.twist_p[5] == 0.05
    assert device_icp.pyramid_params(_camera(), (48, 64), 2, np.zeros(6), (3,)).angle_gate == 0
    assert device_icp.last_level((4, 4, 6)) == 0 and device_icp.last_level((4, 2, 0)) == 1
    for bad in (dict(iterations=(1, 2, 3, 4)), dict(iterations=(-1,)), dict(max_normal_angle=-0.1),
                dict(max_normal_angle=4.0), dict(max_normal_angle=math.nan), dict(max_distance=0.0),
                dict(pyramid_levels=0), dict(pyramid_levels=5), dict(image_shape=(2, 64)),
                dict(twist_p=[0, 0, math.nan, 0, 0, 0])):
        kw = dict(camera=_camera(), image_shape=(48, 64), pyramid_levels=3, twist_p=np.zeros(6))
        kw.update(bad)
        with pytest.raises(ValueError):
            device_icp.pyramid_params(**kw)
    t = ProjectiveIcp3d(None, iterations=(2, 5), pyramid=DepthPyramid(levels=2), max_normal_angle=0.3)
    assert (t.iterations, t.strides, t.max_normal_angle, t.last_pyramid) == ((2, 5), None, 0.3, None)
    assert ProjectiveIcp3d(None).pyramid is None
    for bad in (dict(max_normal_angle=0.3), dict(pyramid="yes"), dict(pyramid=DepthPyramid(levels=2)),
                dict(pyramid=DepthPyramid(), max_normal_angle=-1.0)):
        with pytest.raises(ValueError):
            ProjectiveIcp3d(None, **bad)


def test_package_exports_the_pyramid():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_depth_pyramid, device_icp, rigid_opt
    assert callable(device_depth_pyramid.depth_pyramid) and callable(device_icp.icp_run_pyramid)
    assert rigid_opt.DepthPyramid().levels == 3
    record = np.zeros(64)
    record[58] = 7
    assert device_icp.unpack_record(record)["angle_rejected"] == 7
    assert lsf.fusion.TRACKING_MODES == ("model", "raycast", "icp")


def test_a_constant_image_filters_to_itself():
    for value, dtype, ratio in ((0.75, np.float64, 1.0), (1234, np.uint16, 0.001), (1.5, np.float32, 0.5)):
        depth = np.full((40, 52), value, dtype)
        want = I.scaled_depth(depth, ratio).astype(np.float32)
        for radius in (0, 1, 3, 8):
            assert np.array_equal(P.bilateral(depth, ratio, radius), want)
    holes = np.full((40, 52), 0.75)
    holes[::3, ::5] = 0.0
    holes[7, 9] = np.nan
    out = P.bilateral(holes, 1.0)
    assert np.array_equal(out, np.where(holes > 0, np.float32(0.75), np.float32(0)))


def test_a_fronto_parallel_plane_has_normals_facing_the_camera_at_every_level():
    depth = np.full((48, 64), 0.6, np.float32)
    depths, normals, intr = P.pyramid(depth, 1.0, S.K, levels=4)
    for l, (d, n) in enumerate(zip(depths, normals)):
        assert d.shape == (48 >> l, 64 >> l) and np.all(d == np.float32(0.6))
        np.testing.assert_allclose(n[:-1, :-1], np.broadcast_to([0, 0, -1], n[:-1, :-1].shape), rtol=0, atol=1e-12)
        assert not n[-1].any() and not n[:, -1].any()


def test_level_intrinsics_project_a_point_to_the_block_it_came_from():
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-0.3, 0.3, 2000), rng.uniform(-0.2, 0.2, 2000), rng.uniform(0.4, 1.2, 2000)])
    intr = P.level_intrinsics(S.K, 4)
    pix = [(np.floor(fx * X[0] / X[2] + cx + 0.5), np.floor(fy * X[1] / X[2] + cy + 0.5)) for fx, fy, cx, cy in intr]
    for l in range(1, 4):  # level l's pixel j covers level l-1's pixels 2j and 2j + 1
        for axis in range(2):
            assert np.array_equal(pix[l][axis], np.floor(pix[l - 1][axis] / 2)), (l, axis)
        assert np.array_equal(pix[l][0], np.floor(pix[0][0] / 2 ** l))


def test_the_depth_gated_mean_and_the_normal_gate():
    d = np.array([[0.50, 0.51, 0.0, 0.60], [0.52, 0.90, 0.60, 0.60]], np.float32)
    out = P.downsample(d, 0.03)
    assert out.shape == (1, 2)
    assert out[0, 0] == np.float32((0.5 + float(np.float32(0.51)) + float(np.float32(0.52))) / 3.0)
    assert out[0, 1] == 0.0  # the top-left pixel is a hole
    step = np.full((6, 6), 0.5, np.float32)
    step[:, 3:] = 0.6
    n = P.normals(step, P.level_intrinsics(S.K, 1)[0], 0.03)
    assert not n[:, 2].any() and n[:5, :2].any() and n[:5, 3:5].any()


def test_restated_accuracy_on_the_noisy_scene():
    """five noisy uint16 frames, 48^3: the worst twist errors of strided tracking and of pyramid + filter + gate
    tracking, both pinned; the pyramid path is the closer one on both"""
    n, count = 48, 5
    frames = N.frames(count)
    truth = np.array([k * S.STEP for k in range(count)])

    def worst(twists):
        err = np.abs(np.array(twists) - truth)[1:]
        return err[:, :3].max(), err[:, 3:].max()

    _, _, stride_twists, _, _, _ = I.sequence(frames, S.K, N.RATIO, (n,) * 3, S.offset(n))
    _, _, pyramid_twists, recs = P.sequence(frames, S.K, N.RATIO, (n,) * 3, S.offset(n),
                                            cos_max=P.cos_of(MAX_NORMAL_ANGLE))
    assert [len(r) for r in recs] == [0, 14, 14, 14, 14]
    assert all(r["skipped"] == 0 for rs in recs for r in rs) and all(rs[-1]["angle_rejected"] > 0 for rs in recs[1:])
    np.testing.assert_allclose(worst(stride_twists), (STRIDE_WORST_T, STRIDE_WORST_R), rtol=2e-3)
    np.testing.assert_allclose(worst(pyramid_twists), (PYRAMID_WORST_T, PYRAMID_WORST_R), rtol=2e-3)
    assert PYRAMID_WORST_T < STRIDE_WORST_T and PYRAMID_WORST_R < STRIDE_WORST_R
