"""CPU checks of projective point-to-plane ICP: the numpy restatement (tests/icp_restatement.py) on the analytic scene
(tests/fusion_scene.py) against the true twists, its fixed points (zero motion, an empty prediction), the rotation log,
the ctypes layout of lsf_icp_params, the header's macros, the exports, the refusal of bad arguments and the no-CPU-path
error."""
import ctypes
import math
import os

import numpy as np
import pytest

import depth_pyramid_restatement as P
import fusion_restatement as F
import fusion_scene as S
import icp_restatement as I
import noisy_scene as N
import raycast_restatement as RC
from conftest import ROOT, load_golden
from rigid_restatement import rodrigues
from test_raycast_host import SEQUENCE_ATOL_R as RAYCAST_ATOL_R, SEQUENCE_ATOL_T as RAYCAST_ATOL_T

# the restated "icp" sequence, 48^3, five frames, iterations (4, 4, 6) at strides (4, 2, 1), 2 cm gate, measured: the
# largest translation error of a frame 0.047, 0.065, 0.080 and 0.093 mm, the largest rotation error 7.1e-4, 5.3e-4,
# 6.1e-4 and 6.2e-4 rad (frames 1-4).  At three times the scene's motion: 0.050, 0.068, 0.088 and 0.104 mm, 6.2e-4,
# 7.7e-4, 9.3e-4 and 8.3e-4 rad.  The bounds hold both.  "raycast" tracking errs by up to 7.1 mm and 1.4e-2 rad
# (tests/test_raycast_host.py::test_restated_raycast_sequence), 76x and 20x the worst "icp" frame.
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 2e-4, 1.5e-3
RAYCAST_WORST_T, RAYCAST_WORST_R = 7.10e-3, 1.394e-2


def _errors(twists, step):
    err = np.abs(np.array(twists) - np.array([k * step for k in range(len(twists))]))
    return err[1:, :3].max(axis=1), err[1:, 3:].max(axis=1)


def _check_sequence(step, want_t, want_r):
    n, count = 48, 5
    frames = [S.render(k * step) for k in range(count)]
    _, _, twists, records, hits, icp = I.sequence(frames, S.K, 1.0, (n,) * 3, S.offset(n))
    assert hits[0] is None and min(hits[1:]) > 40000
    assert [len(r) for r in icp] == [0, 14, 14, 14, 14]
    assert all(r["skipped"] == 0 for recs in icp for r in recs)
    assert [r["level"] for r in icp[1]] == [0] * 4 + [1] * 4 + [2] * 6
    assert all(recs[-1]["count"] > 30000 for recs in icp[1:])  # at stride 1
    err_t, err_r = _errors(twists, step)
    assert err_t.max() <= SEQUENCE_ATOL_T and err_r.max() <= SEQUENCE_ATOL_R, (err_t, err_r)
    np.testing.assert_allclose(err_t, want_t, rtol=0.02)
    np.testing.assert_allclose(err_r, want_r, rtol=0.02)
    return err_t, err_r


def test_restated_icp_sequence():
    """SequenceFusion3d(tracking_reference="icp") restated on the 48^3 five-frame scene: every frame within
    (SEQUENCE_ATOL_T, SEQUENCE_ATOL_R) of the true twist, at least 10x inside the pinned "raycast" errors"""
    err_t, err_r = _check_sequence(S.STEP, [4.727e-5, 6.528e-5, 8.002e-5, 9.313e-5],
                                   [7.105e-4, 5.296e-4, 6.128e-4, 6.207e-4])
    assert RAYCAST_WORST_T <= RAYCAST_ATOL_T and RAYCAST_WORST_R <= RAYCAST_ATOL_R
    assert 10 * err_t.max() <= RAYCAST_WORST_T and 10 * err_r.max() <= RAYCAST_WORST_R


def test_restated_icp_sequence_at_three_times_the_motion():
    """about 9 mm and 3 degrees per frame"""
    _check_sequence(3 * S.STEP, [4.959e-5, 6.845e-5, 8.788e-5, 1.0439e-4], [6.167e-4, 7.658e-4, 9.295e-4, 8.281e-4])


def _prediction(twist_p, n=48, frames=2):
    off = S.offset(n)
    t, w = F.empty_model((n,) * 3)
    for k, depth in enumerate(S.frames(frames)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
    pd, pn, _ = RC.raycast(t, w, S.K, twist_p, off, normals=True)
    return pd, pn


@pytest.mark.parametrize("twist_p", [np.zeros(6), np.array([2.0 ** -8, -2.0 ** -9, 2.0 ** -7, 0, 0, 0])])
def test_zero_motion_is_a_fixed_point(twist_p):
    """live = prediction at the prediction's twist: every residual is exactly 0, and so is every step.  The twists
    have no rotation and float32-exact translations, where the estimate's pose and the ray-cast's float32-rounded camera
    are the same matrix"""
    pd, pn = _prediction(twist_p)
    records, twist = I.icp(pd, pd, pn, S.K, 1.0, twist_p)
    assert np.abs(twist - twist_p).max() <= 1e-12
    for r in records:
        assert r["skipped"] == 0 and r["count"] > 1000 and r["energy"] <= 1e-24
    _, residuals, _ = I.iteration(pd, pd, pn, S.K, 1.0, twist_p, twist_p)
    lit = ~np.isnan(residuals)
    assert lit.sum() == records[-1]["count"] and not residuals[lit].any()


def test_empty_prediction_skips_every_iteration():
    pd, pn = np.zeros((48, 64), np.float32), np.zeros((48, 64, 3), np.float32)
    live = np.full((48, 64), 0.5, np.float32)
    start = np.array([0.001, 0.002, -0.003, 0.01, 0.0, -0.02])
    records, twist = I.icp(live, pd, pn, S.K, 1.0, np.zeros(6), start, (2, 1), (2, 1))
    assert np.array_equal(twist, start) and len(records) == 3
    for r in records:
        assert r["skipped"] == 1 and r["count"] == 0 and not r["A"].any() and not r["delta"].any()


PINNED_FIELDS = ("A", "b", "A_abs", "b_abs", "energy", "count", "delta", "twist", "skipped", "level")


def pinned_runs():
    """the arrays of tests/golden/ref_icp_restatement.npz: frame 1 of the noisy scene tracked from the zero twist
    against frame 0's 48^3 model, iterations (2, 2), by the strided restatement at strides (2, 1) and by the pyramid
    restatement over two levels without the gate and with a 20 degree gate.  Per run: the records' fields stacked over
    the iterations, the final twist and the last iteration's residual image"""
    n = 48
    frames = N.frames(2)
    tsdf, weight, _ = F.fuse_depth(*F.empty_model((n,) * 3), frames[0], S.K, N.RATIO, S.offset(n), np.zeros(6))
    pd, pn, _ = RC.raycast(tsdf, weight, S.K, np.zeros(6), S.offset(n), normals=True)
    live, zero = frames[1], np.zeros(6)
    out = {"hits": np.array(np.count_nonzero(pd))}

    def keep(name, records, twist, residuals, fields):
        for f in fields:
            out[name + "_" + f] = np.array([r[f] for r in records])
        out[name + "_final_twist"], out[name + "_residuals"] = twist, residuals

    records, twist = I.icp(live, pd, pn, S.K, N.RATIO, zero, zero, (2, 2), (2, 1))
    last, residuals, _ = I.iteration(live, pd, pn, S.K, N.RATIO, records[-2]["twist"], zero, 1)
    assert np.array_equal(last["twist"], twist)
    keep("strided", records, twist, residuals, PINNED_FIELDS)
    levels = P.pyramid(live, N.RATIO, S.K, levels=2)
    for name, cos_max in (("pyramid", None), ("gated", P.cos_of(math.radians(20)))):
        records, twist, residuals = P.icp(levels, pd, pn, S.K, zero, zero, (2, 2), cos_max=cos_max)
        keep(name, records, twist, residuals, PINNED_FIELDS + ("angle_rejected",))
    return out


def test_the_restatements_equal_their_pinned_results():
    """the oracle of every ICP GPU test, pinned: the strided and the pyramid restatement recompute the stored runs
    (tests/golden/make_golden_icp.py) bit for bit, NaNs in the same places"""
    want, got = load_golden("ref_icp_restatement.npz"), pinned_runs()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert np.array_equal(want[name], got[name], equal_nan=want[name].dtype.kind == "f"), name
    assert got["hits"] == 44447
    assert got["strided_count"].tolist() == [8753, 9004, 35942, 35920]
    assert got["pyramid_count"].tolist() == [8767, 8938, 35924, 35935]
    assert got["gated_count"].tolist() == [6584, 8395, 33074, 33120]
    assert got["gated_angle_rejected"].tolist() == [2183, 581, 2849, 2830]


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 0.3, 1.0, 2.0, 2.5, 3.0])
def test_log_inverts_rodrigues(angle):
    rng = np.random.default_rng(int(angle * 1000) + 1)
    for _ in range(5):
        axis = rng.normal(size=3)
        r = axis / np.linalg.norm(axis) * angle
        np.testing.assert_allclose(I.log_rotation(rodrigues(r)), r, rtol=0, atol=1e-12)


def test_compose_is_the_left_perturbation():
    """g' = R'^T (v - t') equals exp(omega) R^T (v - t) + tau for the composed twist"""
    twist = np.array([0.01, -0.02, 0.005, 0.1, -0.2, 0.05])
    delta = np.array([0.002, 0.001, -0.003, 0.01, 0.02, -0.015])
    new = I.compose(twist, delta)
    v = np.array([0.1, -0.05, 0.6])
    g = rodrigues(twist[3:]).T @ (v - twist[:3])
    want = rodrigues(delta[3:]) @ g + delta[:3]
    np.testing.assert_allclose(rodrigues(new[3:]).T @ (v - new[:3]), want, rtol=0, atol=1e-15)


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.IcpParams
    assert [f[0] for f in p._fields_] == ["fx", "fy", "cx", "cy", "depth_unit_ratio", "max_distance", "twist_p",
                                          "height", "width", "depth_dtype", "levels", "iterations", "strides"]
    assert ctypes.sizeof(p) == 12 * 8 + 4 * 4 + 2 * 4 * 4 and p.height.offset == 96 and p.strides.offset == 128
    assert (lib.ICP_MAX_LEVELS, lib.ICP_RECORD_DOUBLES, lib.ICP_MAX_BLOCKS) == (4, 64, 256)
    assert lib.ICP_SCRATCH_BYTES == 2 * 256 * 29 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for macro, value in (("LSF_ICP_MAX_LEVELS", "4"), ("LSF_ICP_RECORD_DOUBLES", "64"), ("LSF_ICP_MAX_BLOCKS", "256"),
                         ("LSF_ICP_SCRATCH_BYTES", "(2 * LSF_ICP_MAX_BLOCKS * 29 * 8)")):
        assert "#define %s %s" % (macro, value) in header
    assert "#define LSF_ABI_VERSION 4" in header and lib.ABI_VERSION == 4
    assert "lsf_icp_run" in lib.PROTOTYPES and lib.lib.lsf_icp_run is not None


def _good_params():
    import levelsetfusion_python_amd._lib as lib
    p = lib.IcpParams()
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance = 70.0, 70.0, 32.0, 24.0, 0.001, 0.02
    p.height, p.width, p.depth_dtype, p.levels = 48, 64, lib.DEPTH_U16, 2
    p.iterations[:2] = [2, 3]
    p.strides[:2] = [2, 1]
    return p


def test_the_c_abi_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    f = lib.lib.lsf_icp_run
    p = _good_params()
    # never dereferenced: every call below is refused on the host.  The fake buffers are 1 MiB apart, so only the
    # cases built to alias do.
    live, pd, pn, tw, rec, sc, res = (ctypes.c_void_p((1 << 20) * k) for k in (1, 2, 3, 4, 5, 6, 7))
    for field, value in (("height", 0), ("width", -1), ("height", 1 << 16), ("fx", 0.0), ("fy", math.nan),
                         ("cx", math.inf), ("depth_unit_ratio", math.nan), ("max_distance", 0.0),
                         ("max_distance", -0.01), ("max_distance", math.nan), ("depth_dtype", 3),
                         ("depth_dtype", -1), ("levels", 0), ("levels", 5)):
        q = lib.IcpParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "height" and value == 1 << 16:
            q.width = 1 << 16  # 2^32 pixels
        assert f(live, pd, pn, tw, rec, sc, None, ctypes.byref(q), None) == -1, (field, value)
    for edit in (lambda q: q.strides.__setitem__(1, 0), lambda q: q.strides.__setitem__(0, -2),
                 lambda q: q.iterations.__setitem__(0, -1), lambda q: q.twist_p.__setitem__(4, math.nan)):
        q = lib.IcpParams.from_buffer_copy(p)
        edit(q)
        assert f(live, pd, pn, tw, rec, sc, None, ctypes.byref(q), None) == -1
    P = ctypes.byref(p)
    for args in ((None, pd, pn, tw, rec, sc, None), (live, None, pn, tw, rec, sc, None),
                 (live, pd, None, tw, rec, sc, None), (live, pd, pn, None, rec, sc, None),
                 (live, pd, pn, tw, None, sc, None), (live, pd, pn, tw, rec, None, None),
                 (live, pd, pn, live, rec, sc, None),      # the twist aliases the live image
                 (live, pd, pn, tw, pn, sc, None),         # records alias the normals
                 (live, pd, pn, tw, rec, rec, None),       # scratch aliases the records
                 (live, pd, pn, tw, rec, sc, pd),          # residuals alias the prediction
                 (live, pd, pn, tw, rec, sc, sc)):         # residuals alias the scratch
        assert f(*args, P, None) == -1, args
    assert f(live, pd, pn, tw, rec, sc, None, None, None) == -1
    near = ctypes.c_void_p((1 << 20) * 2 + 4 * 48 * 64 - 4)  # the last float of the prediction's depth
    assert f(live, pd, pn, tw, rec, sc, near, P, None) == -1
    q = lib.IcpParams.from_buffer_copy(p)
    q.iterations[0] = q.iterations[1] = 0
    assert f(live, pd, pn, tw, None, sc, None, ctypes.byref(q), None) == 0  # nothing to launch


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    p = device_icp.params(cam, (480, 640), np.arange(6) * 0.01, 0)
    assert (p.height, p.width, p.levels, list(p.iterations), list(p.strides)) == (480, 640, 3, [4, 4, 6, 0],
                                                                                   [4, 2, 1, 0])
    assert (p.fx, p.cx, p.depth_unit_ratio, p.max_distance, p.twist_p[5]) == (700.0, 320.0, 0.001, 0.02, 0.05)
    for bad in (dict(iterations=(1, 2), strides=(1,)), dict(iterations=(1,) * 5, strides=(1,) * 5),
                dict(iterations=(-1,), strides=(1,)), dict(iterations=(1,), strides=(0,)), dict(max_distance=0.0),
                dict(max_distance=math.nan), dict(twist_p=np.zeros(3)), dict(twist_p=[0, 0, 0, 0, math.inf, 0]),
                dict(image_shape=(0, 4))):
        kw = dict(camera=cam, image_shape=(48, 64), twist_p=np.zeros(6), depth_code=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            device_icp.params(**kw)


def test_package_exports_icp():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_icp, fusion, rigid_opt
    assert lsf.ProjectiveIcp3d is rigid_opt.ProjectiveIcp3d and "ProjectiveIcp3d" in lsf.__all__
    assert callable(device_icp.icp_run)
    assert fusion.TRACKING_MODES == ("model", "raycast", "icp")
    assert "icp" in fusion.__doc__ and "point-to-plane" in fusion.__doc__
    t = lsf.ProjectiveIcp3d(None, iterations=(3, 2), strides=(2, 1), max_distance=0.05)
    assert (t.iterations, t.strides, t.max_distance, t.last_records) == ((3, 2), (2, 1), 0.05, [])
    with pytest.raises(ValueError):
        lsf.ProjectiveIcp3d(None, max_distance=0)


def test_no_cpu_path():
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    z = torch.zeros((4, 4))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        device_icp.icp_run(z, 1, z, torch.zeros((4, 4, 3)), cam, np.zeros(6))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        lsf.ProjectiveIcp3d(cam).optimize(np.ones((4, 4), np.float32), z, torch.zeros((4, 4, 3)), np.zeros(6))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        lsf.fusion.SequenceFusion3d(cam, 8, [0, 0, 100], tracking_reference="icp")
