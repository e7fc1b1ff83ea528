"""GPU checks of projective point-to-plane ICP (csrc/lsf_icp.hip, rigid_opt.ProjectiveIcp3d) against the numpy
restatement (tests/icp_restatement.py), and of SequenceFusion3d(tracking_reference="icp") against the restated
sequence.  Per-pixel values (the residual image, the correspondence count) are compared bit for bit; A, b and the
energy are sums the device reduces in a tree, compared to 1e-12 of the sum of their terms' magnitudes (near
convergence the terms of b cancel to ~1e-3 of that scale, so a tolerance on the sum itself would measure the order of
the additions); twists to 1e-9."""

import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_scene as S
import icp_restatement as I
import raycast_restatement as RC
from test_icp_host import SEQUENCE_ATOL_R, SEQUENCE_ATOL_T

pytestmark = pytest.mark.gpu

SUM_RTOL, TWIST_ATOL = 1e-12, 1e-9
NON_CUBIC = ((40, 36, 52), np.array([-26.25, -18.0, 112.5]))
_PREDICTIONS = {}


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(ratio=1.0):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=ratio)


def _prediction(shape, off):
    """the model of frames 0 and 1 fused at their true twists, ray-cast with normals at frame 1's twist (restated)"""
    key = (shape, tuple(off))
    if key not in _PREDICTIONS:
        t, w = F.empty_model(shape)
        for k, depth in enumerate(S.frames(2)):
            t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k))
        pd, pn, _ = RC.raycast(t, w, S.K, S.true_twist(1), off, normals=True)
        _PREDICTIONS[key] = (pd, pn)
    return _PREDICTIONS[key]


def _live(dtype):
    """frame 2 in a live dtype and its ratio"""
    f = S.render(S.true_twist(2))
    if dtype == np.uint16:
        return np.round(f * 1000).astype(np.uint16), 0.001
    if dtype == np.float32:
        return f * np.float32(2), 0.5
    return f.astype(np.float64), 1.0


def _run(live, ratio, pd, pn, twist_p, twist, iterations, strides, residuals=False):
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    depth, code = device_depth(live)
    return device_icp.icp_run(depth, code, torch.from_numpy(pd).cuda(), torch.from_numpy(pn).cuda(), _camera(ratio),
                              twist_p, twist, iterations, strides, residuals=residuals)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_record(got, want):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"]
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    return r


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_one_iteration_against_restatement(lsf, stride):
    """residuals bit for bit (NaN where a pixel has no correspondence, or is off the stride), the count exactly"""
    off = S.offset(48)
    pd, pn = _prediction((48,) * 3, off)
    live, ratio = _live(np.float32)
    twist_p = S.true_twist(1)
    start = twist_p + np.array([0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
    twist, records, res = _run(live, ratio, pd, pn, twist_p, start, (1,), (stride,), residuals=True)
    want, want_res, after = I.iteration(live, pd, pn, S.K, ratio, start, twist_p, stride)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] > 1000
    assert _bits_equal(res.cpu().numpy(), want_res)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("volume", ["48", "128", "non-cubic"])
def test_pyramid_against_restatement(lsf, volume, dtype):
    shape, off = {"48": ((48,) * 3, S.offset(48)), "128": ((128,) * 3, S.offset(128)), "non-cubic": NON_CUBIC}[volume]
    pd, pn = _prediction(shape, off)
    live, ratio = _live(dtype)
    twist_p = S.true_twist(1)
    twist, records, _ = _run(live, ratio, pd, pn, twist_p, twist_p, I.ITERATIONS, I.STRIDES)
    want, want_twist = I.icp(live, pd, pn, S.K, ratio, twist_p)
    assert len(records) == len(want) == 14
    for got, w in zip(records, want):
        assert _check_record(got, w)["level"] == w["level"]
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert np.abs(twist - S.true_twist(2)).max() < 2e-3


def test_reruns_are_bit_identical(lsf):
    off = S.offset(48)
    pd, pn = _prediction((48,) * 3, off)
    live, ratio = _live(np.uint16)
    a = _run(live, ratio, pd, pn, S.true_twist(1), None, I.ITERATIONS, I.STRIDES, residuals=True)
    b = _run(live, ratio, pd, pn, S.true_twist(1), None, I.ITERATIONS, I.STRIDES, residuals=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy())


def test_projective_icp3d_interface(lsf):
    off = S.offset(48)
    pd, pn = _prediction((48,) * 3, off)
    live, ratio = _live(np.float64)
    tracker = lsf.ProjectiveIcp3d(_camera(ratio))
    twist = tracker.optimize(live, pd, pn, S.true_twist(1))
    want, want_twist = I.icp(live, pd, pn, S.K, ratio, S.true_twist(1))
    assert twist.shape == (6,) and twist.dtype == np.float64
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert [r["count"] for r in tracker.last_records] == [w["count"] for w in want]
    assert tracker.last_residuals is None
    empty = np.zeros_like(pd)
    start = S.true_twist(1) + 0.001
    still = lsf.ProjectiveIcp3d(_camera(ratio), iterations=(2,), strides=(1,)).optimize(
        live, empty, np.zeros_like(pn), S.true_twist(1), start, residuals=True)
    assert np.array_equal(still, start)


def test_sequence_icp_against_restatement(lsf, capsys):
    """48^3, five frames: each frame's ICP records (counts exact, twists to 1e-9) and the model (bit for bit) match
    the restated sequence, and the twists stay within the host test's bounds of the true ones"""
    n, count = 48, 5
    off = S.offset(n)
    frames = S.frames(count)
    seq = lsf.SequenceFusion3d(_camera(), n, off, tracking_reference="icp")
    _, _, twists, _, hits, icp = I.sequence(frames, S.K, 1.0, (n,) * 3, off)
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        assert rec["prediction_hits"] == hits[k]
        assert len(rec["rigid_records"]) == len(icp[k])
        for got, want in zip(rec["rigid_records"], icp[k]):
            assert got["count"] == want["count"] and got["level"] == want["level"]
            np.testing.assert_allclose(got["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
        np.testing.assert_allclose(seq.twists[-1], twists[k], rtol=0, atol=TWIST_ATOL)
        model_t, model_w, want_rec = F.fuse_depth(model_t, model_w, depth, S.K, 1.0, off, seq.twists[-1])
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), model_w)
        assert rec["fusion"]["fused"] == want_rec["fused"]
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(count)]))
    with capsys.disabled():
        print("\n\"icp\" tracking, |twist - truth| per frame (m, rad):\n", np.array2string(err, precision=6))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err


@pytest.mark.parametrize("mode", ["model", "raycast"])
def test_other_modes_ignore_the_icp_settings(lsf, mode):
    """the "model" and "raycast" paths do not read the ICP settings: sequences with and without them are equal bit
    for bit (their kernels' ISA is the parent's; tests/test_gpu_raycast.py and test_gpu_fusion.py pin their results)"""
    n = 32
    off = S.offset(n)
    a = lsf.SequenceFusion3d(_camera(), n, off, rigid_iterations=10, tracking_reference=mode)
    b = lsf.SequenceFusion3d(_camera(), n, off, rigid_iterations=10, tracking_reference=mode, icp_iterations=(1, 2),
                             icp_strides=(3, 1), icp_max_distance=0.5)
    for depth in S.frames(3):
        ra, rb = a.integrate(depth), b.integrate(depth)
        assert ra["fusion"] == rb["fusion"] and ra["prediction_hits"] == rb["prediction_hits"]
    assert all(np.array_equal(x, y) for x, y in zip(a.twists, b.twists))
    assert _bits_equal(a.canonical.tsdf.cpu().numpy(), b.canonical.tsdf.cpu().numpy())


def test_icp_sequence_without_iterations_keeps_the_twist(lsf):
    n = 32
    seq = lsf.SequenceFusion3d(_camera(), n, S.offset(n), tracking_reference="icp", icp_iterations=(0,),
                               icp_strides=(1,), initial_twist=S.true_twist(1))
    for depth in S.frames(2):
        rec = seq.integrate(depth)
        assert rec["rigid_records"] == [] and rec["prediction_hits"] is None
    assert all(np.array_equal(t, S.true_twist(1)) for t in seq.twists) and seq.prediction is None
