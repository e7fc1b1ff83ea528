"""GPU checks of the live depth pyramid (csrc/lsf_depth_pyramid.hip, rigid_opt.DepthPyramid) and of ICP over it
(lsf_icp_run_pyramid, ProjectiveIcp3d(pyramid=...), SequenceFusion3d(icp_pyramid=...)) against the numpy restatement
(tests/depth_pyramid_restatement.py).  The filtered level 0 is compared to 1 float32 ulp (the device's float64 exp and
numpy's may differ in the last bit); the coarser levels and the normals, restated from the device's own level 0, bit
for bit.  ICP: the residual image, the correspondence count and the gate's rejections bit for bit, A, b and the energy
to 1e-12 of their terms' magnitudes, twists to 1e-9, the tolerances of tests/test_gpu_icp.py."""
import os

import numpy as np
import pytest
import torch

import depth_pyramid_restatement as P
import fusion_restatement as F
import fusion_scene as S
import noisy_scene as N
import raycast_restatement as RC
from test_depth_pyramid_host import MAX_NORMAL_ANGLE

pytestmark = pytest.mark.gpu

SUM_RTOL, TWIST_ATOL = 1e-12, 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_PREDICTION = {}


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(ratio):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=ratio)


def _frame(kind):
    """(depth image, ratio) of a test input"""
    noisy = N.render(S.true_twist(2), seed=2)
    if kind == "uint16":
        return noisy, N.RATIO
    if kind == "float32":
        return (noisy * np.float32(0.002)).astype(np.float32), 0.5
    if kind == "float64":
        return noisy * 0.001, 1.0
    from levelsetfusion_python_amd import image_io
    return image_io.read_depth_image(os.path.join(GOLDEN, "depth_000000.exr")), 0.001


def _build(lsf, depth, ratio, **settings):
    pyr = lsf.rigid_opt.DepthPyramid(**settings)
    out = pyr.build(depth, _camera(ratio))
    return pyr, [d.cpu().numpy() for d in out.depth], [n.cpu().numpy() for n in out.normals], out


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kind", ["uint16", "float32", "float64", "exr"])
@pytest.mark.parametrize("radius", [3, 0])
def test_pyramid_against_restatement(lsf, kind, radius):
    depth, ratio = _frame(kind)
    _, depths, normals, out = _build(lsf, depth, ratio, radius=radius)
    want0 = P.bilateral(depth, ratio, radius)
    got0 = depths[0]
    assert np.array_equal(got0 > 0, want0 > 0) and np.array_equal(got0 == 0, want0 == 0)
    ulps = np.abs(got0.view(np.int32).astype(np.int64) - want0.view(np.int32).astype(np.int64))
    assert ulps.max() <= (1 if radius else 0), ulps.max()
    want_d, want_n, want_k = P.pyramid_from_level0(got0, S.K, 3)
    assert [d.shape for d in depths] == [(480, 640), (240, 320), (120, 160)]
    for l in range(3):
        assert _bits_equal(depths[l], want_d[l]), l
        assert _bits_equal(normals[l], want_n[l]), l
        assert tuple(out.intrinsics[l]) == want_k[l]
    assert normals[0].any() and (depths[2] > 0).any()


def test_pyramid_reruns_are_bit_identical(lsf):
    depth, ratio = _frame("uint16")
    a, b = _build(lsf, depth, ratio)[3], _build(lsf, depth, ratio)[3]
    assert _bits_equal(a.buffers[0].cpu().numpy(), b.buffers[0].cpu().numpy())
    assert _bits_equal(a.buffers[1].cpu().numpy(), b.buffers[1].cpu().numpy())


def _prediction(n=48):
    """the model of noisy frames 0 and 1 fused at their true twists, ray-cast with normals at frame 1's twist"""
    if n not in _PREDICTION:
        off = S.offset(n)
        t, w = F.empty_model((n,) * 3)
        for k, depth in enumerate(N.frames(2)):
            t, w, _ = F.fuse_depth(t, w, depth, S.K, N.RATIO, off, S.true_twist(k))
        pd, pn, _ = RC.raycast(t, w, S.K, S.true_twist(1), off, normals=True)
        _PREDICTION[n] = (pd, pn)
    return _PREDICTION[n]


def _check_record(got, want, level):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"] and r["level"] == level
    assert r["angle_rejected"] == want["angle_rejected"]
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)


def _run_pyramid_icp(lsf, gate, iterations=(4, 4, 6), residuals=True):
    from levelsetfusion_python_amd import device_icp
    pd, pn = _prediction()
    depth, ratio = _frame("uint16")
    _, depths, normals, out = _build(lsf, depth, ratio)
    twist_p = S.true_twist(1)
    angle = MAX_NORMAL_ANGLE if gate else None
    got = device_icp.icp_run_pyramid(*out.buffers, 3, torch.from_numpy(pd).cuda(), torch.from_numpy(pn).cuda(),
                                     _camera(ratio), twist_p, twist_p, iterations, max_normal_angle=angle,
                                     residuals=residuals)
    levels = (depths, normals, out.intrinsics)
    want = P.icp(levels, pd, pn, S.K, twist_p, twist_p, iterations, cos_max=P.cos_of(angle) if gate else None)
    return got, want


@pytest.mark.parametrize("gate", [True, False])
def test_pyramid_icp_against_restatement(lsf, gate):
    (twist, records, res), (want, want_twist, want_res) = _run_pyramid_icp(lsf, gate)
    assert len(records) == len(want) == 14
    for got, w in zip(records, want):
        _check_record(got, w, w["level"])
    assert (want[-1]["angle_rejected"] > 0) == gate and want[-1]["count"] > 30000
    assert _bits_equal(res.cpu().numpy(), want_res)
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert np.abs(twist - S.true_twist(2)).max() < 3e-3


def test_pyramid_icp_residuals_have_the_last_level_s_extents(lsf):
    (_, records, res), (want, _, want_res) = _run_pyramid_icp(lsf, True, iterations=(2, 3, 0))
    assert res.shape == (240, 320) and len(records) == 5
    assert _bits_equal(res.cpu().numpy(), want_res)
    for got, w in zip(records, want):
        _check_record(got, w, w["level"])


def test_pyramid_icp_reruns_are_bit_identical(lsf):
    a, _ = _run_pyramid_icp(lsf, True)
    b, _ = _run_pyramid_icp(lsf, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy())


def test_projective_icp3d_with_a_pyramid(lsf):
    pd, pn = _prediction()
    depth, ratio = _frame("uint16")
    pyr = lsf.rigid_opt.DepthPyramid()
    tracker = lsf.ProjectiveIcp3d(_camera(ratio), pyramid=pyr, max_normal_angle=MAX_NORMAL_ANGLE)
    twist = tracker.optimize(depth, pd, pn, S.true_twist(1), residuals=True)
    levels = (P.pyramid_from_level0(tracker.last_pyramid.depth[0].cpu().numpy(), S.K, 3)[:2]
              + (tracker.last_pyramid.intrinsics,))
    want, want_twist, _ = P.icp(levels, pd, pn, S.K, S.true_twist(1), cos_max=P.cos_of(MAX_NORMAL_ANGLE))
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert [r["count"] for r in tracker.last_records] == [w["count"] for w in want]
    assert [r["angle_rejected"] for r in tracker.last_records] == [w["angle_rejected"] for w in want]
    assert tracker.last_residuals.shape == (480, 640)


def test_no_pyramid_is_today_s_tracker(lsf):
    """pyramid=None gives the twists and records of a tracker built without the new arguments, bit for bit"""
    pd, pn = _prediction()
    depth, ratio = _frame("uint16")
    a = lsf.ProjectiveIcp3d(_camera(ratio))
    b = lsf.ProjectiveIcp3d(_camera(ratio), pyramid=None, max_normal_angle=None)
    ta, tb = a.optimize(depth, pd, pn, S.true_twist(1)), b.optimize(depth, pd, pn, S.true_twist(1))
    assert np.array_equal(ta, tb) and b.last_pyramid is None
    for ra, rb in zip(a.last_records, b.last_records):
        assert all(np.array_equal(ra[k], rb[k]) for k in ra) and rb["angle_rejected"] == 0


def test_sequence_with_a_pyramid_against_restatement(lsf, capsys):
    """48^3, five noisy frames: each frame's ICP records (counts and rejections exact, twists to 1e-9) and the model
    (bit for bit: fusion integrates the raw depth) match the restated sequence"""
    n, count = 48, 5
    off = S.offset(n)
    frames = N.frames(count)
    pyr = lsf.rigid_opt.DepthPyramid()
    seq = lsf.SequenceFusion3d(_camera(N.RATIO), n, off, tracking_reference="icp", icp_pyramid=pyr,
                               icp_max_normal_angle=MAX_NORMAL_ANGLE)
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        twist_before = seq.twists[-1] if k else None
        rec = seq.integrate(depth)
        if k:
            # restated from the device's own level 0 of this frame (the filter's exp may differ in the last bit)
            pd, pn, hits = RC.raycast(model_t, model_w, S.K, twist_before, off, 0.004, depth.shape, normals=True)
            assert rec["prediction_hits"] == hits
            level0 = pyr.build(depth, _camera(N.RATIO)).depth[0].cpu().numpy()
            levels = P.pyramid_from_level0(level0, S.K, 3)
            want, want_twist, _ = P.icp(levels, pd, pn, S.K, twist_before, twist_before,
                                        cos_max=P.cos_of(MAX_NORMAL_ANGLE))
            assert len(rec["rigid_records"]) == len(want) == 14
            for got, w in zip(rec["rigid_records"], want):
                assert got["count"] == w["count"] and got["angle_rejected"] == w["angle_rejected"]
                np.testing.assert_allclose(got["twist"].ravel(), w["twist"], rtol=0, atol=TWIST_ATOL)
            np.testing.assert_allclose(seq.twists[-1], want_twist, rtol=0, atol=TWIST_ATOL)
        model_t, model_w, want_rec = F.fuse_depth(model_t, model_w, depth, S.K, N.RATIO, off, seq.twists[-1])
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
        assert rec["fusion"]["fused"] == want_rec["fused"]
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(count)]))
    with capsys.disabled():
        print("\n\"icp\" + pyramid on the noisy scene, |twist - truth| per frame (m, rad):\n",
              np.array2string(err, precision=6))
    assert err[1:, :3].max() < 1e-3 and err[1:, 3:].max() < 3e-3
