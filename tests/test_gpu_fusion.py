"""GPU checks of fusion into a canonical TSDF volume (csrc/lsf_fusion.hip, levelsetfusion_python_amd.fusion) against
the numpy restatement of the rule (tests/fusion_restatement.py), the rigid tracker's own live volume, and compositions
of the public pieces."""
import math

import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_scene as S
import rigid3d_restatement as R3
from test_gpu_rigid3d import _depth
from test_rigid3d_host import K_SYN

pytestmark = pytest.mark.gpu

SUM_RTOL, TWIST_ATOL = 1e-12, 1e-9
TWISTS = [np.zeros(6), np.array([0.013, -0.021, 0.008, 0.05, -0.17, 0.11]), np.array([-0.02, 0.01, 0.03, -0.06, 0.04, 0.09])]


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K_, ratio=0.001):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _host_record(r):
    from levelsetfusion_python_amd.device_fusion import unpack_record
    return unpack_record(r.cpu().numpy())


def _assert_record(got, want):
    assert got["fused"] == want["fused"] and got["first_seen"] == want["first_seen"]
    assert got["max_abs_change"] == want["max_abs_change"]
    np.testing.assert_allclose(got["sum_abs_change"], want["sum_abs_change"], rtol=SUM_RTOL, atol=0)


def _random_model(shape, rng, cap=8.0):
    """tsdf in [-1, 1] with a few exact +-1, weights 0, mid and at the cap"""
    t = rng.uniform(-1, 1, shape).astype(np.float32)
    t.reshape(-1)[::13] = 1.0
    w = rng.choice(np.array([0, 0, 1, 2.5, 5, cap], np.float32), shape)
    return t, w


def _random_live(shape, rng):
    l = rng.uniform(-1.3, 1.3, shape).astype(np.float32)
    flat = l.reshape(-1)
    flat[::7] = 1.0
    flat[::11] = -1.0
    flat[::17] = np.nan
    flat[::19] = np.nextafter(np.float32(1), np.float32(0))
    return l


@pytest.mark.parametrize("shape", [(64, 64, 64), (33, 17, 70), (129, 131), (5, 3, 3), (1, 3), (2, 2, 1)])
@pytest.mark.parametrize("w,cap", [(1.0, math.inf), (0.75, 8.0), (3.0, 4.0)])
def test_volume_mode_against_restatement(lsf, shape, w, cap):
    rng = np.random.default_rng(hash((shape, w)) % 2 ** 32)
    t, W = _random_model(shape, rng, cap if np.isfinite(cap) else 8.0)
    live = _random_live(shape, rng)
    vol = lsf.fusion.CanonicalVolume(shape, max_weight=cap)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(W))
    rec = vol.integrate_volume(live, weight=w)
    assert rec.dtype == torch.float64 and rec.is_cuda and rec.shape == (8,)
    want_t, want_w, want_rec = F.fuse(t, W, live, w, cap)
    assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
    host = rec.cpu().numpy()
    _assert_record(_host_record(rec), want_rec)
    assert not np.any(host[4:])


def test_volume_mode_unaligned_views(lsf):
    """buffers that are not 16-byte aligned take scalar accesses over the same voxel order: same bits, same record"""
    from levelsetfusion_python_amd import device_fusion
    rng = np.random.default_rng(5)
    n = 10001
    t, W = _random_model((n,), rng)
    live = _random_live((n,), rng)
    big = torch.empty(3 * (n + 1), dtype=torch.float32, device="cuda")
    tv, wv, lv = big[1:n + 1], big[n + 2:2 * n + 2], big[2 * n + 3:3 * n + 3]
    tv.copy_(torch.from_numpy(t)), wv.copy_(torch.from_numpy(W)), lv.copy_(torch.from_numpy(live))
    rec = device_fusion.integrate_volume(tv, wv, lv, 1.5, 6.0)
    want_t, want_w, want_rec = F.fuse(t, W, live, 1.5, 6.0)
    assert _bits_equal(tv.cpu().numpy(), want_t) and _bits_equal(wv.cpu().numpy(), want_w)
    _assert_record(_host_record(rec), want_rec)
    ta, wa, la = (torch.from_numpy(x.copy()).cuda() for x in (t, W, live))
    rec_a = device_fusion.integrate_volume(ta, wa, la, 1.5, 6.0)
    assert np.array_equal(rec_a.cpu().numpy(), rec.cpu().numpy())


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_depth_mode_equals_the_tracker_s_live_volume_fused(lsf, depth_dtype):
    from levelsetfusion_python_amd import device_fusion, device_rigid
    from levelsetfusion_python_amd.tsdf import generation as gen
    d = _depth(depth_dtype)
    cam = _camera(K_SYN)
    dev, code = gen.device_depth(d)
    rng = np.random.default_rng(7)
    for shape, off in (((40, 40, 40), np.array([-20.5, -20.25, 230.75])), ((33, 17, 70), np.array([-35.0, -8.5, 232.0]))):
        t, W = _random_model(shape, rng)
        for k, twist in enumerate(TWISTS):
            a_t, a_w = torch.from_numpy(t).cuda(), torch.from_numpy(W).cuda()
            b_t, b_w = a_t.clone(), a_w.clone()
            w, cap = (1.0, math.inf) if k == 0 else (0.5, 6.0)
            rec_a = device_fusion.integrate_depth(a_t, a_w, dev, code, cam, off, twist, w=w, max_weight=cap)
            live, _ = device_rigid.live_and_gradient_3d(dev, code, cam, shape, off, twist)
            rec_b = device_fusion.integrate_volume(b_t, b_w, live, w, cap)
            assert _bits_equal(a_t.cpu().numpy(), b_t.cpu().numpy()) and _bits_equal(a_w.cpu().numpy(),
                                                                                      b_w.cpu().numpy())
            assert np.array_equal(rec_a.cpu().numpy(), rec_b.cpu().numpy())
            want_t, want_w, want_rec = F.fuse_depth(t, W, d, K_SYN, 0.001, off, twist, 20, 0.004, w, cap)
            assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
            got = _host_record(rec_a)
            _assert_record(got, want_rec)
            assert got["fused"] > 1000


def test_canonical_volume_depth_from_numpy(lsf):
    d = _depth(np.float32)
    off = np.array([-16, -16, 234.5])
    vol = lsf.fusion.CanonicalVolume(32)
    rec = vol.integrate_depth(d, _camera(K_SYN), TWISTS[1], off)
    want_t, want_w, want_rec = F.fuse_depth(*F.empty_model((32, 32, 32)), d, K_SYN, 0.001, off, TWISTS[1])
    assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
    _assert_record(_host_record(rec), want_rec)
    assert want_rec["fused"] == want_rec["first_seen"] > 0
    vol.reset()
    assert torch.all(vol.tsdf == 1) and torch.all(vol.weight == 0)


def test_record_bit_identical_across_runs(lsf):
    from levelsetfusion_python_amd import device_fusion
    rng = np.random.default_rng(9)
    shape = (256, 256, 64)
    t, W = _random_model(shape, rng)
    live = torch.from_numpy(_random_live(shape, rng)).cuda()
    recs = []
    for _ in range(2):
        a_t, a_w = torch.from_numpy(t).cuda(), torch.from_numpy(W).cuda()
        recs.append(device_fusion.integrate_volume(a_t, a_w, live, 1.0, 5.0).cpu().numpy())
    assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64))


def test_host_refuses_bad_inputs(lsf):
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    t = torch.ones((8, 8, 8), device="cuda")
    w = torch.zeros((8, 8, 8), device="cuda")
    live = torch.zeros((8, 8, 8), device="cuda")
    with pytest.raises(ValueError, match="distinct"):
        device_fusion.integrate_volume(t, t, live)
    with pytest.raises(ValueError, match="distinct"):
        device_fusion.integrate_volume(t, t.view(-1).view(8, 8, 8), live)
    with pytest.raises(ValueError, match="alias"):
        device_fusion.integrate_volume(t, w, t)
    big = torch.zeros(1024, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        device_fusion.integrate_volume(big[:512].view(8, 8, 8), w, big[256:768].view(8, 8, 8))
    with pytest.raises(ValueError, match="one shape"):
        device_fusion.integrate_volume(t, w, torch.zeros((8, 8, 7), device="cuda"))
    with pytest.raises(ValueError, match="one shape"):
        device_fusion.integrate_volume(t, torch.zeros(512, device="cuda"), live)
    with pytest.raises(ValueError, match="float32"):
        device_fusion.integrate_volume(t, w, live.double())
    with pytest.raises(ValueError, match="float32"):
        device_fusion.integrate_volume(t.half(), w, live)
    with pytest.raises(ValueError, match="contiguous"):
        device_fusion.integrate_volume(t, w, live.transpose(0, 2))
    with pytest.raises(ValueError, match="GPU"):
        device_fusion.integrate_volume(t, w, live.cpu())
    with pytest.raises(ValueError, match="weight"):
        device_fusion.integrate_volume(t, w, live, w=0.0)
    with pytest.raises(ValueError, match="max_weight"):
        device_fusion.integrate_volume(t, w, live, max_weight=-1.0)
    dev, code = device_depth(np.full((8, 8), 600, np.uint16))
    t2, w2 = torch.ones((8, 8), device="cuda"), torch.zeros((8, 8), device="cuda")
    with pytest.raises(ValueError, match="3-D"):
        device_fusion.integrate_depth(t2, w2, dev, code, _camera(K_SYN), [0, 0, 0], np.zeros(6))
    with pytest.raises(ValueError, match="6 entries"):
        device_fusion.integrate_depth(t, w, dev, code, _camera(K_SYN), [0, 0, 0], np.zeros(3))
    with pytest.raises(ValueError, match="distinct"):
        device_fusion.integrate_depth(t, t, dev, code, _camera(K_SYN), [0, 0, 0], np.zeros(6))
    assert torch.all(t == 1) and torch.all(w == 0)  # nothing was launched


def _scene_camera():
    return _camera(S.K, 1.0)


def test_sequence_without_nonrigid_teacher_forced(lsf, capsys):
    """64^3, six frames of the analytic scene, 60 rigid iterations: every rigid iteration of a frame equals the restated
    tracker's step from the device's twist before it on the device's model (A and b to 1e-12 relative, the twist to
    1e-9), and each fusion equals the restatement bit for bit.
    The free-running twists do not follow the ground truth on this scene (tests/test_fusion_host.py::
    test_restated_sequence explains why); they are printed for the record."""
    n, count = 64, 6
    off = S.offset(n)
    frames = S.frames(count)
    seq = lsf.SequenceFusion3d(_scene_camera(), n, off)
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        assert rec["frame"] == k and rec["nonrigid"] is None and len(rec["rigid_records"]) == (60 if k else 0)
        twist = seq.twists[-1]
        if k == 0:
            assert np.array_equal(twist, np.zeros(6))
        else:  # every rigid iteration from the device's twist before it, on the device's model
            before = seq.twists[-2]
            for r in rec["rigid_records"]:
                want, after = R3.step(model_t, depth, S.K, 1.0, off, before, 20)
                assert r["skipped"] == want["skipped"]
                np.testing.assert_allclose(r["matrix_a"], want["A"], rtol=SUM_RTOL, atol=0)
                np.testing.assert_allclose(r["vector_b"].ravel(), want["b"], rtol=SUM_RTOL, atol=1e-300)
                np.testing.assert_allclose(r["twist"].ravel(), after, rtol=0, atol=TWIST_ATOL)
                before = r["twist"].ravel()
            assert np.array_equal(before, twist)
        model_t, model_w, want_rec = F.fuse_depth(model_t, model_w, depth, S.K, 1.0, off, twist)
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), model_w)
        _assert_record(rec["fusion"], want_rec)
    err = np.array([seq.twists[k] - S.true_twist(k) for k in range(count)])
    with capsys.disabled():
        print("\nfree-running twist error vs ground truth (m, rad):\n", np.array2string(err, precision=5))
    assert len(seq.frame_records) == count and len(seq.twists) == count


def test_sequence_rigid_iterations_zero_keeps_the_initial_twist(lsf):
    n = 32
    off = S.offset(n)
    start = np.array([0.001, 0.0, -0.002, 0.0, 0.01, 0.0])
    seq = lsf.SequenceFusion3d(_scene_camera(), n, off, rigid_iterations=0, initial_twist=start, max_weight=2.0)
    for depth in S.frames(3):
        seq.integrate(depth)
    assert all(np.array_equal(t, start) for t in seq.twists)
    assert all(r["rigid_records"] == [] for r in seq.frame_records)
    assert float(seq.canonical.weight.max()) == 2.0


def _slavcheva(lsf, n, iterations=4):
    return lsf.SlavchevaOptimizer3d(field_size=n, compute_method=lsf.ComputeMethod.DIRECT,
                                    smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                    level_set_term_enabled=True, maximum_warp_length_lower_threshold=0.0,
                                    max_iterations=iterations, min_iterations=iterations)


@pytest.mark.parametrize("rigid_iterations", [0, 10])
def test_sequence_with_nonrigid_equals_a_manual_composition(lsf, rigid_iterations):
    """one optimizer reused across frames equals, bit for bit, the public pieces with a fresh optimizer per frame"""
    from levelsetfusion_python_amd import device_rigid
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    n = 32
    off = S.offset(n)
    cam = _scene_camera()
    frames = S.frames(4)
    seq = lsf.SequenceFusion3d(cam, n, off, rigid_iterations=rigid_iterations, nonrigid_optimizer=_slavcheva(lsf, n))
    vol = lsf.fusion.CanonicalVolume(n)
    twist = np.zeros(6)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        dev, code = device_depth(depth)
        if k == 0:
            want = vol.integrate_depth(depth, cam, twist, off)
            assert rec["nonrigid"] is None
        else:
            if rigid_iterations:
                twist, _ = device_rigid.rigid_run_3d(vol.tsdf, dev, code, cam, off, rigid_iterations, 0.5, 0.01,
                                                     0.004, 0.004, 20, twist=twist)
            live, _ = device_rigid.live_and_gradient_3d(dev, code, cam, n, off, twist)
            _slavcheva(lsf, n).optimize(live, vol.tsdf)
            want = vol.integrate_volume(live)
            assert rec["nonrigid"] is not None and rec["nonrigid"].library_run in (True, False)
        assert np.array_equal(seq.twists[-1], twist)
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), vol.tsdf.cpu().numpy())
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), vol.weight.cpu().numpy())
        assert rec["fusion"] == _host_record(want)


def _band_error(model, t0):
    band = np.abs(t0) < 1
    return float(np.mean(np.abs(model[band] - t0[band])))


def test_nonrigid_step_on_a_deforming_sequence(lsf, capsys):
    """synthetic.depth_image frames whose bump moves 3 px a frame, poses fixed (no rigid step): the mean |model - frame 0
    TSDF| over frame 0's band, with and without a KillingFusion-style non-rigid step (20 iterations) before each fusion.
    The step was expected to bring the model closer to frame 0.  Measured on an MI355X, it does not: 0.0420 without it,
    0.0974 with it.  The optimizer warps each live volume towards the model, whose unobserved voxels behind the band
    hold +1 ("Fusion").  The test pins both numbers so that a change shows."""
    from levelsetfusion_python_amd import synthetic
    n = 48
    off = np.array([-n // 2, -n // 2, 250 - n // 2])
    frames = [synthetic.depth_image(shift_px=3.0 * k) for k in range(5)]
    cam = _camera(K_SYN)
    t0 = R3.live_volume(frames[0], K_SYN, 0.001, (n,) * 3, off, np.zeros(6))
    errors = {}
    for name, opt in (("rigid only", None), ("non-rigid", _slavcheva(lsf, n, 20))):
        seq = lsf.SequenceFusion3d(cam, n, off, rigid_iterations=0, nonrigid_optimizer=opt)
        for d in frames:
            seq.integrate(d)
        errors[name] = _band_error(seq.canonical.tsdf.cpu().numpy(), t0)
    with capsys.disabled():
        print("\nmean |model - frame-0 TSDF| over frame 0's band:", errors)
    np.testing.assert_allclose(errors["rigid only"], 0.042021144181489944, rtol=1e-3)
    np.testing.assert_allclose(errors["non-rigid"], 0.09738140553236008, rtol=1e-3)
