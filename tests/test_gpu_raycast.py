"""GPU checks of ray-casting the canonical TSDF (csrc/lsf_raycast.hip, fusion.CanonicalVolume.raycast) against the numpy
restatement (tests/raycast_restatement.py), and of SequenceFusion3d(tracking_reference="raycast") against the restated
tracker and fusion rule."""

import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_scene as S
import raycast_restatement as RC
import rigid3d_restatement as R3
from test_raycast_host import SEQUENCE_ATOL_R, SEQUENCE_ATOL_T

pytestmark = pytest.mark.gpu

SUM_RTOL, TWIST_ATOL = 1e-12, 1e-9
SMALL_K = np.array([[140.0, 0, 64], [0, 140.0, 48], [0, 0, 1]], np.float32)  # 128 x 96, the scene camera's view
TWISTS = [np.zeros(6), S.true_twist(1), np.array([-0.004, 0.003, 0.001, -0.02, 0.015, -0.01]),
          # a camera left of the volume, turned towards it: 59 % of the rays that hit enter through the x = 0 face
          np.array([0.3845, -0.01, -0.0684, 0.0, -0.7, 0.0])]


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K_, ratio=1.0):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _fused(shape, off, frames=3, max_weight=np.inf):
    t, w = F.empty_model(shape)
    for k, depth in enumerate(S.frames(frames)):
        t, w, _ = F.fuse_depth(t, w, depth, S.K, 1.0, off, S.true_twist(k), max_weight=max_weight)
    return t, w


def _volume(lsf, t, w):
    vol = lsf.fusion.CanonicalVolume(t.shape)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(w))
    return vol


def _check(vol, t, w, K_, twist, off, shape, fallback=None, ratio=1.0, min_hits=1):
    from levelsetfusion_python_amd import device_raycast
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    fb, code = (None, None) if fallback is None else device_depth(fallback)
    depth, normals, hits = device_raycast.raycast(vol.tsdf, vol.weight, _camera(K_, ratio), twist, off,
                                                  image_shape=shape, normals=True, fallback_depth=fb,
                                                  fallback_code=code)
    want_d, want_n, want_h = RC.raycast(t, w, K_, twist, off, image_shape=shape, normals=True, fallback=fallback,
                                        ratio=ratio)
    assert int(hits.item()) == want_h >= min_hits
    assert _bits_equal(depth.cpu().numpy(), want_d)
    assert _bits_equal(normals.cpu().numpy(), want_n)
    alone, none, _ = device_raycast.raycast(vol.tsdf, vol.weight, _camera(K_, ratio), twist, off, image_shape=shape,
                                            fallback_depth=fb, fallback_code=code)
    assert none is None and _bits_equal(alone.cpu().numpy(), want_d)  # the normals change nothing else
    return want_h


@pytest.mark.parametrize("k", range(len(TWISTS)))
def test_scene_model_against_restatement(lsf, k):
    off = S.offset(48)
    t, w = _fused((48,) * 3, off)
    _check(_volume(lsf, t, w), t, w, S.K, TWISTS[k], off, (480, 640), min_hits=10000)


def test_non_cubic_volume_and_a_small_image(lsf):
    shape = (40, 36, 52)
    off = np.array([-26.25, -18.0, 112.5])
    t, w = _fused(shape, off)
    vol = _volume(lsf, t, w)
    for twist in TWISTS[:3]:
        _check(vol, t, w, SMALL_K, twist, off, (96, 128), min_hits=500)
    _check(vol, t, w, S.K, TWISTS[1], off, (480, 640), min_hits=10000)
    odd_k = np.array([[60.0, 0, 26], [0, 60.0, 18], [0, 0, 1]], np.float32)  # 53 x 37: not a multiple of the tile
    _check(vol, t, w, odd_k, TWISTS[2], off, (37, 53), min_hits=100)


def test_capped_and_empty_models(lsf):
    off = S.offset(48)
    t, w = _fused((48,) * 3, off, frames=4, max_weight=2.0)
    assert w.max() == 2.0
    _check(_volume(lsf, t, w), t, w, S.K, TWISTS[2], off, (480, 640), min_hits=10000)
    vol = lsf.fusion.CanonicalVolume(48)  # tsdf 1, weight 0: no valid sample anywhere
    e_t, e_w = F.empty_model((48,) * 3)
    from levelsetfusion_python_amd import device_raycast
    depth, normals, hits = device_raycast.raycast(vol.tsdf, vol.weight, _camera(S.K), TWISTS[1], off, normals=True)
    assert int(hits.item()) == 0 and not depth.any() and not normals.any()
    want_d, want_n, want_h = RC.raycast(e_t, e_w, S.K, TWISTS[1], off, normals=True)
    assert want_h == 0 and _bits_equal(depth.cpu().numpy(), want_d) and _bits_equal(normals.cpu().numpy(), want_n)
    zero = np.zeros_like(e_t)  # tsdf 0 with weight 1: valid samples, never a sign change from > 0
    _check(_volume(lsf, zero, np.ones_like(e_w)), zero, np.ones_like(e_w), S.K, TWISTS[0], off, (48, 64),
           min_hits=0)


@pytest.mark.parametrize("dtype,ratio", [(np.uint16, 0.001), (np.float32, 1.0), (np.float32, 0.5), (np.float64, 0.25)])
def test_fallback_images(lsf, dtype, ratio):
    off = S.offset(48)
    t, w = _fused((48,) * 3, off, frames=2)
    rng = np.random.default_rng(3)
    if dtype == np.uint16:
        fb = rng.integers(0, 2000, (480, 640)).astype(np.uint16)
    else:
        fb = rng.uniform(0.0, 2.0, (480, 640)).astype(dtype)
    _check(_volume(lsf, t, w), t, w, S.K, TWISTS[1], off, (480, 640), fallback=fb, ratio=ratio, min_hits=10000)


def test_canonical_volume_raycast_interface(lsf):
    from levelsetfusion_python_amd import device_raycast
    off = S.offset(32)
    t, w = _fused((32,) * 3, off, frames=1)
    vol = _volume(lsf, t, w)
    cam = _camera(SMALL_K)
    want_d, want_n, want_h = RC.raycast(t, w, SMALL_K, np.zeros(6), off, image_shape=(96, 128), normals=True)
    d = vol.raycast(cam, np.zeros(6), off, image_shape=(96, 128))
    assert isinstance(d, np.ndarray) and _bits_equal(d, want_d)
    d_t, n_t = vol.raycast(cam, np.zeros(6), off, image_shape=(96, 128), normals=True, as_tensor=True)
    assert d_t.is_cuda and n_t.shape == (96, 128, 3)
    assert _bits_equal(d_t.cpu().numpy(), want_d) and _bits_equal(n_t.cpu().numpy(), want_n)
    fb = np.full((96, 128), 7.0, np.float32)
    filled = vol.raycast(cam, np.zeros(6), off, image_shape=(96, 128), fallback_depth=fb)
    assert np.all(filled[want_d == 0] == 7.0) and _bits_equal(filled[want_d > 0], want_d[want_d > 0])
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for _ in range(2):  # the count is added to
        device_raycast.raycast(vol.tsdf, vol.weight, cam, np.zeros(6), off, image_shape=(96, 128), hit_count=count)
    assert int(count.item()) == 2 * want_h > 0
    with pytest.raises(ValueError, match="shape"):
        vol.raycast(cam, np.zeros(6), off, image_shape=(96, 128), fallback_depth=np.zeros((96, 127), np.float32))
    with pytest.raises(ValueError, match="3-D"):
        lsf.fusion.CanonicalVolume((8, 8)).raycast(cam, np.zeros(6), off)
    with pytest.raises(ValueError, match="image_shape"):
        vol.raycast(cam, np.zeros(6), off, image_shape=(0, 128))


def test_sequence_raycast_teacher_forced(lsf, capsys):
    """48^3, five frames of the analytic scene, 60 rigid iterations, tracking_reference="raycast": each frame's
    prediction equals the restated ray-cast of the device's model at the device's previous twist bit for bit; every
    rigid iteration equals the restated tracker's step against that prediction's live volume (A and b to 1e-12 of
    their largest entry: some entries of A cancel to 1e-12 relative of it, and the device sums in a tree; the twist to
    1e-9); each fusion equals the restatement bit for bit.  The free-running twists stay within
    the CPU test's bounds of the true ones."""
    n, count = 48, 5
    off = S.offset(n)
    frames = S.frames(count)
    seq = lsf.SequenceFusion3d(_camera(S.K), n, off, tracking_reference="raycast")
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        twist = seq.twists[-1]
        if k == 0:
            assert rec["prediction_hits"] is None and seq.prediction is None
        else:
            before = seq.twists[-2]
            want_d, _, want_h = RC.raycast(model_t, model_w, S.K, before, off, fallback=frames[k - 1])
            assert rec["prediction_hits"] == want_h > 40000
            assert _bits_equal(seq.prediction.cpu().numpy(), want_d)
            reference = R3.live_volume(want_d, S.K, 1.0, (n,) * 3, off, before)
            assert len(rec["rigid_records"]) == 60
            for r in rec["rigid_records"]:
                want, after = R3.step(reference, depth, S.K, 1.0, off, before, 20)
                assert r["skipped"] == want["skipped"]
                scale_a, scale_b = np.abs(want["A"]).max(), np.abs(want["b"]).max()
                np.testing.assert_allclose(r["matrix_a"], want["A"], rtol=0, atol=SUM_RTOL * scale_a)
                np.testing.assert_allclose(r["vector_b"].ravel(), want["b"], rtol=0, atol=SUM_RTOL * scale_b)
                np.testing.assert_allclose(r["twist"].ravel(), after, rtol=0, atol=TWIST_ATOL)
                before = r["twist"].ravel()
            assert np.array_equal(before, twist)
        model_t, model_w, want_rec = F.fuse_depth(model_t, model_w, depth, S.K, 1.0, off, twist)
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), model_w)
        assert rec["fusion"]["fused"] == want_rec["fused"] and rec["fusion"]["first_seen"] == want_rec["first_seen"]
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(count)]))
    with capsys.disabled():
        print("\n\"raycast\" tracking, |twist - truth| per frame (m, rad):\n", np.array2string(err, precision=5))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err


def test_model_reference_is_the_default_bit_for_bit(lsf):
    n = 32
    off = S.offset(n)
    a = lsf.SequenceFusion3d(_camera(S.K), n, off, rigid_iterations=20)
    b = lsf.SequenceFusion3d(_camera(S.K), n, off, rigid_iterations=20, tracking_reference="model")
    for depth in S.frames(4):
        ra, rb = a.integrate(depth), b.integrate(depth)
        assert ra["fusion"] == rb["fusion"] and rb["prediction_hits"] is None
    assert all(np.array_equal(x, y) for x, y in zip(a.twists, b.twists))
    assert _bits_equal(a.canonical.tsdf.cpu().numpy(), b.canonical.tsdf.cpu().numpy())
    assert _bits_equal(a.canonical.weight.cpu().numpy(), b.canonical.weight.cpu().numpy())
    assert b.prediction is None
    with pytest.raises(ValueError, match="tracking_reference"):
        lsf.SequenceFusion3d(_camera(S.K), n, off, tracking_reference="frame")


def test_raycast_sequence_with_uint16_frames_and_no_rigid_step(lsf):
    """the fallback is the previous frame in its own dtype and units; rigid_iterations=0 casts nothing"""
    n = 32
    off = S.offset(n)
    frames = [np.round(f * 1000).astype(np.uint16) for f in S.frames(3)]
    cam = _camera(S.K, 0.001)
    seq = lsf.SequenceFusion3d(cam, n, off, rigid_iterations=5, tracking_reference="raycast")
    still = lsf.SequenceFusion3d(cam, n, off, rigid_iterations=0, tracking_reference="raycast")
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        seq.integrate(depth)
        assert still.integrate(depth)["prediction_hits"] is None
        if k:
            want_d, _, _ = RC.raycast(model_t, model_w, S.K, seq.twists[-2], off, fallback=frames[k - 1], ratio=0.001)
            assert _bits_equal(seq.prediction.cpu().numpy(), want_d)
        model_t, model_w, _ = F.fuse_depth(model_t, model_w, depth, S.K, 0.001, off, seq.twists[-1])
    assert still.prediction is None and all(np.array_equal(t, np.zeros(6)) for t in still.twists)
