"""GPU checks of weighted depth-mode fusion with free-space carving (lsf_fusion_integrate_depth_weighted in
csrc/lsf_fusion.hip) and of the depth confidence image (csrc/lsf_depth_confidence.hip) against the unweighted entry
point, the numpy restatement (tests/fusion_weighted_restatement.py) and compositions of the public pieces.  tsdf, weight
and the confidence image are compared bit for bit, the record's counts and maximum exactly, and its float64 sum to the
1e-12 relative of tests/fusion_restatement.py, for the reason given there."""
import math

import numpy as np
import pytest
import torch

import fusion_scene as S
import fusion_weighted_restatement as FW
import ghost_scene as G
import noisy_scene as N
from test_gpu_rigid3d import _depth
from test_rigid3d_host import K_SYN

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-12
TWIST = np.array([0.013, -0.021, 0.008, 0.05, -0.17, 0.11])
# the volumes and fractional offsets of tests/test_gpu_fusion.py, and a 45-voxel one whose last voxel is the tail
VOLUMES = [((40, 40, 40), np.array([-20.5, -20.25, 230.75])), ((33, 17, 70), np.array([-35.0, -8.5, 232.0])),
           ((5, 3, 3), np.array([-1.5, -1.25, 247.5]))]
_DEPTH = {}


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K_, ratio=0.001):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _frame(dtype):
    """the rigid tests' depth image (holes and inf in the float ones) on the host and the device, made once"""
    from levelsetfusion_python_amd.tsdf import generation as gen
    if dtype not in _DEPTH:
        d = _depth(dtype)
        _DEPTH[dtype] = (d,) + tuple(gen.device_depth(d))
    return _DEPTH[dtype]


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _random_model(shape, rng, cap=8.0):
    """tsdf in [-1, 1] with a few exact +1, weights 0, mid and at the cap"""
    t = rng.uniform(-1, 1, shape).astype(np.float32)
    t.reshape(-1)[::13] = 1.0
    w = rng.choice(np.array([0, 0, 1, 2.5, 5, cap], np.float32), shape)
    return t, w


def _random_weights(shape, rng):
    """a weight image with exact 0, negative values, NaN, +inf, tiny normal values and the smallest normal float32"""
    pw = rng.uniform(0.05, 2.0, shape).astype(np.float32)
    flat = pw.reshape(-1)
    flat[::5] = 0.0
    flat[1::11] = -0.5
    flat[2::13] = np.nan
    flat[3::17] = np.inf
    flat[4::19] = 1e-30
    flat[6::23] = np.finfo(np.float32).tiny
    return pw


def _device(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _unpack(r):
    from levelsetfusion_python_amd.device_fusion import unpack_weighted_record
    return unpack_weighted_record(r.cpu().numpy())


def _assert_record(got, want):
    for key in ("fused", "first_seen", "carved", "weight_rejected", "max_abs_change"):
        assert got[key] == want[key], (key, got, want)
    np.testing.assert_allclose(got["sum_abs_change"], want["sum_abs_change"], rtol=SUM_RTOL, atol=0)


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_identity_with_the_unweighted_entry_point(lsf, depth_dtype):
    from levelsetfusion_python_amd import device_fusion
    _, dev, code = _frame(depth_dtype)
    cam = _camera(K_SYN)
    ones = torch.ones(tuple(dev.shape), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(7)
    for shape, off in VOLUMES:
        t, W = _random_model(shape, rng)
        for w, cap in ((1.0, math.inf), (0.5, 6.0)):
            a_t, a_w = _device(t, W)
            want = device_fusion.integrate_depth(a_t, a_w, dev, code, cam, off, TWIST, w=w, max_weight=cap)
            want = want.cpu().numpy()
            for pw in (None, ones):
                b_t, b_w = _device(t, W)
                got = device_fusion.integrate_depth_weighted(b_t, b_w, dev, code, cam, off, TWIST, w=w, max_weight=cap,
                                                             pixel_weight=pw, carve=False).cpu().numpy()
                assert _bits_equal(a_t.cpu().numpy(), b_t.cpu().numpy())
                assert _bits_equal(a_w.cpu().numpy(), b_w.cpu().numpy())
                assert np.array_equal(got[:4].view(np.uint64), want[:4].view(np.uint64)) and not got[4:].any()
            assert want[0] > (1000 if len(t.reshape(-1)) > 1000 else 0)


@pytest.mark.parametrize("carve,cap,w", [(False, math.inf, 1.0), (True, 6.0, 0.5), (True, math.inf, 1.0),
                                         (False, 6.0, 0.5)])
@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32])
def test_against_restatement(lsf, depth_dtype, carve, cap, w):
    from levelsetfusion_python_amd import device_fusion
    d, dev, code = _frame(depth_dtype)
    cam = _camera(K_SYN)
    rng = np.random.default_rng(11)
    pw = _random_weights(d.shape, rng)
    pw_dev, = _device(pw)
    for shape, off in VOLUMES:
        t, W = _random_model(shape, rng)
        a_t, a_w = _device(t, W)
        rec = device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, cam, off, TWIST, w=w, max_weight=cap,
                                                     pixel_weight=pw_dev, carve=carve)
        assert rec.dtype == torch.float64 and rec.is_cuda and rec.shape == (8,)
        want_t, want_w, want = FW.fuse_depth_weighted(t, W, d, K_SYN, 0.001, off, TWIST, 20, 0.004, w, cap, pw, carve)
        assert _bits_equal(a_t.cpu().numpy(), want_t) and _bits_equal(a_w.cpu().numpy(), want_w)
        got = _unpack(rec)
        _assert_record(got, want)
        assert not rec.cpu().numpy()[6:].any()
        if len(t.reshape(-1)) > 1000:
            assert got["fused"] > 1000 and got["weight_rejected"] > 100 and (got["carved"] > 1000) == carve


def test_unaligned_views_give_the_aligned_bits(lsf):
    """tsdf and weight off 16-byte alignment take scalar accesses over the same voxel order"""
    from levelsetfusion_python_amd import device_fusion
    _, dev, code = _frame(np.uint16)
    cam = _camera(K_SYN)
    shape, off = VOLUMES[1]
    n = int(np.prod(shape))
    rng = np.random.default_rng(5)
    t, W = _random_model(shape, rng)
    pw_dev, = _device(_random_weights(tuple(dev.shape), rng))
    big = torch.empty(2 * n + 8, dtype=torch.float32, device="cuda")
    tv, wv = big[1:n + 1].view(shape), big[n + 3:2 * n + 3].view(shape)
    assert tv.data_ptr() % 16 and wv.data_ptr() % 16
    tv.copy_(torch.from_numpy(t)), wv.copy_(torch.from_numpy(W))
    a_t, a_w = _device(t, W)
    kw = dict(w=0.5, max_weight=6.0, pixel_weight=pw_dev, carve=True)
    rec_v = device_fusion.integrate_depth_weighted(tv, wv, dev, code, cam, off, TWIST, **kw)
    rec_a = device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, cam, off, TWIST, **kw)
    assert _bits_equal(tv.cpu().numpy(), a_t.cpu().numpy()) and _bits_equal(wv.cpu().numpy(), a_w.cpu().numpy())
    assert np.array_equal(rec_v.cpu().numpy().view(np.uint64), rec_a.cpu().numpy().view(np.uint64))
    assert rec_a.cpu().numpy()[4] > 0


def test_record_bit_identical_across_runs(lsf):
    from levelsetfusion_python_amd import device_fusion
    _, dev, code = _frame(np.float32)
    cam = _camera(K_SYN)
    shape, off = VOLUMES[0]
    rng = np.random.default_rng(9)
    t, W = _random_model(shape, rng)
    pw_dev, = _device(_random_weights(tuple(dev.shape), rng))
    recs = []
    for _ in range(2):
        a_t, a_w = _device(t, W)
        recs.append(device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, cam, off, TWIST, max_weight=5.0,
                                                           pixel_weight=pw_dev, carve=True).cpu().numpy())
    assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64)) and recs[0][2] > 0


def _holed_noisy_frame():
    """a noisy frame cut to extents that are no multiple of the confidence kernel's 64 x 4 tile, with holes"""
    d = N.render(S.true_twist(2), seed=2)[150:300, 200:403].copy()
    d[20:30, 50:70] = 0
    return d


def test_depth_confidence_against_restatement(lsf):
    """fed the device pyramid's own level 0, so the filter's tolerance stays out of the comparison"""
    from levelsetfusion_python_amd import device_depth_confidence
    d = _holed_noisy_frame()
    assert d.shape == (150, 203) and d.shape[0] % 4 and d.shape[1] % 64
    cam = _camera(S.K, N.RATIO)
    for radius in (3, 0):
        pyr = lsf.rigid_opt.DepthPyramid(levels=1, radius=radius)
        out = pyr.build(d, cam)
        depth_m, normals = out.depth[0], out.normals[0]
        got = device_depth_confidence.depth_confidence(depth_m, normals, cam, 0.55)
        assert got.dtype == torch.float32 and tuple(got.shape) == d.shape
        hd, hn = depth_m.cpu().numpy(), normals.cpu().numpy()
        want = FW.confidence(hd, hn, S.K, 0.55)
        got = got.cpu().numpy()
        assert _bits_equal(got, want)
        holes, no_normal = hd == 0, ~hn.any(axis=-1) & (hd > 0)
        assert holes.sum() >= 200 and no_normal.sum() > 100
        assert not got[holes].any() and not got[no_normal].any()
        # a cosine of two unit vectors (the normal rounded to float32) times a factor <= 1; both sides of z_ref occur
        assert got.min() >= 0 and got.max() <= 1.0 + 2.0 ** -22
        assert (hd[got > 0] > 0.55).any() and (hd[got > 0] < 0.55).any()
        conf = lsf.fusion.DepthConfidence(0.55, lsf.rigid_opt.DepthPyramid(radius=radius))
        assert _bits_equal(conf.build(d, cam).cpu().numpy(), want)
        assert _bits_equal(conf.from_levels(out, cam).cpu().numpy(), want)


def test_ghost_scenario_on_the_device(lsf):
    """frame A with the ghost, then frame B without it: carving equals the restatement bit for bit and takes the ghost
    out of the extracted mesh; without carving it stays"""
    cam = _camera(G.K, 1.0)
    off = S.offset(G.N)
    zero = np.zeros(6)
    a, b = G.with_ghost(), G.plain()
    empty = np.ones((G.N,) * 3, np.float32), np.zeros((G.N,) * 3, np.float32)
    t, w, _ = FW.fuse_depth_weighted(*empty, a, G.K, 1.0, off, zero)
    near = {}
    for carve in (True, False):
        vol = lsf.fusion.CanonicalVolume(G.N)
        vol.integrate_depth(a, cam, zero, off)
        rec = vol.integrate_depth(b, cam, zero, off, carve=carve)
        if carve:
            want_t, want_w, want = FW.fuse_depth_weighted(t, w, b, G.K, 1.0, off, zero, carve=True)
            assert _bits_equal(vol.tsdf.cpu().numpy(), want_t) and _bits_equal(vol.weight.cpu().numpy(), want_w)
            _assert_record(_unpack(rec), want)
            assert want["carved"] > 0
        verts, faces = vol.extract_mesh(off)
        assert len(faces) > 1000
        near[carve] = np.count_nonzero(np.linalg.norm(verts - G.GHOST_CENTRE, axis=1) < G.GHOST_RADIUS + 2 * 0.004)
    assert near[True] == 0 and near[False] > 0


def test_sequence_with_carving_and_confidence_equals_a_manual_composition(lsf):
    """64^3, four noisy frames, "icp" tracking over a pyramid that the confidence shares: the model equals, bit for bit,
    the same device calls made by hand, and the records carry carved and weight_rejected.
    The twists are not compared with those of a run without the two options: frame 0's model is not the same band with
    other weights.  A pixel without a normal has confidence 0 (test_depth_confidence_against_restatement asserts it), so
    the voxels behind the last row and column and behind every depth step at a silhouette stay unobserved, where the
    unweighted rule fuses them; the prediction that frame 1 is tracked against is ray-cast from a different model."""
    from levelsetfusion_python_amd import device_fusion, device_raycast
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    n, count = 64, 4
    off = S.offset(n)
    cam = _camera(S.K, N.RATIO)
    frames = N.frames(count)
    pyr = lsf.rigid_opt.DepthPyramid()
    conf = lsf.fusion.DepthConfidence()
    seq = lsf.SequenceFusion3d(cam, n, off, tracking_reference="icp", icp_pyramid=pyr, carve=True, confidence=conf)
    vol = lsf.fusion.CanonicalVolume(n)
    icp = lsf.ProjectiveIcp3d(cam, pyramid=pyr)
    twist = np.zeros(6)
    for k, frame in enumerate(frames):
        rec = seq.integrate(frame)
        depth, code = device_depth(frame)
        if k == 0:
            pw = conf.build_device(depth, code, cam)
        else:
            pd, pn, _ = device_raycast.raycast(vol.tsdf, vol.weight, cam, twist, off, 0.004, tuple(depth.shape),
                                               normals=True)
            twist, _, _ = icp.track(depth, code, pd, pn, twist, twist)
            pw = conf.from_levels(icp.last_pyramid, cam)
        want = device_fusion.integrate_depth_weighted(vol.tsdf, vol.weight, depth, code, cam, off, twist,
                                                      pixel_weight=pw, carve=True)
        assert np.array_equal(seq.twists[-1], np.asarray(twist, np.float64).reshape(6))
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), vol.tsdf.cpu().numpy())
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), vol.weight.cpu().numpy())
        assert rec["fusion"] == _unpack(want)
        assert rec["fusion"]["carved"] > 10000 and rec["fusion"]["weight_rejected"] > 0
        assert len(rec["rigid_records"]) == (14 if k else 0)
    assert len(seq.frame_records) == count


def test_sequence_defaults_run_the_unweighted_path(lsf):
    n = 32
    off = S.offset(n)
    cam = _camera(S.K, 1.0)
    seq = lsf.SequenceFusion3d(cam, n, off, rigid_iterations=0)
    vol = lsf.fusion.CanonicalVolume(n)
    assert seq.carve is False and seq.confidence is None
    for frame in S.frames(2):
        rec = seq.integrate(frame)
        want = vol.integrate_depth(frame, cam, np.zeros(6), off)
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), vol.tsdf.cpu().numpy())
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), vol.weight.cpu().numpy())
        assert tuple(rec["fusion"]) == lsf.fusion.RECORD_FIELDS
        assert not want.cpu().numpy()[4:].any()


def test_host_refuses_a_bad_weight_image(lsf):
    from levelsetfusion_python_amd import device_fusion
    _, dev, code = _frame(np.uint16)
    cam = _camera(K_SYN)
    t, w = torch.ones((8, 8, 8), device="cuda"), torch.zeros((8, 8, 8), device="cuda")
    good = torch.ones(tuple(dev.shape), device="cuda")
    args = (dev, code, cam, [0, 0, 0], np.zeros(6))
    with pytest.raises(ValueError, match="one shape"):
        device_fusion.integrate_depth_weighted(t, w, *args, pixel_weight=good[:-1])
    with pytest.raises(ValueError, match="float32"):
        device_fusion.integrate_depth_weighted(t, w, *args, pixel_weight=good.double())
    with pytest.raises(ValueError, match="contiguous"):
        device_fusion.integrate_depth_weighted(t, w, *args, pixel_weight=good.t().contiguous().t())
    with pytest.raises(ValueError, match="one device"):
        device_fusion.integrate_depth_weighted(t, w, *args, pixel_weight=good.cpu())
    with pytest.raises(TypeError, match="torch tensor"):
        device_fusion.integrate_depth_weighted(t, w, *args, pixel_weight=np.ones(tuple(dev.shape), np.float32))
    big = torch.ones(480 * 640 + 512, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        device_fusion.integrate_depth_weighted(big[:512].view(8, 8, 8), w, *args,
                                               pixel_weight=big[256:256 + 480 * 640].view(480, 640))
    fdev = dev.to(torch.float32)
    with pytest.raises(ValueError, match="alias"):
        device_fusion.integrate_depth_weighted(t, w, fdev, 1, cam, [0, 0, 0], np.zeros(6), pixel_weight=fdev)
    with pytest.raises(ValueError, match="float32"):
        lsf.fusion.CanonicalVolume(8).integrate_depth(_frame(np.uint16)[0], cam, np.zeros(6), [0, 0, 0],
                                                      pixel_weight=np.ones(tuple(dev.shape)))
    assert torch.all(t == 1) and torch.all(w == 0)  # nothing was launched
