"""GPU checks of the 6-DoF SDF-2-SDF rigid 3-D tracker (csrc/lsf_rigid3d.hip) against the numpy restatement
(tests/rigid3d_restatement.py) and, through y-constant volumes, the reference's 2-D answers (tests/golden/ref_rigid.npz)."""
import os

import numpy as np
import pytest
import torch

import rigid3d_restatement as R3
from conftest import GOLDEN, load_golden
from test_rigid3d_host import K_SYN, XI0, assert_recovered, recovery_case

pytestmark = pytest.mark.gpu

FRAMES = [os.path.join(GOLDEN, n) for n in ("depth_000000.exr", "depth_000003.exr")]
K = np.array([[570.3999633789062, 0, 320], [0, 570.3999633789062, 240], [0, 0, 1]], dtype=np.float32)
# per-iteration A, b and energy of the device's tree reduction against the restatement's pairwise np.sum, and the twist
A_RTOL, TWIST_ATOL = 1e-12, 1e-9
TWISTS = [np.zeros(6), np.array([0.013, -0.021, 0.008, 0.05, -0.17, 0.11]), np.array([-0.2, 0.1, 0.3, -0.6, 0.4, 0.9]),
          np.array([0, 0, 0, 0, 0.5, 0])]


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


def _depth(dtype):
    from levelsetfusion_python_amd import synthetic
    d = synthetic.depth_image()
    if dtype == np.uint16:
        return d
    d = d.astype(dtype) * dtype(1.0001)
    d[::7, ::5] = np.inf
    d[::11, ::3] = 0
    return d


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_live_volume_of_the_run_equals_the_typed_generator(lsf, depth_dtype):
    from levelsetfusion_python_amd import device_rigid
    from levelsetfusion_python_amd.tsdf import generation as gen
    d = _depth(depth_dtype)
    cam = _camera(K_SYN)
    off = np.array([-20.5, -20.25, 230.75])
    dev, code = gen.device_depth(d)
    for twist in TWISTS[:3]:
        live, grad = device_rigid.live_and_gradient_3d(dev, code, cam, 40, off, twist)
        want = gen.generate_tsdf_field_from_depth_image_typed(
            d, cam, None, lsf.transformation.twist_vector_to_matrix3d(twist.astype(np.float32)), field_size=40,
            array_offset=off, dims=3)
        assert _bits_equal(live.cpu().numpy(), want)
        assert _bits_equal(live.cpu().numpy(), R3.live_volume(d, K_SYN, 0.001, (40, 40, 40), off, twist))
        assert _bits_equal(grad.cpu().numpy(), R3.gradient_wrt_twist_3d(want, twist, off))


@pytest.mark.parametrize("shape", [(5, 5, 5), (33, 17, 70), (128, 128, 128), (2, 3, 2)])
def test_gradient_wrt_twist_3d_against_restatement(lsf, shape):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d
    rng = np.random.default_rng(11)
    live = np.clip(rng.normal(0, 0.7, shape), -1, 1).astype(np.float32)
    off = np.array([-30.5, -9, 41.25])
    for twist in TWISTS:
        g = calculate_gradient_wrt_twist_3d(live, twist.reshape(6, 1), off, 0.004)
        assert g.dtype == np.float32 and g.shape == shape + (6,)
        assert _bits_equal(g, R3.gradient_wrt_twist_3d(live, twist, off, 0.004))
    t = calculate_gradient_wrt_twist_3d(torch.from_numpy(live).cuda(), TWISTS[1], off, 0.002, as_tensor=True)
    assert t.is_cuda and _bits_equal(t.cpu().numpy(), R3.gradient_wrt_twist_3d(live, TWISTS[1], off, 0.002))


@pytest.mark.parametrize("k", range(6))
def test_reference_2d_answers_on_the_device(lsf, k):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d
    ref = load_golden("ref_rigid.npz")
    p = "grad.%d." % k
    t = ref[p + "twist"].reshape(3)
    vol = np.repeat(ref[p + "live"].astype(np.float32)[:, None, :], 3, axis=1)
    g = calculate_gradient_wrt_twist_3d(vol, [t[0], 0, t[1], 0, t[2], 0], ref[p + "offset"], float(ref[p + "voxel_size"]))
    assert _bits_equal(g, R3.gradient_wrt_twist_3d(vol, [t[0], 0, t[1], 0, t[2], 0], ref[p + "offset"],
                                                   float(ref[p + "voxel_size"])))
    for y in range(3):
        same = np.array_equal(g[:, y][..., [0, 2, 4]], ref[p + "out"])
        assert same == (k != 5)  # grad.5 (theta = 0.5) is the documented r_y divergence
    assert not np.any(g[..., 1])


def _run(canonical, depth, cam, off, iterations, twist=None, band=20., eta=0.01, voxel_size=0.004):
    from levelsetfusion_python_amd import device_rigid
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    dev, code = device_depth(depth)
    return device_rigid.rigid_run_3d(canonical, dev, code, cam, off, iterations, 0.5, eta, voxel_size, 0.004, band,
                                     twist=twist)


def _teacher_forced(records, canonical, depth, K_, off, band=20., eta=0.01, voxel_size=0.004, start=None):
    """every device record k against the restatement's iteration at the device's own twist before it"""
    twist = np.zeros(6) if start is None else np.asarray(start, np.float64)
    for r in records:
        want, _ = R3.step(canonical, depth, K_, 0.001, off, twist, band, eta, voxel_size)
        got_a, got_b, got_e = r[13:49].reshape(6, 6), r[49:55], r[12]
        assert int(r[55]) == want["skipped"]
        np.testing.assert_allclose(got_a, want["A"], rtol=A_RTOL, atol=0)
        np.testing.assert_allclose(got_b, want["b"], rtol=A_RTOL, atol=1e-300)
        np.testing.assert_allclose(got_e, want["energy"], rtol=A_RTOL)
        twist = r[6:12]


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
def test_run_against_restatement_64(lsf, depth_dtype):
    canonical, _, off = recovery_case(64)
    depth = _depth(depth_dtype)
    twist, records = _run(canonical, depth, _camera(K_SYN), off, 10)
    assert records.shape == (10, 64) and not np.any(records[:, 56:])
    _teacher_forced(records, canonical, depth, K_SYN, off)
    _, want = R3.optimize(canonical, depth, K_SYN, 0.001, off, 10, 20.)
    np.testing.assert_allclose(twist, want, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1, 6:12])


def test_ragged_volume_and_starting_twist(lsf):
    """a (Z, Y, X) that is not a cube nor a tile multiple, started off zero"""
    depth = _depth(np.uint16)
    off = np.array([-35.0, -8.5, 232.0])
    shape = (33, 17, 70)
    canonical = R3.live_volume(depth, K_SYN, 0.001, shape, off, XI0)
    start = np.array([0.001, 0.0, -0.001, 0.0, 0.01, 0.0])
    twist, records = _run(canonical, depth, _camera(K_SYN), off, 4, twist=start)
    _teacher_forced(records, canonical, depth, K_SYN, off, start=start)
    _, want = R3.optimize(canonical, depth, K_SYN, 0.001, off, 4, 20., twist=start)
    np.testing.assert_allclose(twist, want, rtol=0, atol=TWIST_ATOL)


def test_recovers_a_known_twist(lsf):
    from levelsetfusion_python_amd.tsdf import generation as gen
    _, depth, off = recovery_case(64)
    cam = _camera(K_SYN)
    canonical = gen.generate_tsdf_field_from_depth_image_typed(
        depth, cam, None, lsf.transformation.twist_vector_to_matrix3d(XI0), field_size=64, array_offset=off, dims=3,
        as_tensor=True)
    twist, records = _run(canonical, depth, cam, off, 60)
    assert not np.any(records[:, 55])
    assert_recovered(twist, records[:, 12])


def test_fronto_parallel_wall_is_skipped(lsf, capsys):
    """two constant depth images: g_tx, g_ty and g_rz are 0 at every voxel, A has three zero rows and columns"""
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    wall = np.full((480, 640), 600, dtype=np.uint16)
    off = np.array([-16, -16, 110])
    data = ArrayBasedSingleFrameDataset(wall, wall.copy(), 240, 32, off, _camera(K))
    opt = lsf.Sdf2SdfOptimizer3d()
    twist = opt.optimize(data, iteration=3)
    assert twist.shape == (6, 1) and twist.dtype == np.float64 and not np.any(twist)
    assert [r["skipped"] for r in opt.last_records] == [1, 1, 1]
    canonical = R3.tsdf_nearest(wall, K, 0.001, (32, 32, 32), off)
    want, _ = R3.step(canonical, wall, K, 0.001, off, np.zeros(6), 20.)
    assert want["skipped"] == 1
    for r in opt.last_records:
        a = r["matrix_a"]
        assert not np.any(a[[0, 1, 5]]) and not np.any(a[:, [0, 1, 5]]) and np.any(a)
        np.testing.assert_allclose(a, want["A"], rtol=A_RTOL, atol=0)
        assert not np.any(r["twist_star"]) and not np.any(r["twist"])
    assert capsys.readouterr().out.count("SINGULAR MATRIX!") == 3


def test_two_runs_bit_equal(lsf):
    canonical, depth, off = recovery_case(96)
    a = _run(canonical, depth, _camera(K_SYN), off, 5)
    b = _run(canonical, depth, _camera(K_SYN), off, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_exr_frames_through_the_optimizer(lsf, capsys):
    from levelsetfusion_python_amd import image_io
    from levelsetfusion_python_amd.rigid_opt import sdf_2_sdf_optimizer3d as s3
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ImageBasedSingleFrameDataset
    off = np.array([-32, -32, 60])  # the surface, at about 0.47 m, crosses the volume's far half
    data = ImageBasedSingleFrameDataset(FRAMES[0], FRAMES[1], 240, 64, off, _camera(K))
    opt = s3.Sdf2SdfOptimizer3d(verbosity_parameters=s3.Sdf2SdfOptimizer3d.VerbosityParameters(True, True))
    twist = opt.optimize(data, iteration=10)
    assert twist.shape == (6, 1) and np.all(np.isfinite(twist))
    energies = [r["energy"] for r in opt.last_records]
    assert energies[-1] < energies[0]
    d0, d1 = image_io.read_depth_image(FRAMES[0]), image_io.read_depth_image(FRAMES[1])
    canonical = R3.tsdf_nearest(d0, K, 0.001, (64, 64, 64), off)
    records = np.array([np.concatenate([r["twist_star"].ravel(), r["twist"].ravel(), [r["energy"]],
                                        r["matrix_a"].ravel(), r["vector_b"].ravel(), [r["skipped"]], np.zeros(8)])
                        for r in opt.last_records])
    _teacher_forced(records, canonical, d1, K, off)
    _, want = R3.optimize(canonical, d1, K, 0.001, off, 10, 20.)
    np.testing.assert_allclose(twist.reshape(6), want, rtol=0, atol=TWIST_ATOL)
    lines = capsys.readouterr().out.splitlines()
    r = opt.last_records[0]
    assert lines[0] == "%s[ITERATION 0 COMPLETED]%s energy: %f" % (s3.BOLD_LIGHT_CYAN, s3.RESET, r["energy"])
    assert lines[1] == "optimal twist: %s, twist: %s" % (", ".join("%f" % v for v in r["twist_star"].ravel()),
                                                         ", ".join("%f" % v for v in r["twist"].ravel()))


def test_dataset_volumes(lsf):
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    from levelsetfusion_python_amd.tsdf.generation import FilteringMethod
    d0, d1 = _depth(np.uint16), _depth(np.float32)
    off = np.array([-12, -12, 238.5])
    data = ArrayBasedSingleFrameDataset(d0, d1, 240, 24, off, _camera(K_SYN))
    live, canonical = data.generate_3d_sdf_fields()
    assert _bits_equal(canonical, R3.tsdf_nearest(d0, K_SYN, 0.001, (24, 24, 24), off))
    assert _bits_equal(live, R3.live_volume(d1, K_SYN, 0.001, (24, 24, 24), off, np.zeros(6)))
    t = np.array([0.001, 0.002, -0.003, 0.01, 0.02, -0.03], dtype=np.float32)
    moved = data.generate_3d_live_field(twist=t)
    assert _bits_equal(moved, R3.live_volume(d1, K_SYN, 0.001, (24, 24, 24), off, t))
    with pytest.raises(ValueError, match="nearest pixel"):
        data.generate_3d_canonical_field(method=FilteringMethod.BILINEAR_IMAGE_SPACE)


def test_host_argument_checks_on_device(lsf):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d
    with pytest.raises(ValueError, match="3-D volume"):
        calculate_gradient_wrt_twist_3d(np.zeros((4, 4), np.float32), np.zeros(6), [0, 0, 0])
    with pytest.raises(ValueError, match="3-D volume"):
        calculate_gradient_wrt_twist_3d(np.zeros((4, 1, 4), np.float32), np.zeros(6), [0, 0, 0])
    with pytest.raises(ValueError, match="6 entries"):
        calculate_gradient_wrt_twist_3d(np.zeros((4, 4, 4), np.float32), np.zeros(3), [0, 0, 0])
    with pytest.raises(ValueError, match="positive"):
        calculate_gradient_wrt_twist_3d(np.zeros((4, 4, 4), np.float32), np.zeros(6), [0, 0, 0], voxel_size=-1)
    with pytest.raises(ValueError, match="iteration"):
        _run(np.zeros((4, 4, 4), np.float32), np.zeros((8, 8), np.uint16), _camera(K), [0, 0, 0], -1)
    twist, records = _run(np.zeros((4, 4, 4), np.float32), np.zeros((8, 8), np.uint16), _camera(K), [0, 0, 0], 0,
                          twist=np.arange(6.0))
    assert np.array_equal(twist, np.arange(6.0)) and records.shape == (0, 64)
