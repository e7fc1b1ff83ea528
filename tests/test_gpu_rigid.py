"""GPU checks of the SDF-2-SDF rigid tracker and the typed TSDF input stage (csrc/lsf_rigid.hip, csrc/lsf_tsdf_typed.h)
against the reference's answers (tests/golden/ref_rigid.npz) and the numpy restatement (tests/rigid_restatement.py)."""
import os

import numpy as np
import pytest
import torch

import rigid_restatement as R
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

FRAMES = [os.path.join(GOLDEN, n) for n in ("depth_000000.exr", "depth_000003.exr")]
K = np.array([[570.3999633789062, 0, 320], [0, 570.3999633789062, 240], [0, 0, 1]], dtype=np.float32)
# measured: per-iteration A, b and energy of the device's tree reduction against the reference's sequential loop, and
# its twist (tests/test_gpu_rigid.py, MI355X)
A_RTOL, TWIST_ATOL = 1e-12, 1e-9


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_rigid.npz")


def _camera(lsf, K_, ratio=0.001):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


@pytest.mark.parametrize("k", range(1, 12))
def test_sdf_generation_answers(lsf, ref, k):
    from levelsetfusion_python_amd.tsdf import generation as gen
    p = "gen.%02d." % k
    E = ref[p + "E"]
    field = gen.generate_2d_tsdf_field_from_depth_image(
        ref[p + "depth"], _camera(lsf, ref[p + "K"], float(ref[p + "ratio"])), int(ref[p + "row"]),
        camera_extrinsic_matrix=E, field_size=int(ref[p + "field_size"]), default_value=float(ref[p + "default"]),
        voxel_size=float(ref[p + "voxel"]), array_offset=ref[p + "offset"],
        narrow_band_width_voxels=float(ref[p + "band"]))
    assert np.allclose(ref[p + "expected"], field)
    if ref[p + "depth"].dtype != np.uint16:  # the typed path: the reference's own bits
        assert np.array_equal(field, ref[p + "out"])


def test_old_and_new_paths_equal_on_uint16(lsf):
    from levelsetfusion_python_amd.tsdf import generation as gen
    from levelsetfusion_python_amd import image_io
    d = image_io.read_depth_image(FRAMES[0])
    E = np.eye(4, dtype=np.float32)
    E[0, 3], E[2, 3] = 0.01, -0.02
    for K_ in (K, K.astype(np.float64)):
        cam = _camera(lsf, K_)
        for off in ((-64, -64, 50), np.array([[-16], [-16], [93]], dtype=np.int32)):
            old = gen.generate_2d_tsdf_field_from_depth_image(d, cam, 240, E, field_size=128, array_offset=off)
            new = gen.generate_tsdf_field_from_depth_image_typed(d, cam, 240, E, field_size=128, array_offset=off)
            assert old.view(np.uint32).tolist() == new.view(np.uint32).tolist()
        old3 = gen.generate_3d_tsdf_field_from_depth_image(d, cam, E, field_size=32, array_offset=(-16, -16, 100))
        new3 = gen.generate_tsdf_field_from_depth_image_typed(d, cam, None, E, field_size=32,
                                                              array_offset=(-16, -16, 100), dims=3)
        assert np.array_equal(old3.view(np.uint32), new3.view(np.uint32))


@pytest.mark.parametrize("depth_dtype", [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("e_dtype", [np.float32, np.float64])
def test_float_depth_and_fractional_offsets_against_restatement(lsf, depth_dtype, e_dtype):
    from levelsetfusion_python_amd.tsdf import generation as gen
    from levelsetfusion_python_amd import image_io
    d = image_io.read_depth_image(FRAMES[1]).astype(depth_dtype)
    if depth_dtype != np.uint16:
        d = d * depth_dtype(1.0001)
        d[::7, ::5] = np.inf
        d[::11, ::3] = 0
    E = lsf.transformation.twist_vector_to_matrix3d(np.array([0.01, 0, -0.02, 0, 0.1, 0])).astype(e_dtype)
    off = np.array([-40.5, -40.25, 60.75])
    cam = _camera(lsf, K)
    for n, row in ((80, 240), (37, 100)):
        got = gen.generate_2d_tsdf_field_from_depth_image(d, cam, row, E, field_size=n, array_offset=off,
                                                          narrow_band_width_voxels=6)
        want = R.tsdf_nearest(d, K, 0.001, (n, n), off, E, 6, 0.004, row)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if depth_dtype == np.uint16:
        got3 = gen.generate_3d_tsdf_field_from_depth_image(d, cam, E, field_size=24, array_offset=off)
    else:  # the volume generator keeps refusing float depth (tests/test_gpu_tsdf.py)
        with pytest.raises(ValueError, match="float depth"):
            gen.generate_3d_tsdf_field_from_depth_image(d, cam, E, field_size=24, array_offset=off)
        got3 = gen.generate_tsdf_field_from_depth_image_typed(d, cam, None, E, field_size=24, array_offset=off, dims=3)
    want3 = R.tsdf_nearest(d, K, 0.001, (24, 24, 24), off, E, 20, 0.004)
    assert np.array_equal(got3.view(np.uint32), want3.view(np.uint32))


@pytest.mark.parametrize("k", range(6))
def test_gradient_wrt_twist_reference_answers(lsf, ref, k):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist
    p = "grad.%d." % k
    g = calculate_gradient_wrt_twist(ref[p + "live"], ref[p + "twist"], ref[p + "offset"], float(ref[p + "voxel_size"]))
    assert g.dtype == np.float32 and g.shape == ref[p + "out"].shape
    assert np.array_equal(g, ref[p + "out"])


@pytest.mark.parametrize("shape", [(512, 512), (45, 77), (2, 2)])
def test_gradient_wrt_twist_against_restatement(lsf, shape):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist
    rng = np.random.default_rng(7)
    live = np.clip(rng.normal(0, 0.7, shape), -1, 1).astype(np.float32)
    twist = np.array([[0.013], [-0.021], [0.17]])
    off = np.array([-30.5, -9, 41.25])
    g = calculate_gradient_wrt_twist(live, twist, off, 0.004)
    assert np.array_equal(g.view(np.uint32), R.gradient_wrt_twist(live, twist, off, 0.004).view(np.uint32))


def _dataset(lsf, n, off, frames=FRAMES):
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ImageBasedSingleFrameDataset
    return ImageBasedSingleFrameDataset(frames[0], frames[1], 240, n, off, _camera(lsf, K))


def test_sdf_2_sdf_optimizer01_end_to_end(lsf, ref):
    opt = lsf.Sdf2SdfOptimizer2d()
    twist = opt.optimize(_dataset(lsf, 32, np.array([[-16], [-16], [93.4375]])), narrow_band_width_voxels=2.,
                         iteration=10)
    assert twist.shape == (3, 1) and twist.dtype == np.float64
    assert np.allclose(ref["opt.test01.expected_twist"], twist, atol=1e-6)


@pytest.mark.parametrize("tag", ["test01", "same_cpp", "large"])
def test_per_iteration_records_against_reference(lsf, ref, tag):
    p = "opt.%s." % tag
    n, off = int(ref[p + "field_size"]), ref[p + "offset"]
    if tag == "same_cpp":
        off = off.astype(np.int32).reshape(3, 1)
    opt = lsf.Sdf2SdfOptimizer2d()
    twist = opt.optimize(_dataset(lsf, n, off), narrow_band_width_voxels=float(ref[p + "band"]),
                         iteration=int(ref[p + "iterations"]), eta=float(ref[p + "eta"]))
    assert len(opt.last_records) == int(ref[p + "iterations"])
    for i, rec in enumerate(opt.last_records):
        assert rec["skipped"] == ref[p + "skipped"][i]
        np.testing.assert_allclose(rec["matrix_a"], ref[p + "A"][i], rtol=A_RTOL, atol=0)
        np.testing.assert_allclose(rec["vector_b"].reshape(3), ref[p + "b"][i], rtol=A_RTOL)
        np.testing.assert_allclose(rec["energy"], ref[p + "energy"][i], rtol=A_RTOL)
        np.testing.assert_allclose(rec["twist"].reshape(3), ref[p + "twist"][i], rtol=0, atol=TWIST_ATOL)
    np.testing.assert_allclose(twist, ref[p + "final_twist"], rtol=0, atol=TWIST_ATOL)


def test_singular_pair_skips_every_update(lsf, ref, capsys):
    from levelsetfusion_python_amd import image_io
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    d0 = image_io.read_depth_image(FRAMES[0])
    data = ArrayBasedSingleFrameDataset(d0, np.full((480, 640), np.inf), 240, 16, np.array([-8, -8, 100]),
                                        _camera(lsf, K))
    opt = lsf.Sdf2SdfOptimizer2d()
    twist = opt.optimize(data, iteration=3)
    assert np.array_equal(twist, np.zeros((3, 1)))
    assert [r["skipped"] for r in opt.last_records] == list(ref["opt.singular.skipped"]) == [1, 1, 1]
    assert all(not np.any(r["matrix_a"]) for r in opt.last_records)
    np.testing.assert_allclose([r["energy"] for r in opt.last_records], ref["opt.singular.energy"], rtol=A_RTOL)
    assert capsys.readouterr().out.count("SINGULAR MATRIX!") == 3


def test_flat_wall_skips_like_the_reference(lsf, ref, capsys):
    """two constant depth images: the twist gradient's x component is 0 at every voxel, so A has a zero row and column
    -- not zero, yet cond(A) is inf: the reference prints SINGULAR MATRIX! and returns the zero twist, and so must we"""
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    wall = np.full((480, 640), 600, dtype=np.uint16)
    data = ArrayBasedSingleFrameDataset(wall, wall.copy(), 240, 32, np.array([-16, -16, 110]), _camera(lsf, K))
    opt = lsf.Sdf2SdfOptimizer2d()
    twist = opt.optimize(data, iteration=3)
    assert np.array_equal(twist, ref["opt.flat.final_twist"]) and not np.any(twist)
    assert [r["skipped"] for r in opt.last_records] == list(ref["opt.flat.skipped"]) == [1, 1, 1]
    for i, r in enumerate(opt.last_records):
        a = r["matrix_a"]
        assert not np.any(a[0]) and not np.any(a[:, 0]) and np.any(a)
        np.testing.assert_allclose(a, ref["opt.flat.A"][i], rtol=A_RTOL, atol=0)
        np.testing.assert_allclose(r["energy"], ref["opt.flat.energy"][i], rtol=A_RTOL)
        assert not np.isfinite(np.linalg.cond(a))
    assert capsys.readouterr().out.count("SINGULAR MATRIX!") == 3


def test_verbosity_text_and_order(lsf, capsys):
    from levelsetfusion_python_amd.rigid_opt import sdf_2_sdf_optimizer2d as s2s
    opt = s2s.Sdf2SdfOptimizer2d(verbosity_parameters=s2s.Sdf2SdfOptimizer2d.VerbosityParameters(True, True))
    opt.optimize(_dataset(lsf, 32, np.array([-16, -16, 93.4375])), narrow_band_width_voxels=2., iteration=2)
    lines = capsys.readouterr().out.splitlines()
    r = opt.last_records
    want = []
    for i in range(2):
        want.append("%s[ITERATION %d COMPLETED]%s energy: %f" % (s2s.BOLD_LIGHT_CYAN, i, s2s.RESET, r[i]["energy"]))
        ts, tw = r[i]["twist_star"].reshape(-1), r[i]["twist"].reshape(-1)
        want.append("optimal twist: %f, %f, %f, twist: %f, %f, %f" % (ts[0], ts[1], ts[2], tw[0], tw[1], tw[2]))
    assert lines == want


def test_two_runs_bit_equal(lsf):
    data = _dataset(lsf, 128, np.array([-64, -64, 50.5]))
    a, b = lsf.Sdf2SdfOptimizer2d(), lsf.Sdf2SdfOptimizer2d()
    ta = a.optimize(data, iteration=5)
    tb = b.optimize(data, iteration=5)
    assert np.array_equal(ta, tb)
    for ra, rb in zip(a.last_records, b.last_records):
        for key in ("matrix_a", "vector_b", "twist", "twist_star"):
            assert np.array_equal(ra[key], rb[key])
        assert ra["energy"] == rb["energy"]


@pytest.mark.parametrize("n,off", [(512, np.array([-256, -256, -100.5])), (203, np.array([-101.25, -101, 10]))])
def test_large_and_ragged_fields_against_restatement(lsf, n, off):
    """512^2: the combine runs over 256 workgroups with several tiles each; 203 is not a multiple of the 16 x 16 tile"""
    from levelsetfusion_python_amd import image_io
    d0, d1 = image_io.read_depth_image(FRAMES[0]), image_io.read_depth_image(FRAMES[1])
    vs = 0.001
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    data = ArrayBasedSingleFrameDataset(d0, d1, 240, n, off, _camera(lsf, K))
    opt = lsf.Sdf2SdfOptimizer2d()
    twist = opt.optimize(data, voxel_size=vs, narrow_band_width_voxels=20., iteration=3)
    canonical = R.tsdf_nearest(d0, K, 0.001, (n, n), off, None, 20., 0.004, 240)
    records, want = R.optimize(canonical, d1, K, 0.001, 240, off, 3, 20., 0.01, vs)
    for rec, got in zip(records, opt.last_records):
        assert rec["skipped"] == got["skipped"] == 0
        np.testing.assert_allclose(got["matrix_a"], rec["A"], rtol=A_RTOL)
        np.testing.assert_allclose(got["vector_b"].reshape(3), rec["b"], rtol=A_RTOL)
        np.testing.assert_allclose(got["energy"], rec["energy"], rtol=A_RTOL)
    np.testing.assert_allclose(twist.reshape(3), want, rtol=0, atol=TWIST_ATOL)


def test_host_argument_checks_on_device(lsf):
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist
    from levelsetfusion_python_amd.tsdf import generation as gen
    with pytest.raises(ValueError, match="2-D field"):
        calculate_gradient_wrt_twist(np.zeros((1, 5), np.float32), np.zeros(3), [0, 0, 0])
    with pytest.raises(ValueError, match="2-D field"):
        calculate_gradient_wrt_twist(np.zeros((4, 4, 4), np.float32), np.zeros(3), [0, 0, 0])
    with pytest.raises(ValueError, match="3 entries"):
        calculate_gradient_wrt_twist(np.zeros((4, 4), np.float32), np.zeros(2), [0, 0, 0])
    with pytest.raises(ValueError, match="positive"):
        calculate_gradient_wrt_twist(np.zeros((4, 4), np.float32), np.zeros(3), [0, 0, 0], voxel_size=0)
    cam = _camera(lsf, K)
    with pytest.raises(ValueError, match="uint16"):
        gen.generate_2d_tsdf_field_from_depth_image(np.zeros((4, 4), np.int32), cam, 1, field_size=4)
    with pytest.raises(ValueError, match="nearest-pixel"):  # bilinear and EWA stay uint16
        gen.generate_2d_tsdf_field_from_depth_image(np.zeros((4, 4)), cam, 1, field_size=4,
                                                    interpolation_method=gen.FilteringMethod.BILINEAR_IMAGE_SPACE)
    g = calculate_gradient_wrt_twist(torch.zeros((4, 4), device="cuda"), np.zeros(3), [0, 0, 0], as_tensor=True)
    assert g.is_cuda and tuple(g.shape) == (4, 4, 3)
