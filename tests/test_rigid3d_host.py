"""CPU checks of the 6-DoF SDF-2-SDF rigid 3-D tracker's host half: the numpy restatement
(tests/rigid3d_restatement.py) against the reference's 2-D gradient answers (tests/golden/ref_rigid.npz), its recovery
of a known twist, the ctypes layout of lsf_rigid3d_params, host argument checks and the exports."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import rigid3d_restatement as R3
from conftest import ROOT, load_golden

PKG = os.path.join(ROOT, "levelsetfusion-python_amd")
K_SYN = np.array([[700.0, 0, 320], [0, 700.0, 240], [0, 0, 1]], dtype=np.float32)
# the recovery case: about one 4 mm voxel of translation and one degree of rotation on every axis, float32-representable
XI0 = np.array([0.004, -0.004, 0.004, 0.0175, -0.0175, 0.0175], dtype=np.float32).astype(np.float64)
# measured on the restatement (64^3, 60 iterations, rate 0.5): |twist - XI0| <= 1.3e-6 m in translation and <= 4.9e-6
# rad in rotation, energy 1.25e3 -> 1.4e-3 (profiles/rigid3d_cost.md); the tolerances keep a margin of about 4x
RECOVERY_ATOL_T, RECOVERY_ATOL_R = 5e-6, 2e-5


def _load(name, rel):  # host modules of the package, without loading the HIP library
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recovery_case(n=64):
    """canonical volume of synthetic.depth_image() under twist_vector_to_matrix3d(XI0); the live depth is the same image"""
    depth = _load("_t_synthetic", "synthetic.py").depth_image()
    off = np.array([-n // 2, -n // 2, 250 - n // 2], dtype=np.float64)
    canonical = R3.tsdf_nearest(depth, K_SYN, 0.001, (n, n, n), off, R3.matrix3d(XI0), 20, 0.004)
    return canonical, depth, off


def assert_recovered(twist, energies):
    err = np.abs(np.asarray(twist, dtype=np.float64).reshape(6) - XI0)
    assert np.all(err[:3] <= RECOVERY_ATOL_T) and np.all(err[3:] <= RECOVERY_ATOL_R), err
    assert energies[-1] < 1e-5 * energies[0]


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_rigid.npz")


def _y_constant(live2d, rows=3):
    return np.repeat(np.asarray(live2d, dtype=np.float32)[:, None, :], rows, axis=1)


@pytest.mark.parametrize("k", range(5))
def test_gradient_reduces_to_the_reference_2d_answers(ref, k):
    """a y-constant volume at r = 0: (t_x, t_z, r_y) is the reference's 2-D gradient in every y row, t_y is 0"""
    p = "grad.%d." % k
    t = ref[p + "twist"].reshape(3)
    assert t[2] == 0
    g = R3.gradient_wrt_twist_3d(_y_constant(ref[p + "live"]), [t[0], 0, t[1], 0, 0, 0], ref[p + "offset"],
                                 float(ref[p + "voxel_size"]))
    assert g.dtype == np.float32 and g.shape == ref[p + "live"].shape[:1] + (3,) + ref[p + "live"].shape[1:] + (6,)
    for y in range(3):
        # np.array_equal, as the 2-D restatement's test: the reference's dot product may give +0 where the
        # term-by-term form gives -0
        assert np.array_equal(g[:, y][..., [0, 2, 4]], ref[p + "out"])
    assert np.array_equal(g[..., 1].view(np.uint32), np.zeros(g.shape[:3], np.uint32))


def test_gradient_differs_from_the_2d_reference_at_nonzero_r_y(ref):
    """grad.5 (theta = 0.5): twist_vector_to_matrix2d(-twist) turns the x-z plane the other way from Rodrigues about y"""
    p = "grad.5."
    t = ref[p + "twist"].reshape(3)
    assert t[2] == 0.5
    g = R3.gradient_wrt_twist_3d(_y_constant(ref[p + "live"]), [t[0], 0, t[1], 0, t[2], 0], ref[p + "offset"],
                                 float(ref[p + "voxel_size"]))
    assert np.array_equal(g[:, 1][..., [0, 2]], ref[p + "out"][..., [0, 1]])
    assert not np.array_equal(g[:, 1][..., 4], ref[p + "out"][..., 2])
    # the x-z block of twist_vector_to_matrix3d(-twist) is the transpose of twist_vector_to_matrix2d(-twist)'s
    import rigid_restatement as R
    m3 = R3.matrix3d(-np.array([t[0], 0, t[1], 0, t[2], 0]))[[0, 2]][:, [0, 2]]
    m2 = R.matrix2d(-t)[:2, :2]
    assert np.allclose(m3, m2.T) and not np.allclose(m3, m2)


def test_singular_rule_6x6():
    a = np.diag([1.0, 2, 3, 4, 5, 6])
    assert R3.singular_class(a) == 0
    wall = a.copy()
    wall[[0, 1, 5], :] = 0
    wall[:, [0, 1, 5]] = 0
    assert R3.singular_class(wall) == 1 and not np.isfinite(np.linalg.cond(wall))
    assert R3.singular_class(np.zeros((6, 6))) == 1
    nan = a.copy()
    nan[2, 3] = np.nan
    assert R3.singular_class(nan) == 1
    assert R3.singular_class(np.diag([1e-300, 1, 1, 1, 1, 1])) == 0


def test_the_convention_converges():
    """the restatement's tracker, started at 0, recovers XI0 with the energy falling"""
    canonical, depth, off = recovery_case()
    records, twist = R3.optimize(canonical, depth, K_SYN, 0.001, off, 60, 20)
    assert all(r["skipped"] == 0 for r in records)
    energies = [r["energy"] for r in records]
    assert_recovered(twist, energies)
    # XI0 is nearly a fixed point: the canonical volume's rotation is Rodrigues in float64, the live one's is rounded
    # to float32, so a few voxels differ
    rec, after = R3.step(canonical, depth, K_SYN, 0.001, off, XI0, 20)
    assert rec["energy"] < 1e-9 * energies[0] and np.allclose(after, XI0, rtol=0, atol=1e-6)


def test_params_layout():
    import levelsetfusion_python_amd._lib as lib
    p = lib.Rigid3dParams
    names = [f[0] for f in p._fields_]
    assert names == ["tsdf", "array_offset", "voxel_size", "twist", "rate", "eta", "depth_dtype", "depth", "height",
                     "width", "iterations"]
    assert ctypes.sizeof(p) == ctypes.sizeof(lib.TsdfParams) + 8 * 3 + 8 + 8 * 6 + 8 + 4 * 6
    assert p.twist.size == 6 * 8 and p.twist.offset == p.voxel_size.offset + 8
    assert lib.RIGID3D_RECORD_DOUBLES == 64 and lib.RIGID3D_MAX_BLOCKS == 256
    assert lib.RIGID3D_SCRATCH_BYTES == 2 * 256 * 28 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for macro, value in (("LSF_RIGID3D_RECORD_DOUBLES", "64"), ("LSF_RIGID3D_MAX_BLOCKS", "256"),
                         ("LSF_RIGID3D_SCRATCH_BYTES", "(2 * LSF_RIGID3D_MAX_BLOCKS * 28 * 8)")):
        assert "#define %s %s" % (macro, value) in header
    for name in ("lsf_rigid3d_gradient", "lsf_rigid3d_run"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_rigid
    with pytest.raises(ValueError, match="6 entries"):
        device_rigid.twist6(np.zeros(3))
    assert device_rigid.twist6(np.zeros((6, 1))).shape == (6,)
    for bad in ((1, 4, 4), (4, 4), 1, (2, 2, 2, 2)):
        with pytest.raises(ValueError, match="three extents"):
            device_rigid.volume_shape(bad)
    assert device_rigid.volume_shape(5) == (5, 5, 5) and device_rigid.volume_shape((33, 17, 70)) == (33, 17, 70)
    with pytest.raises(ValueError, match="positive"):
        device_rigid._params3d((4, 4, 4), [0, 0, 0], 0.0)
    with pytest.raises(ValueError, match="3 entries"):
        device_rigid._params3d((4, 4, 4), [0, 0], 0.004)
    p = device_rigid._params3d((3, 4, 5), [0, 0, 0.5], 0.004)
    assert (p.depth, p.height, p.width) == (3, 4, 5) and p.array_offset[2] == 0.5


def test_the_c_abi_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    p = lib.Rigid3dParams()
    p.depth, p.height, p.width, p.voxel_size = 4, 4, 4, 0.004
    p.tsdf.image_width, p.tsdf.image_height, p.tsdf.narrow_band_half_width = 8, 8, 0.04
    buf = ctypes.c_void_p(16)  # never dereferenced: every call below is refused on the host
    for field, value in (("depth", 1), ("height", 1), ("width", 0), ("voxel_size", 0.0), ("iterations", -1),
                         ("depth_dtype", 7)):
        q = lib.Rigid3dParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.lib.lsf_rigid3d_run(buf, buf, buf, buf, buf, ctypes.byref(q), None) == -1, field
        if field not in ("iterations",):
            assert lib.lib.lsf_rigid3d_gradient(None, buf, buf, None, ctypes.byref(q), None) == -1, field
    assert lib.lib.lsf_rigid3d_gradient(None, None, buf, buf, ctypes.byref(p), None) == -1  # no input
    assert lib.lib.lsf_rigid3d_gradient(buf, None, None, None, ctypes.byref(p), None) == -1  # no output
    assert lib.lib.lsf_rigid3d_run(None, buf, buf, buf, buf, ctypes.byref(p), None) == -1
    assert lib.lib.lsf_rigid3d_run(buf, buf, buf, buf, buf, None, None) == -1
    q = lib.Rigid3dParams.from_buffer_copy(p)
    q.tsdf.narrow_band_half_width = 0.0
    assert lib.lib.lsf_rigid3d_run(buf, buf, buf, buf, buf, ctypes.byref(q), None) == -1


def test_package_exports_the_3d_tracker():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd.rigid_opt import sdf_2_sdf_optimizer3d, sdf_generation, sdf_gradient_field
    assert lsf.Sdf2SdfOptimizer3d is sdf_2_sdf_optimizer3d.Sdf2SdfOptimizer3d
    assert lsf.sdf_2_sdf_optimizer3d is sdf_2_sdf_optimizer3d and "Sdf2SdfOptimizer3d" in lsf.__all__
    assert callable(sdf_gradient_field.calculate_gradient_wrt_twist_3d)
    for cls in (sdf_generation.ImageBasedSingleFrameDataset, sdf_generation.ArrayBasedSingleFrameDataset):
        for name in ("generate_3d_canonical_field", "generate_3d_live_field", "generate_3d_sdf_fields"):
            assert callable(getattr(cls, name))
    opt = lsf.Sdf2SdfOptimizer3d()
    assert opt.rate == 0.5 and opt.last_records == []
    assert opt.verbosity_parameters.print_per_iteration_info is False
    r = np.arange(64, dtype=np.float64)
    rec = sdf_2_sdf_optimizer3d.unpack_record(r)
    assert rec["twist_star"].reshape(-1).tolist() == list(range(6)) and rec["twist"][0, 0] == 6
    assert rec["energy"] == 12 and rec["matrix_a"][0, 0] == 13 and rec["matrix_a"][5, 5] == 48
    assert rec["vector_b"][5, 0] == 54 and rec["skipped"] == 55


def test_no_cpu_path():
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd.rigid_opt.sdf_generation import ArrayBasedSingleFrameDataset
    from levelsetfusion_python_amd.rigid_opt.sdf_gradient_field import calculate_gradient_wrt_twist_3d
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d = np.full((8, 8), 600, np.uint16)
    data = ArrayBasedSingleFrameDataset(d, d, 4, 4, np.array([-2, -2, 140]),
                                        DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_SYN)))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        lsf.Sdf2SdfOptimizer3d().optimize(data, iteration=2)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        calculate_gradient_wrt_twist_3d(np.zeros((4, 4, 4), np.float32), np.zeros(6), [0, 0, 0])
