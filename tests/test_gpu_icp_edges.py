"""GPU checks of the strided ICP (csrc/lsf_icp.hip: lsf_icp_run) on the ragged, adversarial pair of
tests/icp_edge_scene.py, against the numpy restatement (tests/icp_restatement.py): a 73 x 101 image that no stride and
no tile divides, a live frame with 0, negative, NaN and +inf depths, a prediction with depth > 0 under a zero normal,
and a start twist that projects live pixels out of the image.  The residual image is compared bit for bit, NaN at
off-stride pixels up to the last row and column; count and skipped exactly; A, b, the energy and the twist to the
tolerances of tests/test_gpu_icp.py.  tests/test_icp_edges_host.py checks the pair itself on the CPU."""
import numpy as np
import pytest
import torch

import icp_edge_scene as IS
from test_gpu_icp import SUM_RTOL, TWIST_ATOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(ratio):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=IS.K), depth_unit_ratio=ratio)


def _run(kind, iterations, strides, residuals=False):
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    image, ratio = IS.live(kind)
    pd, pn = IS.prediction()
    depth, code = device_depth(image)
    if residuals:  # the residual image is allocated uninitialised: leave a block of its size that is not NaN behind
        stale = torch.full(IS.IMAGE, 7.0, dtype=torch.float32, device="cuda")
        del stale
    return device_icp.icp_run(depth, code, torch.from_numpy(pd).cuda(), torch.from_numpy(pn).cuda(), _camera(ratio),
                              IS.twist_p(), IS.start_twist(), iterations, strides, max_distance=IS.MAX_DISTANCE,
                              residuals=residuals)


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


@pytest.mark.parametrize("kind", IS.LIVE_TYPES)
@pytest.mark.parametrize("stride", IS.STRIDES)
def test_one_iteration_on_the_ragged_pair(lsf, stride, kind):
    want, want_res, after = IS.restated_iteration(kind, stride)
    twist, records, res = _run(kind, (1,), (stride,), residuals=True)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] >= 5 and r["skipped"] == 0 and np.abs(r["matrix_a"]).min() > 0
    res = res.cpu().numpy()
    assert res.shape == IS.IMAGE and _bits_equal(res, want_res)
    off = np.ones(IS.IMAGE, bool)
    off[::stride, ::stride] = False
    assert np.isnan(res[off]).all() and int((~np.isnan(res)).sum()) == want["count"]  # up to the last row and column
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


@pytest.mark.parametrize("kind", IS.LIVE_TYPES)
def test_a_whole_pass_on_the_ragged_pair(lsf, kind):
    """(2, 2, 3) iterations over strides (4, 2, 1).  Against icp_restatement.icp, which runs free from the same start:
    count, skipped and level of every record exactly and every twist to 1e-9.  The sums are compared iteration by
    iteration with the restated iteration at the device's own previous twist: SUM_RTOL bounds the rounding of a sum
    taken in another order over the same terms, and from the second iteration on the free-running twists differ by
    their own 1e-13, which moves b by more than that (measured on the device: 6.1e-14 against a bound of 2.5e-14,
    where the first iteration, from identical inputs, is inside it).  The last residual image is bit for bit"""
    import icp_restatement as I
    iterations, strides = IS.PYRAMID
    free, free_twist = IS.restated_pass(kind)
    twist, records, res = _run(kind, iterations, strides, residuals=True)
    assert len(records) == len(free) == sum(iterations)
    image, ratio = IS.live(kind)
    pd, pn = IS.prediction()
    before = IS.start_twist()
    per_iteration = [s for n, s in zip(iterations, strides) for _ in range(n)]
    for got, f, stride in zip(records, free, per_iteration):
        with np.errstate(invalid="ignore"):  # the infinite depths
            want, want_res, _ = I.iteration(image, pd, pn, IS.K, ratio, before, IS.twist_p(), stride, IS.MAX_DISTANCE)
        r = _check_record(got, want)
        assert r["level"] == f["level"] and r["count"] == f["count"] >= 5 and r["skipped"] == f["skipped"] == 0
        np.testing.assert_allclose(r["twist"].ravel(), f["twist"], rtol=0, atol=TWIST_ATOL)
        before = got[6:12].copy()
    np.testing.assert_allclose(twist, free_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert _bits_equal(res.cpu().numpy(), want_res)


def test_reruns_are_bit_identical(lsf):
    a = _run("float32", *IS.PYRAMID, residuals=True)
    b = _run("float32", *IS.PYRAMID, residuals=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy())


@pytest.mark.parametrize("entry", ["icp_run", "icp_run_photometric", "icp_run_robust"])
def test_a_live_depth_that_is_not_what_its_code_says_is_refused(lsf, monkeypatch, entry):
    """an 8 x 8 float32 image given as float64 would be read past its end, given as uint16 misread; a 3-D tensor has no
    (H, W): each is a ValueError before any launch"""
    from levelsetfusion_python_amd import _lib, device_icp
    from levelsetfusion_python_amd.rigid_opt import RobustLoss

    def launched(*args):
        raise AssertionError("the library was called")
    for name in ("lsf_icp_run", "lsf_icp_run_photometric", "lsf_icp_run_robust"):
        monkeypatch.setattr(_lib.lib, name, launched)
    live = torch.ones((8, 8), dtype=torch.float32, device="cuda")
    pd, pn = torch.ones((8, 8), device="cuda"), torch.zeros((8, 8, 3), device="cuda")
    colour = dict(live_colour=torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"),
                  pred_colour=torch.zeros((8, 8, 4), device="cuda"), photometric_weight=0.1)
    zero = np.zeros(6)

    def run(depth, code):
        if entry == "icp_run":
            return device_icp.icp_run(depth, code, pd, pn, _camera(1.0), zero)
        if entry == "icp_run_photometric":
            return device_icp.icp_run_photometric(depth, code, colour["live_colour"], pd, pn, colour["pred_colour"],
                                                  _camera(1.0), zero, colour["photometric_weight"])
        return device_icp.icp_run_robust(depth, code, pd, pn, _camera(1.0), zero, RobustLoss("tukey", 0.01))
    for code in (_lib.DEPTH_F64, _lib.DEPTH_U16):
        with pytest.raises(ValueError, match="its depth_code says"):
            run(live, code)
    with pytest.raises(ValueError, match=r"\(H, W\) image"):
        run(torch.ones((2, 8, 8), dtype=torch.float32, device="cuda"), _lib.DEPTH_F32)
