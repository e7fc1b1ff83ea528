"""GPU checks of the ray-cast colour image (lsf_raycast_colour, csrc/lsf_raycast.hip), of the joint geometric and
photometric ICP (lsf_icp_run_photometric, csrc/lsf_icp.hip; rigid_opt.ProjectiveIcp3d) and of
SequenceFusion3d(photometric_weight=) against the numpy restatement (tests/photometric_restatement.py).  The tolerances
are tests/test_gpu_icp.py's: per-pixel images and counts bit for bit; A, b and the energies to 1e-12 of the sum of their
terms' magnitudes; twists to 1e-9.  The accuracy bounds come from tests/test_photometric_host.py."""
import functools

import numpy as np
import pytest
import torch

import colour_scene as CS
import fusion_scene as S
import icp_restatement as I
import photometric_restatement as PR
import textured_wall_scene as W
from test_gpu_icp import SUM_RTOL, TWIST_ATOL
from test_photometric_host import (CAST_K, CAST_SHAPE, LAMBDA, RUN_ATOL_R, RUN_ATOL_T, RUN_ITERATIONS, RUN_STRIDES,
                                   SEQUENCE_ATOL_R, SEQUENCE_ATOL_T, SEQUENCE_COLOUR_BAND, SEQUENCE_FRAMES, SEQUENCE_N,
                                   restated_run, restated_sequence, sequence_frames, wall_inputs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera(K, ratio=1.0):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K), depth_unit_ratio=ratio)


def _dev(a):
    """a copy of a (possibly read-only) host array on the device"""
    return torch.from_numpy(np.array(a)).cuda()


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(live, ratio, image, pd, pn, pc, K, twist_p, twist, iterations, strides, lam=LAMBDA, gate=np.inf,
         residuals=False):
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    depth, code = device_depth(np.array(live))
    return device_icp.icp_run_photometric(depth, code, _dev(image), _dev(pd),
                                          _dev(pn), _dev(pc), _camera(K, ratio),
                                          twist_p, lam, twist, iterations, strides, max_intensity_difference=gate,
                                          residuals=residuals)


def _check_record(got, want):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"]
    assert r["photometric_count"] == want["photometric_count"] and r["angle_rejected"] == 0
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["photometric_energy"], want["photometric_energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    return r


@functools.lru_cache(maxsize=None)
def _restated_cast(fallback):
    """the restated ray-cast with colour of colour_scene's model at frame 1's twist, K / 8, 88 x 56"""
    t, w, c, _, _ = CS.restated_model()
    fb = _fallback_image() if fallback else None
    return PR.raycast_colour(t, w, c, CAST_K, S.true_twist(1), CS.offset(), CS.VOXEL, CAST_SHAPE, normals=True,
                             fallback=fb, ratio=0.001)


def _fallback_image():
    rows, cols = np.meshgrid(np.arange(CAST_SHAPE[0]), np.arange(CAST_SHAPE[1]), indexing="ij")
    return (600 + 3 * rows + cols).astype(np.uint16)


@pytest.mark.parametrize("fallback", [False, True])
def test_raycast_colour_against_restatement(lsf, fallback):
    """the colour image bit for bit with NaNs in the same places (pixels the fallback filled included); depth, normals
    and hit count bit-equal to lsf_raycast's on the same inputs and to the restatement.  88 x 56: both axes end in a
    partial 16 x 16 tile"""
    from levelsetfusion_python_amd import device_raycast
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    t, w, c = (_dev(a) for a in CS.restated_model()[:3])
    cam = _camera(CAST_K, 0.001)
    fb, code = device_depth(_fallback_image()) if fallback else (None, None)
    args = (t, w, cam, S.true_twist(1), CS.offset(), CS.VOXEL, CAST_SHAPE)
    depth, normals, hits, colour = device_raycast.raycast(*args, normals=True, fallback_depth=fb, fallback_code=code,
                                                          colour=c)
    plain = device_raycast.raycast(*args, normals=True, fallback_depth=fb, fallback_code=code)
    assert len(plain) == 3
    assert _bits_equal(depth.cpu().numpy(), plain[0].cpu().numpy())
    assert _bits_equal(normals.cpu().numpy(), plain[1].cpu().numpy()) and int(hits.item()) == int(plain[2].item())
    want_depth, want_normals, want_hits, want_colour = _restated_cast(fallback)
    assert _bits_equal(depth.cpu().numpy(), want_depth) and _bits_equal(normals.cpu().numpy(), want_normals)
    assert int(hits.item()) == want_hits
    got = colour.cpu().numpy()
    assert got.shape == CAST_SHAPE + (4,) and _bits_equal(got, want_colour)
    coloured = np.isfinite(got).all(axis=2)
    assert 2 * int(coloured.sum()) >= want_hits and np.isnan(got[~coloured]).all()
    if fallback:
        bare = _restated_cast(False)[0] > 0
        assert (~bare).sum() > 1000 and np.all(want_depth[~bare] > 0) and np.isnan(got[~bare]).all()
    # without normals the colour is the same
    _, none, _, again = device_raycast.raycast(*args, fallback_depth=fb, fallback_code=code, colour=c)
    assert none is None and _bits_equal(again.cpu().numpy(), want_colour)


def test_canonical_volume_raycast_colours(lsf):
    t, w, c = (_dev(a) for a in CS.restated_model()[:3])
    vol = lsf.fusion.CanonicalVolume(CS.N, colour=True)
    vol.tsdf.copy_(t)
    vol.weight.copy_(w)
    vol.colour.copy_(c)
    args = (_camera(CAST_K), S.true_twist(1), CS.offset(), CS.VOXEL, CAST_SHAPE)
    want = _restated_cast(False)
    depth, colour = vol.raycast(*args, colours=True)
    assert _bits_equal(depth, want[0]) and colour.dtype == np.float32 and _bits_equal(colour, want[3])
    depth, normals, colour = vol.raycast(*args, normals=True, colours=True, as_tensor=True)
    assert colour.is_cuda and _bits_equal(normals.cpu().numpy(), want[1]) and _bits_equal(colour.cpu().numpy(), want[3])
    assert _bits_equal(vol.raycast(*args), want[0])
    with pytest.raises(ValueError, match="colour=True"):
        lsf.fusion.CanonicalVolume(8).raycast(*args, colours=True)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_one_iteration_against_restatement(lsf, stride, dtype):
    """both residual images bit for bit, both counts equal, the sums and the twist at the tolerances of the ICP tests"""
    pd, pn, pc, depth, image = wall_inputs()
    live, ratio = W.live_depth(depth, dtype)
    start = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015])
    twist, records, res, ires = _run(live, ratio, image, pd, pn, pc, W.K_SMALL, np.zeros(6), start, (1,), (stride,),
                                     residuals=True)
    want, want_res, want_ires, after = PR.iteration(live, image, pd, pn, pc, W.K_SMALL, ratio, start, np.zeros(6),
                                                    LAMBDA, stride)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] > 1000 and 2 * r["photometric_count"] > r["count"]
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


def test_whole_run_against_restatement(lsf):
    """strides (4, 2, 1), iterations (4, 5, 10), lambda 0.1: every record against the restatement, the final twist
    within the host test's bound of the true one; lsf_icp_run on the same inputs skips every iteration.

    Every record is held to the restated run in its counts, level, skipped flag and twist (1e-9).  Its sums are held to
    1e-12 of their terms' magnitudes against the restated iteration taken at the twist the device itself entered the
    iteration with (the record before it): that tolerance is the rounding of one sum in another order and presumes one
    input.  The two runs' twists may differ by the 1e-9 above -- after the first solves they differ by a few ulps, the
    two inverses being different algorithms -- and A turns a twist difference d into a difference A d of b: here
    A[2][2] is the pair count, 17595, while the terms of b[2] sum to 0.06 in magnitude near convergence, so 1e-17 m of
    t_z moves b[2] by three times the tolerance (measured against the restated run's own record: 1.4e-13 against
    5.8e-14)."""
    from levelsetfusion_python_amd import device_icp
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    pd, pn, pc, depth, image = wall_inputs()
    twist, records, _, _ = _run(depth, 1.0, image, pd, pn, pc, W.K_SMALL, np.zeros(6), None, RUN_ITERATIONS,
                                RUN_STRIDES)
    want, want_twist = restated_run()
    assert len(records) == len(want) == 19
    entered = np.zeros(6)
    for got, w in zip(records, want):
        r = device_icp.unpack_record(got)
        assert (r["count"], r["photometric_count"], r["skipped"], r["level"]) == \
            (w["count"], w["photometric_count"], w["skipped"], w["level"])
        np.testing.assert_allclose(r["twist"].ravel(), w["twist"], rtol=0, atol=TWIST_ATOL)
        own, _, _, _ = PR.iteration(depth, image, pd, pn, pc, W.K_SMALL, 1.0, entered, np.zeros(6), LAMBDA,
                                    RUN_STRIDES[w["level"]])
        _check_record(got, own)
        entered = got[6:12].copy()
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    err = np.abs(twist - W.MOTION)
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R, err
    d, code = device_depth(np.array(depth))
    still, geometric, _ = device_icp.icp_run(d, code, _dev(pd), _dev(pn),
                                             _camera(W.K_SMALL), np.zeros(6), None, RUN_ITERATIONS, RUN_STRIDES)
    assert all(device_icp.unpack_record(r)["skipped"] == 1 for r in geometric) and len(geometric) == 19
    assert np.array_equal(still, np.zeros(6))


def test_gates(lsf):
    """a finite max_intensity_difference drops some terms and not all; a rectangle of NaN in pred_colour takes the
    photometric term from the pixels that project into it and leaves their geometric pair"""
    pd, pn, pc, depth, image = wall_inputs()
    start, zero = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015]), np.zeros(6)
    holed = pc.copy()
    holed[40:70, 50:100] = np.nan
    open_rec, open_res, open_ires, _ = PR.iteration(depth, image, pd, pn, pc, W.K_SMALL, 1.0, start, zero, LAMBDA)
    gate = float(np.nanmedian(np.abs(open_ires)))
    for colour, g in ((pc, gate), (holed, gate), (holed, np.inf)):
        want, want_res, want_ires, after = PR.iteration(depth, image, pd, pn, colour, W.K_SMALL, 1.0, start, zero,
                                                        LAMBDA, 1, I.MAX_DISTANCE, g)
        assert 0 < want["photometric_count"] < open_rec["photometric_count"] and want["count"] == open_rec["count"]
        assert _bits_equal(want_res, open_res)
        twist, records, res, ires = _run(depth, 1.0, image, pd, pn, colour, W.K_SMALL, zero, start, (1,), (1,),
                                         gate=g, residuals=True)
        _check_record(records[0], want)
        assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
        np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)
    lost = np.isnan(want_ires) & ~np.isnan(open_ires)  # the hole alone: the last case has no gate
    assert lost.sum() > 1000 and not lost[:30].any() and not lost[80:].any() and not np.isnan(want_res[lost]).any()


def test_second_trip_of_the_capped_grid(lsf):
    """272 x 256 at stride 1: 17 x 16 = 272 tiles against LSF_ICP_MAX_BLOCKS = 256 workgroups, so the first 16 take a
    second tile"""
    from levelsetfusion_python_amd import _lib
    shape = (256, 272)
    K = np.array([[300.0, 0, 136], [0, 300.0, 128], [0, 0, 1]], dtype=np.float32)
    assert ((shape[0] + 15) // 16) * ((shape[1] + 15) // 16) == 272 > _lib.ICP_MAX_BLOCKS
    pd, pn, pc = W.prediction(np.zeros(6), K, shape)
    depth, image, _ = W.render(W.MOTION, K, shape)
    start = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015])
    _, records, res, ires = _run(depth, 1.0, image, pd, pn, pc, K, np.zeros(6), start, (1,), (1,), residuals=True)
    want, want_res, want_ires, _ = PR.iteration(depth, image, pd, pn, pc, K, 1.0, start, np.zeros(6), LAMBDA)
    r = _check_record(records[0], want)
    assert r["count"] > 60000 and 2 * r["photometric_count"] > r["count"]
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    # the tiles of the second trip (256 .. 271: the bottom tile row but for its first tile) hold terms of both kinds
    assert np.isfinite(want_res[240:, 16:]).sum() > 1000 and np.isfinite(want_ires[240:, 16:]).sum() > 1000


def test_reruns_are_bit_identical(lsf):
    pd, pn, pc, depth, image = wall_inputs()
    live, ratio = W.live_depth(depth, np.uint16)
    runs = [_run(live, ratio, image, pd, pn, pc, W.K_SMALL, np.zeros(6), None, RUN_ITERATIONS, RUN_STRIDES,
                 residuals=True) for _ in range(2)]
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy()) and _bits_equal(a[3].cpu().numpy(), b[3].cpu().numpy())


def test_projective_icp3d_interface(lsf):
    pd, pn, pc, depth, image = wall_inputs()
    tracker = lsf.ProjectiveIcp3d(_camera(W.K_SMALL), RUN_ITERATIONS, RUN_STRIDES, photometric_weight=LAMBDA)
    twist = tracker.optimize(depth, pd, pn, np.zeros(6), residuals=True, colour_image=image, prediction_colour=pc)
    want, want_twist = restated_run()
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert [r["photometric_count"] for r in tracker.last_records] == [w["photometric_count"] for w in want]
    assert tracker.last_residuals.shape == tracker.last_intensity_residuals.shape == depth.shape
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        tracker.optimize(depth, pd, pn, np.zeros(6))


def test_sequence_against_restatement(lsf, capsys):
    """three frames of the wall, 64^3: counts equal, twists to 1e-9, the model's tsdf, weight and colour bit for bit
    against the restated sequence, and the tracking error within the host test's bound"""
    n = SEQUENCE_N
    frames = sequence_frames()
    want_t, want_w, want_c, twists, fusion, hits, icp = restated_sequence()
    seq = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), colour=True, colour_band=SEQUENCE_COLOUR_BAND,
                               tracking_reference="icp", photometric_weight=LAMBDA)
    for k, (depth, image) in enumerate(frames):
        rec = seq.integrate(depth, image)
        assert rec["prediction_hits"] == hits[k] and len(rec["rigid_records"]) == len(icp[k])
        for got, want in zip(rec["rigid_records"], icp[k]):
            assert got["count"] == want["count"] and got["photometric_count"] == want["photometric_count"]
            assert got["level"] == want["level"] and got["skipped"] == want["skipped"]
            np.testing.assert_allclose(got["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
        np.testing.assert_allclose(seq.twists[-1], twists[k], rtol=0, atol=TWIST_ATOL)
        assert rec["fusion"]["fused"] == fusion[k]["fused"] and rec["fusion"]["coloured"] == fusion[k]["coloured"]
    assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), want_t)
    assert _bits_equal(seq.canonical.weight.cpu().numpy(), want_w)
    assert _bits_equal(seq.canonical.colour.cpu().numpy(), want_c)
    assert tuple(seq.prediction_colour.shape) == (S.HEIGHT, S.WIDTH, 4) and seq.prediction_colour.is_cuda
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(SEQUENCE_FRAMES)]))
    with capsys.disabled():
        print("\nphotometric \"icp\" tracking, |twist - truth| per frame (m, rad):\n", np.array2string(err, precision=7))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err


def test_defaults_untouched(lsf):
    """without a weight the new keywords change nothing: twists, records and model equal a sequence built without
    them"""
    n = 48
    frames = [(d, c) for d, c, _ in CS.frames()[:3]]
    a = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), colour=True, tracking_reference="icp")
    b = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), colour=True, tracking_reference="icp",
                             photometric_weight=None, icp_max_intensity_difference=0.25)
    for depth, image in frames:
        ra, rb = a.integrate(depth, image), b.integrate(depth, image)
        assert ra["fusion"] == rb["fusion"] and ra["prediction_hits"] == rb["prediction_hits"]
        assert len(ra["rigid_records"]) == len(rb["rigid_records"])
        for x, y in zip(ra["rigid_records"], rb["rigid_records"]):
            assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
            assert x["photometric_count"] == 0 and x["photometric_energy"] == 0.0
    assert all(np.array_equal(x, y) for x, y in zip(a.twists, b.twists)) and b.prediction_colour is None
    for name in ("tsdf", "weight", "colour"):
        assert _bits_equal(getattr(a.canonical, name).cpu().numpy(), getattr(b.canonical, name).cpu().numpy())
    assert a.frame_records[1]["rigid_records"][-1]["skipped"] == 0
