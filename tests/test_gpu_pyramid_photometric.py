"""GPU checks of the intensity pyramids (lsf_intensity_pyramid, csrc/lsf_intensity_pyramid.hip; rigid_opt.IntensityPyramid),
of the joint geometric and photometric ICP over the depth pyramid (lsf_icp_run_pyramid_photometric, csrc/lsf_icp.hip;
ProjectiveIcp3d(pyramid=, intensity_pyramid=, photometric_weight=)) and of SequenceFusion3d(icp_intensity_pyramid=)
against the numpy restatement (tests/pyramid_photometric_restatement.py).  The intensity pyramids are compared bit for
bit.  The depth pyramid's level 0 may differ from numpy's in the last bit of the filter's exp
(tests/test_gpu_depth_pyramid.py), so the ICP restatements start from the device's own level 0.  The tolerances are
tests/test_gpu_icp.py's: per-pixel images and counts bit for bit; A, b and the energies to 1e-12 of the sum of their
terms' magnitudes; twists to 1e-9.  The accuracy bounds come from tests/test_pyramid_photometric_host.py."""
import functools

import numpy as np
import pytest
import torch

import depth_pyramid_restatement as DP
import fusion_scene as S
import pyramid_photometric_restatement as PP
import textured_wall_scene as W
from test_gpu_icp import SUM_RTOL, TWIST_ATOL
from test_photometric_host import (SEQUENCE_COLOUR_BAND, SEQUENCE_FRAMES, SEQUENCE_N, sequence_frames, wall_inputs)
from test_pyramid_photometric_host import (GATE_ANGLE, LAMBDA, LEVELS, PHOTOMETRIC_SHARE, RUN_ATOL_R, RUN_ATOL_T,
                                           RUN_ITERATIONS, SEQUENCE_ATOL_R, SEQUENCE_ATOL_T, holed_prediction,
                                           restated_pyramids, restated_run_from)

pytestmark = pytest.mark.gpu

START = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015])
ZERO = np.zeros(6)


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


def _device_pyramids(lsf, depth, image, pc, K, levels=LEVELS):
    """the three device pyramids of a frame and a prediction with the default settings, and the host copy of the depth
    pyramid's level 0"""
    pyr = lsf.rigid_opt.DepthPyramid(levels=levels).build(np.array(depth), _camera(K))
    ip = lsf.rigid_opt.IntensityPyramid(levels)
    return pyr, ip.build_device(_dev(image)), ip.build_prediction(_dev(pc)), pyr.depth[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _wall(lsf):
    """the wall's device pyramids and their restatement from the device's level 0; nothing modifies either"""
    pd, pn, pc, depth, image = wall_inputs()
    pyr, live, pred, level0 = _device_pyramids(lsf, depth, image, pc, W.K_SMALL)
    return pyr, live, pred, level0, restated_pyramids(level0)


def _run(pyr, live, pred, pd, pn, K, twist_p, twist, iterations, gate=None, lam=LAMBDA, gate_i=np.inf,
         residuals=True):
    from levelsetfusion_python_amd import device_icp
    return device_icp.icp_run_pyramid_photometric(*pyr.buffers, live.buffer, len(pyr.depth), _dev(pd), _dev(pn),
                                                  pred.buffer, _camera(K), twist_p, lam, twist, iterations,
                                                  max_normal_angle=gate, max_intensity_difference=gate_i,
                                                  residuals=residuals)


def _check_record(got, want):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"]
    assert r["photometric_count"] == want["photometric_count"] and r["angle_rejected"] == want["angle_rejected"]
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["photometric_energy"], want["photometric_energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    return r


def _pyramid_inputs(case):
    """(uint8 colour image, float32 (H, W, 4) prediction colour with NaNs) of an intensity pyramid test"""
    if case == "wall":  # 152 x 120: levels 76 x 60 and 38 x 30
        _, _, pc, _, image = wall_inputs()
        return image, holed_prediction(pc)
    rng = np.random.default_rng(11)
    if case == "odd":  # 75 x 53: levels 37 x 26 and 18 x 13, the last row and column of the input are never read
        shape = (53, 75)
        pc = rng.random(shape + (4,)).astype(np.float32)
        pc[rng.random(shape) < 0.05] = np.nan
        pc[52, :, 3] = np.inf
        pc[:, 74, 3] = np.nan
    else:  # colour_scene's model seen in 88 x 56 pixels: silhouette NaNs
        from test_gpu_photometric import _restated_cast
        pc = _restated_cast(False)[3]
        shape = pc.shape[:2]
        assert shape == (56, 88) and np.isnan(pc[..., 3]).sum() > 500 and np.isfinite(pc[..., 3]).sum() > 500
    return rng.integers(0, 256, shape + (3,), dtype=np.uint8), pc


@pytest.mark.parametrize("case", ["wall", "odd", "cast"])
def test_intensity_pyramids_against_restatement(lsf, case):
    """both sources bit for bit with NaNs in the same places, every level, and the buffer holding them back to back"""
    image, pc = _pyramid_inputs(case)
    ip = lsf.rigid_opt.IntensityPyramid(LEVELS)
    h, w = image.shape[:2]
    for got, want in ((ip.build_device(_dev(image)), PP.live_pyramid(image, LEVELS)),
                      (ip.build_prediction(_dev(pc)), PP.prediction_pyramid(pc, LEVELS))):
        assert [tuple(l.shape) for l in got.intensity] == [(h >> l, w >> l) for l in range(LEVELS)]
        for l in range(LEVELS):
            assert _bits_equal(got.intensity[l].cpu().numpy(), want[l]), l
        assert _bits_equal(got.buffer.cpu().numpy(), np.concatenate([l.ravel() for l in want]))
    nans = [int(np.isnan(l).sum()) for l in want]
    assert nans[0] > 0 and nans[-1] > 0 and np.isfinite(want[-1]).sum() > 0
    one = lsf.rigid_opt.IntensityPyramid(1).build_device(_dev(image))
    assert len(one.intensity) == 1 and _bits_equal(one.buffer.cpu().numpy(), PP.live_level0(image).ravel())


def test_intensity_pyramid_wrapper_refuses_bad_images(lsf):
    from levelsetfusion_python_amd import device_intensity_pyramid as D
    image, pc = _pyramid_inputs("wall")
    for bad, source in ((image, "colour"), (_dev(image), "prediction"), (_dev(pc), "colour"), (_dev(pc)[..., :3], "colour"),
                        (_dev(image)[:, ::2], "colour"), (_dev(image), "grey")):
        with pytest.raises(ValueError):
            D.intensity_pyramid(bad, source, 3)
    with pytest.raises(ValueError, match="no 4-level pyramid"):
        D.intensity_pyramid(_dev(image)[:7].contiguous(), "colour", 4)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_one_iteration_against_restatement(lsf, level, gate):
    """one iteration on each pyramid level (152 x 120, 76 x 60, 38 x 30: all end in partial tiles), gate off and on:
    both residual images and the three counts bit for bit, the sums and the twist at the tolerances of the ICP tests"""
    pd, pn, _, _, _ = wall_inputs()
    pyr, live, pred, _, (lv, il, ip) = _wall(lsf)
    angle = GATE_ANGLE if gate else None
    twist, records, res, ires = _run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, START, (1,) + (0,) * level, angle)
    want, want_res, want_ires, after = PP.iteration(lv[0][level], lv[1][level], il[level], ip[level], lv[2][level],
                                                    pd, pn, W.K_SMALL, START, ZERO, LAMBDA,
                                                    cos_max=DP.cos_of(angle) if gate else None)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] > 1000 and r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"]
    assert (r["angle_rejected"] > 0) == gate
    assert tuple(res.shape) == tuple(ires.shape) == (W.SHAPE_SMALL[0] >> level, W.SHAPE_SMALL[1] >> level)
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


def test_whole_run_against_restatement(lsf):
    """iterations (4, 4, 6) with the 20 degree gate.  Every record is held to the independent restated run in its
    counts, level, skipped flag and twist (1e-9), and its sums to 1e-12 of their terms' magnitudes against the restated
    iteration taken at the twist the device itself entered the iteration with: the method of
    tests/test_gpu_photometric.py, whose whole-run test says why.  The final twist lies within the host test's bound of
    the true one, and lsf_icp_run_pyramid on the same pyramid skips every iteration"""
    from levelsetfusion_python_amd import device_icp
    pd, pn, _, _, _ = wall_inputs()
    pyr, live, pred, level0, (lv, il, ip) = _wall(lsf)
    twist, records, res, ires = _run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, None, RUN_ITERATIONS, GATE_ANGLE)
    want, want_twist, want_res, want_ires = restated_run_from(level0)
    assert len(records) == len(want) == 14
    entered = np.zeros(6)
    for got, w in zip(records, want):
        r = device_icp.unpack_record(got)
        assert (r["count"], r["photometric_count"], r["angle_rejected"], r["skipped"], r["level"]) == \
            (w["count"], w["photometric_count"], w["angle_rejected"], w["skipped"], w["level"])
        assert r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"]
        np.testing.assert_allclose(r["twist"].ravel(), w["twist"], rtol=0, atol=TWIST_ATOL)
        l = LEVELS - 1 - w["level"]
        own, _, _, _ = PP.iteration(lv[0][l], lv[1][l], il[l], ip[l], lv[2][l], pd, pn, W.K_SMALL, entered, ZERO,
                                    LAMBDA, cos_max=DP.cos_of(GATE_ANGLE))
        _check_record(got, own)
        entered = got[6:12].copy()
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert np.isfinite(res.cpu().numpy()).sum() == want[-1]["count"]
    assert np.isfinite(ires.cpu().numpy()).sum() == want[-1]["photometric_count"]
    err = np.abs(twist - W.MOTION)
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R, err
    still, geometric, _ = device_icp.icp_run_pyramid(*pyr.buffers, LEVELS, _dev(pd), _dev(pn), _camera(W.K_SMALL), ZERO,
                                                     None, RUN_ITERATIONS, max_normal_angle=GATE_ANGLE)
    assert all(device_icp.unpack_record(r)["skipped"] == 1 for r in geometric) and len(geometric) == 14
    assert np.array_equal(still, ZERO)


@pytest.mark.parametrize("gate", [False, True])
def test_second_trip_of_the_capped_grid(lsf, gate):
    """one level and one iteration at 272 x 256: 17 x 16 = 272 tiles against LSF_ICP_MAX_BLOCKS = 256 workgroups, so
    the first 16 take a second tile, in both instantiations of the new source"""
    from levelsetfusion_python_amd import _lib
    shape = (256, 272)
    K = np.array([[300.0, 0, 136], [0, 300.0, 128], [0, 0, 1]], dtype=np.float32)
    assert ((shape[0] + 15) // 16) * ((shape[1] + 15) // 16) == 272 > _lib.ICP_MAX_BLOCKS
    pd, pn, pc = W.prediction(ZERO, K, shape)
    depth, image, _ = W.render(W.MOTION, K, shape)
    pyr, live, pred, level0 = _device_pyramids(lsf, depth, image, pc, K, 1)
    angle = GATE_ANGLE if gate else None
    _, records, res, ires = _run(pyr, live, pred, pd, pn, K, ZERO, START, (1,), angle)
    lv = DP.pyramid_from_level0(level0, K, 1)
    want, want_res, want_ires, _ = PP.iteration(lv[0][0], lv[1][0], PP.live_level0(image), PP.prediction_level0(pc),
                                                lv[2][0], pd, pn, K, START, ZERO, LAMBDA,
                                                cos_max=DP.cos_of(angle) if gate else None)
    r = _check_record(records[0], want)
    assert r["count"] > 60000 and r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"]
    assert (r["angle_rejected"] > 0) == gate
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    # the tiles of the second trip (256 .. 271: the bottom tile row but for its first tile) hold terms of both kinds
    assert np.isfinite(want_res[240:, 16:]).sum() > 1000 and np.isfinite(want_ires[240:, 16:]).sum() > 1000


def test_max_intensity_difference(lsf):
    """a finite gate on |r_I| (the open iteration's median) drops some photometric terms and not all, on the middle
    level; the geometric pairs stay"""
    pd, pn, _, _, _ = wall_inputs()
    pyr, live, pred, _, (lv, il, ip) = _wall(lsf)
    args = (lv[0][1], lv[1][1], il[1], ip[1], lv[2][1], pd, pn, W.K_SMALL, START, ZERO, LAMBDA)
    open_rec, open_res, open_ires, _ = PP.iteration(*args)
    gate = float(np.nanmedian(np.abs(open_ires)))
    want, want_res, want_ires, after = PP.iteration(*args, max_difference=gate)
    assert 0 < want["photometric_count"] < open_rec["photometric_count"] <= want["count"] == open_rec["count"]
    twist, records, res, ires = _run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, START, (1, 0), gate_i=gate)
    r = _check_record(records[0], want)
    assert 0 < r["photometric_count"] < r["count"]
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(res.cpu().numpy(), open_res)
    assert _bits_equal(ires.cpu().numpy(), want_ires)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


def test_a_hole_in_the_prediction_s_colour(lsf):
    """NaNs in the prediction's Y spread by one block a level, take the photometric term from the pixels that
    interpolate across them and leave their geometric pair"""
    pd, pn, pc, depth, image = wall_inputs()
    holed = holed_prediction(pc)
    pyr, live, _, _, (lv, il, _) = _wall(lsf)
    pred = lsf.rigid_opt.IntensityPyramid(LEVELS).build_prediction(_dev(holed))
    ip = PP.prediction_pyramid(holed, LEVELS)
    for level in (0, 2):
        want, want_res, want_ires, _ = PP.iteration(lv[0][level], lv[1][level], il[level], ip[level], lv[2][level], pd,
                                                    pn, W.K_SMALL, START, ZERO, LAMBDA)
        _, records, res, ires = _run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, START, (1,) + (0,) * level)
        _check_record(records[0], want)
        assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
        lost = np.isnan(want_ires) & np.isfinite(want_res)
        assert lost.sum() > (1000 >> (2 * level)) and want["photometric_count"] > 0


def test_zero_iterations_and_reruns(lsf):
    """a call without iterations launches nothing and returns the twist it was given; two runs are bit-identical"""
    pd, pn, _, _, _ = wall_inputs()
    pyr, live, pred, _, _ = _wall(lsf)
    twist, records, res, ires = _run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, START, (0, 0, 0))
    assert np.array_equal(twist, START) and records.shape == (0, 64)
    twist, records, _, _ = _run(pyr, live, pred, pd, pn, W.K_SMALL, START, None, (0,), residuals=False)
    assert np.array_equal(twist, START) and records.shape == (0, 64)
    a, b = (_run(pyr, live, pred, pd, pn, W.K_SMALL, ZERO, None, RUN_ITERATIONS, GATE_ANGLE) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy()) and _bits_equal(a[3].cpu().numpy(), b[3].cpu().numpy())


def test_projective_icp3d_interface(lsf):
    pd, pn, pc, depth, image = wall_inputs()
    make = functools.partial(lsf.ProjectiveIcp3d, _camera(W.K_SMALL), RUN_ITERATIONS,
                             pyramid=lsf.rigid_opt.DepthPyramid(), max_normal_angle=GATE_ANGLE)
    tracker = make(intensity_pyramid=lsf.rigid_opt.IntensityPyramid(), photometric_weight=LAMBDA)
    twist = tracker.optimize(depth, pd, pn, ZERO, residuals=True, colour_image=image, prediction_colour=pc)
    level0 = tracker.last_pyramid.depth[0].cpu().numpy()
    want, want_twist, _, _ = restated_run_from(level0)
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    for key in ("count", "photometric_count", "angle_rejected", "skipped", "level"):
        assert [r[key] for r in tracker.last_records] == [w[key] for w in want], key
    assert all(r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"] for r in tracker.last_records)
    err = np.abs(twist - W.MOTION)
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R, err
    assert tuple(tracker.last_residuals.shape) == tuple(tracker.last_intensity_residuals.shape) == depth.shape
    live, pred = tracker.last_intensity_pyramids
    _, il, ip = restated_pyramids(level0)
    assert all(_bits_equal(live.intensity[l].cpu().numpy(), il[l]) for l in range(LEVELS))
    assert all(_bits_equal(pred.intensity[l].cpu().numpy(), ip[l]) for l in range(LEVELS))
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        tracker.optimize(depth, pd, pn, ZERO)
    # the same pyramid tracker without the term: every iteration is skipped, the twist stays
    plain = make()
    assert np.array_equal(plain.optimize(depth, pd, pn, ZERO), ZERO)
    assert len(plain.last_records) == 14 and all(r["skipped"] == 1 and r["count"] > 1000 for r in plain.last_records)
    assert plain.last_intensity_pyramids is None


def test_sequence_within_the_host_test_s_bound(lsf, capsys):
    """three frames of the wall, 64^3, tracked on the pyramid with the term: every record updates with most pairs
    carrying a photometric term, the tracking error stays within the host test's bound, and the same sequence without
    the term skips frame 1's iterations"""
    n = SEQUENCE_N
    frames = sequence_frames()
    kw = dict(colour=True, colour_band=SEQUENCE_COLOUR_BAND, tracking_reference="icp", icp_iterations=RUN_ITERATIONS,
              icp_pyramid=lsf.rigid_opt.DepthPyramid(), icp_max_normal_angle=GATE_ANGLE)
    seq = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), photometric_weight=LAMBDA,
                               icp_intensity_pyramid=lsf.rigid_opt.IntensityPyramid(), **kw)
    for k, (depth, image) in enumerate(frames):
        rec = seq.integrate(depth, image)
        assert len(rec["rigid_records"]) == (14 if k else 0)
        for r in rec["rigid_records"]:
            assert r["skipped"] == 0 and r["count"] > 1000 and r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"]
        assert rec["fusion"]["fused"] > 0 and rec["fusion"]["coloured"] > 0
    assert tuple(seq.prediction_colour.shape) == (S.HEIGHT, S.WIDTH, 4) and seq.prediction_colour.is_cuda
    assert len(seq.icp.last_pyramid.depth) == LEVELS and len(seq.icp.last_intensity_pyramids[1].intensity) == LEVELS
    assert _bits_equal(seq.icp.last_intensity_pyramids[1].intensity[0].cpu().numpy(),
                       seq.prediction_colour[..., 3].cpu().numpy())
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(SEQUENCE_FRAMES)]))
    with capsys.disabled():
        print("\njoint pyramid \"icp\" tracking, |twist - truth| per frame (m, rad):\n",
              np.array2string(err, precision=7))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err
    plain = lsf.SequenceFusion3d(_camera(S.K), n, S.offset(n), **kw)
    for depth, image in frames[:2]:
        rec = plain.integrate(depth, image)
    assert len(rec["rigid_records"]) == 14 and all(r["skipped"] == 1 for r in rec["rigid_records"])
