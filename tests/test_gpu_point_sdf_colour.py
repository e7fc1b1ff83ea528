"""GPU checks of point-to-SDF tracking with the colour term and on the depth pyramid (csrc/lsf_point_sdf.hip:
lsf_point_sdf_run_photometric, lsf_point_sdf_run_pyramid; rigid_opt.PointToSdf3d) against the numpy restatement
(tests/point_sdf_colour_restatement.py), and of SequenceFusion3d(colour=True, tracking_reference="sdf") with such a
tracker.  The scene is tests/textured_wall_scene.py seen by tests/fusion_scene.py's camera, 640 x 480, against the 64^3
model of frame 0 (tests/test_point_sdf_colour_host.py).  The tolerances are tests/test_gpu_point_sdf.py's: per-pixel
values (both residual images, the weight image, the three counts) bit for bit; A, b, both energies and the weight sums,
which the device reduces in a tree, to 1e-12 of the sum of their terms' magnitudes; twists to 1e-9.  The depth
pyramid's level 0 may differ from numpy's in the last bit of the filter's exp (tests/test_gpu_depth_pyramid.py), so the
pyramid restatements start from the device's own level 0.  The accuracy bounds are twice the errors
tests/test_point_sdf_colour_host.py measures on the CPU."""
import functools

import numpy as np
import pytest
import torch

import depth_pyramid_restatement as DP
import fusion_scene as S
import point_sdf_colour_restatement as PC
import point_sdf_restatement as P
import pyramid_photometric_restatement as PP
import robust_icp_restatement as RR
import textured_wall_scene as W
from test_gpu_icp import NON_CUBIC, SUM_RTOL, TWIST_ATOL, _bits_equal, _camera
from test_point_sdf_colour_host import (COLOUR_BAND, LAMBDA, N, NON_CUBIC_ATOL_R, NON_CUBIC_ATOL_T, RUN_ATOL_R,
                                        RUN_ATOL_T, SEQUENCE_ATOL_R, SEQUENCE_ATOL_T, twist_errors, wall_frames,
                                        wall_model)

pytestmark = pytest.mark.gpu

START = S.true_twist(0)
PERTURBED = S.true_twist(0) + np.array([4e-4, -3e-4, 2e-4, 1e-3, -2e-3, 1.5e-3])
# on frame 1 from frame 0's twist |r| reaches 9.6 mm and |r_I| 0.28 (95 % below 0.2): both terms have outliers
TUKEY = RR.Loss("tukey", 0.008, 0.2)


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _dev(a):
    """a copy of a (possibly read-only) host array on the device"""
    return torch.from_numpy(np.array(a)).cuda()


def _loss(loss):
    from levelsetfusion_python_amd.rigid_opt import RobustLoss
    return None if loss is None else RobustLoss(loss.kind, loss.scale, loss.intensity_scale)


def _model(volume="64"):
    if volume == "64":
        return wall_model()
    shape, off = NON_CUBIC
    return wall_model(shape, tuple(float(v) for v in off))


def _strided(model, live, ratio, image, twist, iterations=P.ITERATIONS, strides=P.STRIDES, loss=None, lam=LAMBDA,
             gate=np.inf, residuals=True):
    """device_point_sdf.point_sdf_run_photometric of the model (tsdf, weight, colour, offset); lam None: geometry"""
    from levelsetfusion_python_amd import device_point_sdf
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    t, w, c, off = model
    depth, code = device_depth(live)
    joint = {} if lam is None else dict(colour=_dev(c), live_colour=_dev(image), photometric_weight=lam,
                                        max_intensity_difference=gate)
    return device_point_sdf.point_sdf_run_photometric(_dev(t), _dev(w), depth, code, _camera(ratio), off, twist,
                                                      iterations=iterations, strides=strides, robust=_loss(loss),
                                                      residuals=residuals, **joint)


@functools.lru_cache(maxsize=None)
def _device_pyramids(levels=3, radius=DP.RADIUS):
    """frame 1's device depth pyramid and intensity pyramid, the host copy of the depth pyramid's level 0 and the
    restated pyramids from it; nothing modifies them"""
    import levelsetfusion_python_amd as lsf
    depth, image = wall_frames()[1]
    pyr = lsf.rigid_opt.DepthPyramid(levels=levels, radius=radius).build(np.array(depth), _camera())
    live = lsf.rigid_opt.IntensityPyramid(levels).build_device(_dev(image))
    level0 = pyr.depth[0].cpu().numpy()
    depths, _, intr = DP.pyramid_from_level0(level0, S.K, levels)
    return pyr, live, depths, intr, PP.live_pyramid(image, levels)


def _pyramid(model, pyr, live, twist, iterations=P.ITERATIONS, loss=None, lam=LAMBDA, gate=np.inf, residuals=True):
    from levelsetfusion_python_amd import device_point_sdf
    t, w, c, off = model
    joint = {} if lam is None else dict(colour=_dev(c), pyramid_intensity=live.buffer, photometric_weight=lam,
                                        max_intensity_difference=gate)
    return device_point_sdf.point_sdf_run_pyramid(_dev(t), _dev(w), pyr.buffers[0], len(pyr.depth), (480, 640),
                                                  _camera(), off, twist, iterations=iterations, robust=_loss(loss),
                                                  residuals=residuals, **joint)


def _check_record(got, want, robust=False):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"]
    assert r["angle_rejected"] == want["no_sample"]  # slot 58: the pixels with a depth and no valid sample
    assert r["photometric_count"] == want["photometric_count"]
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["photometric_energy"], want["photometric_energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    if robust:
        np.testing.assert_allclose(r["weight_sum"], want["weight_sum"], rtol=SUM_RTOL)
        np.testing.assert_allclose(r["photometric_weight_sum"], want["photometric_weight_sum"], rtol=SUM_RTOL)
        assert r["outliers"] == want["outliers"]
    else:
        assert r["weight_sum"] == 0.0 and r["photometric_weight_sum"] == 0.0 and r["outliers"] == 0
    return r


def _check_run(records, start, iterations, iterate, robust=False):
    """every record of a whole run against the restated iteration taken at the twist the device itself entered the
    iteration with (the record before it), as tests/test_gpu_photometric.py does: the sums' tolerance is the rounding of
    one sum in another order and presumes one input, while two whole runs' twists drift apart by a few ulps after the
    first solves (the two inverses are different algorithms), which A turns into more than that tolerance of b near
    convergence.  iterate(entered twist, entry of iterations) is point_sdf_colour_restatement.iteration's result.
    Returns the last iteration's restated (residual image, intensity residual image, weight image)"""
    levels = [k for k, n in enumerate(iterations) for _ in range(n)]
    assert len(records) == len(levels)
    entered, images = np.asarray(start, np.float64), None
    for got, level in zip(records, levels):
        own, res, ires, weights, _ = iterate(entered, level)
        r = _check_record(got, own, robust)
        assert r["level"] == level
        entered, images = got[6:12].copy(), (res, ires, weights)
    return images


@pytest.mark.parametrize("stride", [1, 3])
def test_one_strided_joint_iteration_against_restatement(lsf, stride):
    """640 x 480 has 1200 tiles at stride 1, against 256 workgroups: the grid-stride loop's later trips; 640 / 3 is
    ragged.  Both residual images bit for bit (NaN where a pixel has no pair / no term, or is off the stride), the
    three counts exactly"""
    model = _model()
    t, w, c, off = model
    depth, image = wall_frames()[1]
    twist, records, res, ires, weights = _strided(model, depth, 1.0, image, PERTURBED, (1,), (stride,))
    want, want_res, want_ires, _, after = PC.iteration(t, w, PC.strided_source(depth, S.K, 1.0, stride, image),
                                                       PERTURBED, off, colour=c, lam=LAMBDA)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] > 500 and 2 * r["photometric_count"] > r["count"] and weights is None
    assert r["angle_rejected"] > 0
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


def test_the_intensity_pyramid_of_the_frame(lsf):
    _, live, _, _, want = _device_pyramids()
    for got, level in zip(live.intensity, want):
        assert _bits_equal(got.cpu().numpy(), level)


@pytest.mark.parametrize("entry", [0, 1, 2])
def test_one_pyramid_joint_iteration_on_each_level(lsf, entry):
    """entry k of (.., 1, ..) runs on level 2 - k: 160 x 120, 320 x 240 and 640 x 480; the images have that level's
    extents and record slot 57 is the entry index"""
    model = _model()
    t, w, c, off = model
    pyr, live, depths, intr, intensities = _device_pyramids()
    iterations = tuple(1 if k == entry else 0 for k in range(3))
    level = 2 - entry
    twist, records, res, ires, _ = _pyramid(model, pyr, live, PERTURBED, iterations)
    source = PC.pyramid_source(depths[level], intr[level], intensities[level])
    want, want_res, want_ires, _, after = PC.iteration(t, w, source, PERTURBED, off, colour=c, lam=LAMBDA)
    r = _check_record(records[0], want)
    assert r["level"] == entry and r["count"] > 200 and 2 * r["photometric_count"] > r["count"]
    assert tuple(res.shape) == tuple(ires.shape) == (480 >> level, 640 >> level)
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
def test_whole_strided_joint_run_against_restatement(lsf, dtype):
    model = _model()
    t, w, c, off = model
    depth, image = wall_frames()[1]
    live, ratio = W.live_depth(np.array(depth), dtype)
    twist, records, res, ires, _ = _strided(model, live, ratio, image, START)
    sources = [PC.strided_source(live, S.K, ratio, s, image) for s in P.STRIDES]
    want_res, want_ires, _ = _check_run(records, START, P.ITERATIONS, lambda tw, k: PC.iteration(
        t, w, sources[k], tw, off, colour=c, lam=LAMBDA))
    assert len(records) == 14 and not records[:, 55].any()
    assert np.array_equal(twist, records[-1][6:12])
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    err = np.abs(twist - S.true_twist(1))
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R, err


@pytest.mark.parametrize("volume", ["64", "non-cubic"])
def test_whole_pyramid_joint_run_against_restatement(lsf, volume):
    model = _model(volume)
    t, w, c, off = model
    pyr, live, depths, intr, intensities = _device_pyramids()
    twist, records, res, ires, _ = _pyramid(model, pyr, live, START)
    sources = [PC.pyramid_source(depths[2 - k], intr[2 - k], intensities[2 - k]) for k in range(3)]
    want_res, want_ires, _ = _check_run(records, START, P.ITERATIONS, lambda tw, k: PC.iteration(
        t, w, sources[k], tw, off, colour=c, lam=LAMBDA))
    assert len(records) == 14 and not records[:, 55].any() and np.array_equal(twist, records[-1][6:12])
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    err = np.abs(twist - S.true_twist(1))
    atol_t, atol_r = (RUN_ATOL_T, RUN_ATOL_R) if volume == "64" else (NON_CUBIC_ATOL_T, NON_CUBIC_ATOL_R)
    assert err[:3].max() <= atol_t and err[3:].max() <= atol_r, err


def test_a_block_of_colour_weights_set_to_zero(lsf):
    """the geometric residual is unchanged there, r_I is NaN exactly where the restatement's is, and the photometric
    count drops"""
    t, w, c, off = _model()
    holed = np.array(c)
    assert np.all(c[41:46, 26:36, 28:40, 3] > 0)  # the wall's coloured band crosses the volume at z = 41 .. 45
    holed[:, 26:36, 28:40, 3] = 0.0
    depth, image = wall_frames()[1]
    source = PC.strided_source(depth, S.K, 1.0, 1, image)
    _, records, res, ires, _ = _strided((t, w, holed, off), depth, 1.0, image, PERTURBED, (1,), (1,))
    want, want_res, want_ires, _, _ = PC.iteration(t, w, source, PERTURBED, off, colour=holed, lam=LAMBDA)
    whole, whole_res, whole_ires, _, _ = PC.iteration(t, w, source, PERTURBED, off, colour=c, lam=LAMBDA)
    lost = np.isfinite(whole_ires) & np.isnan(want_ires)
    assert lost.sum() > 50 and want["photometric_count"] == whole["photometric_count"] - lost.sum()
    assert want["count"] == whole["count"] and _bits_equal(want_res, whole_res)
    got = ires.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want_ires)) and _bits_equal(got, want_ires)
    assert _bits_equal(res.cpu().numpy(), whole_res)
    _check_record(records[0], want)


def test_a_finite_intensity_gate(lsf):
    """the gate is the 80 % quantile of the ungated |r_I| on the CPU: a fifth of the terms fail"""
    model = _model()
    t, w, c, off = model
    depth, image = wall_frames()[1]
    source = PC.strided_source(depth, S.K, 1.0, 1, image)
    whole, _, whole_ires, _, _ = PC.iteration(t, w, source, PERTURBED, off, colour=c, lam=LAMBDA)
    gate = float(np.quantile(np.abs(whole_ires[np.isfinite(whole_ires)]).astype(np.float64), 0.8))
    want, want_res, want_ires, _, _ = PC.iteration(t, w, source, PERTURBED, off, colour=c, lam=LAMBDA,
                                                   max_difference=gate)
    failed = whole["photometric_count"] - want["photometric_count"]
    assert 0.05 * whole["photometric_count"] < failed < 0.5 * whole["photometric_count"]
    _, records, res, ires, _ = _strided(model, depth, 1.0, image, PERTURBED, (1,), (1,), gate=gate)
    _check_record(records[0], want)
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)


@pytest.mark.parametrize("source", ["strided", "pyramid"])
def test_tukey_on_both_terms_against_restatement(lsf, source):
    model = _model()
    t, w, c, off = model
    depth, image = wall_frames()[1]
    if source == "strided":
        twist, records, res, ires, weights = _strided(model, depth, 1.0, image, START, loss=TUKEY)
        sources = [PC.strided_source(depth, S.K, 1.0, s, image) for s in P.STRIDES]
    else:
        pyr, live, depths, intr, intensities = _device_pyramids()
        twist, records, res, ires, weights = _pyramid(model, pyr, live, START, loss=TUKEY)
        sources = [PC.pyramid_source(depths[2 - k], intr[2 - k], intensities[2 - k]) for k in range(3)]
    want_res, want_ires, want_weights = _check_run(records, START, P.ITERATIONS, lambda tw, k: PC.iteration(
        t, w, sources[k], tw, off, colour=c, lam=LAMBDA, loss=TUKEY), robust=True)
    assert records[0][63] > 0 and 0 < records[0][62] < records[0][59]  # outliers on both terms
    assert np.array_equal(twist, records[-1][6:12])
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(ires.cpu().numpy(), want_ires)
    assert _bits_equal(weights.cpu().numpy(), want_weights)


@pytest.mark.parametrize("kind", ["huber", "tukey"])
def test_infinite_scales_give_the_loss_free_twins(lsf, kind):
    model = _model()
    depth, image = wall_frames()[1]
    pyr, live = _device_pyramids()[:2]
    loss = RR.Loss(kind, np.inf, np.inf)
    for plain, robust in ((_strided(model, depth, 1.0, image, START),
                           _strided(model, depth, 1.0, image, START, loss=loss)),
                          (_pyramid(model, pyr, live, START), _pyramid(model, pyr, live, START, loss=loss))):
        assert np.array_equal(plain[0], robust[0]) and np.array_equal(plain[1][:, :61], robust[1][:, :61])
        assert np.array_equal(robust[1][:, 61], plain[1][:, 56]) and np.array_equal(robust[1][:, 62], plain[1][:, 59])
        assert not robust[1][:, 63].any() and not plain[1][:, 61:].any()
        res = robust[2].cpu().numpy()
        assert _bits_equal(res, plain[2].cpu().numpy())
        assert _bits_equal(robust[3].cpu().numpy(), plain[3].cpu().numpy())
        weights = robust[4].cpu().numpy()
        assert plain[4] is None and np.array_equal(np.isnan(weights), np.isnan(res))
        assert np.all(weights[np.isfinite(res)] == 1.0)


def test_without_the_new_settings_the_run_is_the_plain_one(lsf):
    """photometric_weight=None through the new strided entry point gives lsf_point_sdf_run's twist, records and residual
    image bit for bit, on a scene geometry constrains (tests/fusion_scene.py's spheres), with and without a loss; so does
    PointToSdf3d without the new keywords"""
    from levelsetfusion_python_amd import device_point_sdf
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    from test_point_sdf_host import model as sphere_model
    t, w = sphere_model()
    off = S.offset(48)
    live = S.render(S.true_twist(2))
    depth, code = device_depth(live)
    for loss in (None, RR.Loss("tukey", 0.003)):
        kw = dict(robust=_loss(loss), residuals=True)
        plain = device_point_sdf.point_sdf_run(_dev(t), _dev(w), depth, code, _camera(), off, S.true_twist(1), **kw)
        new = device_point_sdf.point_sdf_run_photometric(_dev(t), _dev(w), depth, code, _camera(), off,
                                                         S.true_twist(1), **kw)
        assert np.array_equal(plain[0], new[0]) and np.array_equal(plain[1], new[1]) and new[3] is None
        assert plain[1][-1][56] > 1000 and not plain[1][:, 55].any()
        assert _bits_equal(plain[2].cpu().numpy(), new[2].cpu().numpy())
        if loss is not None:
            assert _bits_equal(plain[3].cpu().numpy(), new[4].cpu().numpy())
    tracker = lsf.PointToSdf3d(_camera())
    twist = tracker.optimize(live, np.array(t), np.array(w), off, S.true_twist(1), residuals=True)
    plain = device_point_sdf.point_sdf_run(_dev(t), _dev(w), depth, code, _camera(), off, S.true_twist(1),
                                           residuals=True)
    assert np.array_equal(twist, plain[0]) and _bits_equal(tracker.last_residuals.cpu().numpy(),
                                                           plain[2].cpu().numpy())
    assert tracker.last_intensity_residuals is None and tracker.last_pyramid is None


def test_a_one_level_unfiltered_pyramid_is_the_stride_1_run(lsf):
    """a one-level pyramid with radius 0 holds float32(depth * ratio): with a float32 metre image at ratio 1 that is the
    image itself, so the geometry-only pyramid run equals the stride-1 run of lsf_point_sdf_run in every field -- the
    twist, every record and the residual image, bit for bit.  With a uint16 image the pyramid rounds depth * ratio to
    float32 where the strided source keeps the float64 product: the counts and the residual image's NaN pattern are
    compared exactly, the twist to the effect of a float32 rounding of the depth (2^-24 * 0.7 m = 4e-8 m a point;
    1e-6 allows the solve's conditioning)"""
    from levelsetfusion_python_amd import device_point_sdf
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    from test_point_sdf_host import model as sphere_model
    t, w = sphere_model()
    off = S.offset(48)
    frame = S.render(S.true_twist(2))
    for live, ratio, exact in ((frame, 1.0, True), (np.round(frame * 1000).astype(np.uint16), 0.001, False)):
        depth, code = device_depth(live)
        pyr = lsf.rigid_opt.DepthPyramid(levels=1, radius=0).build_device(depth, code, _camera(ratio))
        plain = device_point_sdf.point_sdf_run(_dev(t), _dev(w), depth, code, _camera(ratio), off, S.true_twist(1),
                                               iterations=(6,), strides=(1,), residuals=True)
        got = device_point_sdf.point_sdf_run_pyramid(_dev(t), _dev(w), pyr.buffers[0], 1, frame.shape, _camera(ratio),
                                                     off, S.true_twist(1), iterations=(6,), residuals=True)
        assert plain[1][-1][56] > 1000 and got[3] is None and got[4] is None
        a, b = plain[2].cpu().numpy(), got[2].cpu().numpy()
        if exact:
            assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and _bits_equal(a, b)
        else:
            assert np.array_equal(plain[1][0, 56:59], got[1][0, 56:59])  # the first iteration's counts
            np.testing.assert_allclose(got[0], plain[0], rtol=0, atol=1e-6)
            assert (np.isnan(a) != np.isnan(b)).sum() <= 0.001 * a.size


def test_point_to_sdf3d_joint_interface(lsf):
    t, w, c, off = _model()
    depth, image = wall_frames()[1]
    tracker = lsf.PointToSdf3d(_camera(), photometric_weight=LAMBDA, robust=_loss(TUKEY))
    twist = tracker.optimize(np.array(depth), np.array(t), np.array(w), off, START, residuals=True,
                             colour=np.array(c), colour_image=np.array(image))
    records = np.array([np.concatenate([r["delta"].ravel(), r["twist"].ravel()]) for r in tracker.last_records])
    entered = START if len(records) < 2 else records[-2][6:12]
    want, want_res, want_ires, want_weights, after = PC.iteration(
        t, w, PC.strided_source(depth, S.K, 1.0, 1, image), entered, off, colour=c, lam=LAMBDA, loss=TUKEY)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)
    last = tracker.last_records[-1]
    assert (last["count"], last["photometric_count"], last["outliers"]) == \
        (want["count"], want["photometric_count"], want["outliers"])
    assert len(tracker.last_records) == 14 and _bits_equal(tracker.last_residuals.cpu().numpy(), want_res)
    assert _bits_equal(tracker.last_intensity_residuals.cpu().numpy(), want_ires)
    assert _bits_equal(tracker.last_weights.cpu().numpy(), want_weights)
    with pytest.raises(ValueError, match="colour and colour_image"):
        tracker.optimize(np.array(depth), np.array(t), np.array(w), off, START)


def _sequence(lsf, tracker):
    seq = lsf.SequenceFusion3d(_camera(), N, S.offset(N), colour=True, colour_band=COLOUR_BAND,
                               tracking_reference="sdf", sdf_tracker=tracker)
    for depth, image in wall_frames():
        rec = seq.integrate(np.array(depth), np.array(image))
    return seq, rec


@pytest.mark.parametrize("kind", ["strided", "pyramid"])
def test_joint_sdf_sequence_holds_the_wall(lsf, kind, capsys):
    """SequenceFusion3d(colour=True, tracking_reference="sdf") with a joint tracker on the three wall frames at 64^3
    stays within twice the restated sequences' errors"""
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid
    extra = dict(pyramid=DepthPyramid(), intensity_pyramid=IntensityPyramid()) if kind == "pyramid" else {}
    tracker = lsf.PointToSdf3d(_camera(), photometric_weight=LAMBDA, **extra)
    seq, rec = _sequence(lsf, tracker)
    assert len(rec["rigid_records"]) == 14 and rec["prediction_hits"] is None
    assert all(r["skipped"] == 0 and 2 * r["photometric_count"] > r["count"] > 1000 for r in rec["rigid_records"])
    assert (tracker.last_pyramid is not None) == (kind == "pyramid")
    err = twist_errors(seq.twists)
    with capsys.disabled():
        print("\njoint \"sdf\" tracking (%s), |twist - truth| per frame (m, rad):\n" % kind,
              np.array2string(err, precision=8))
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R, err


def test_the_default_sdf_tracker_drifts_on_the_wall(lsf):
    """the same frames through the default sdf_tracker: frame 1 skips every iteration and frame 2 ends outside the joint
    sequences' bound in the plane"""
    seq, _ = _sequence(lsf, None)
    assert all(r["skipped"] == 1 for r in seq.frame_records[1]["rigid_records"])
    err = twist_errors(seq.twists)
    assert max(err[2, 0], err[2, 1]) > SEQUENCE_ATOL_T and err[2, 5] > SEQUENCE_ATOL_R, err
