"""GPU checks of robust ICP (RobustSource in csrc/lsf_icp.hip; device_icp.icp_run_robust and icp_run_pyramid_robust;
ProjectiveIcp3d(robust=), SequenceFusion3d(icp_robust=)) against the numpy restatement
(tests/robust_icp_restatement.py), on the four configurations: strided and gated pyramid on tests/moving_part_scene.py,
photometric and pyramid photometric on tests/textured_wall_scene.py at the same 160 x 120.  With infinite scales the
robust entry points must equal the plain ones bit for bit.  The tolerances are tests/test_gpu_icp.py's: per-pixel images
(residuals, intensity residuals, weights), counts and outliers bit for bit; A, b, the energies and the weight sums to
1e-12 of the sum of their terms' magnitudes; twists to 1e-9.  The depth pyramid's level 0 may differ from numpy's in the
last bit of the filter's exp, so the pyramid restatements start from the device's own level 0."""
import functools
import math

import numpy as np
import pytest
import torch

import depth_pyramid_restatement as DP
import fusion_restatement as F
import fusion_scene as S
import icp_restatement as I
import moving_part_scene as M
import pyramid_photometric_restatement as PP
import robust_icp_restatement as RR
import textured_wall_scene as W
from test_gpu_icp import SUM_RTOL, TWIST_ATOL

pytestmark = pytest.mark.gpu

CONFIGURATIONS = ("strided", "pyramid", "photometric", "pyramid photometric")
ZERO = np.zeros(6)
START = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015])
LEVELS, ITERATIONS, STRIDES = 3, M.ITERATIONS, M.STRIDES
GATE_ANGLE = math.radians(20.0)
LAMBDA = 0.1
# finite scales: the scene's for r; for r_I (units of Y; the wall's |r_I| is about 0.1 at the start) values that leave
# inliers and outliers both
LOSSES = {"huber": RR.Loss("huber", M.HUBER_SCALE, 0.05), "tukey": RR.Loss("tukey", M.TUKEY_SCALE, 0.2)}


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


def _host(t):
    return None if t is None else t.cpu().numpy()


def _device_loss(loss):
    from levelsetfusion_python_amd.rigid_opt import RobustLoss
    return RobustLoss(loss.kind, loss.scale, loss.intensity_scale)


class Case:
    """one configuration on one scene: the device inputs, the plain and the robust device run, and the restated
    iteration of schedule entry k.  Prediction at the zero twist"""

    def __init__(self, lsf, name, K=M.K, shape=M.SHAPE, levels=LEVELS, gate=True):
        self.name, self.K, self.shape, self.levels = name, K, shape, levels
        self.pyramid, self.photo = name.startswith("pyramid"), name.endswith("photometric")
        self.angle = GATE_ANGLE if (self.pyramid and gate) else None
        self.cos = None if self.angle is None else DP.cos_of(self.angle)
        self.lam = LAMBDA if self.photo else None
        if self.photo:
            self.pd, self.pn, self.pc = W.prediction(ZERO, K, shape)
            self.depth, self.image, _ = W.render(W.MOTION, K, shape)
        else:
            width, height = shape[1], shape[0]
            self.pd = M.render(ZERO, False, width, height, K)
            self.pn = DP.normals(self.pd, (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])))
            self.depth = M.render(M.TRUE_TWIST, True, width, height, K)
            self.pc = self.image = None
        self.camera = _camera(K)
        self.d_pd, self.d_pn = _dev(self.pd), _dev(self.pn)
        self.d_pc = _dev(self.pc) if self.photo else None
        self.d_image = _dev(self.image) if self.photo else None
        from levelsetfusion_python_amd.tsdf.generation import device_depth
        self.d_depth, self.code = device_depth(np.array(self.depth))
        self.live = self.pred = None
        if self.pyramid:
            self.pyr = lsf.rigid_opt.DepthPyramid(levels=levels).build(np.array(self.depth), self.camera)
            self.lv = DP.pyramid_from_level0(self.pyr.depth[0].cpu().numpy(), K, levels)
            if self.photo:
                ip = lsf.rigid_opt.IntensityPyramid(levels)
                self.live, self.pred = ip.build_device(self.d_image), ip.build_prediction(self.d_pc)
                self.il, self.ip = PP.live_pyramid(self.image, levels), PP.prediction_pyramid(self.pc, levels)

    def schedule(self, iterations, strides):
        return dict(iterations=iterations) if self.pyramid else dict(iterations=iterations, strides=strides)

    def plain(self, twist, iterations=ITERATIONS, strides=STRIDES):
        """the existing entry point: (twist, records, residuals, intensity residuals or None)"""
        from levelsetfusion_python_amd import device_icp as D
        kw = dict(self.schedule(iterations, strides), residuals=True)
        if self.pyramid and self.photo:
            out = D.icp_run_pyramid_photometric(*self.pyr.buffers, self.live.buffer, self.levels, self.d_pd, self.d_pn,
                                                self.pred.buffer, self.camera, ZERO, self.lam, twist,
                                                max_normal_angle=self.angle, **kw)
        elif self.pyramid:
            out = D.icp_run_pyramid(*self.pyr.buffers, self.levels, self.d_pd, self.d_pn, self.camera, ZERO, twist,
                                    max_normal_angle=self.angle, **kw)
        elif self.photo:
            out = D.icp_run_photometric(self.d_depth, self.code, self.d_image, self.d_pd, self.d_pn, self.d_pc,
                                        self.camera, ZERO, self.lam, twist, **kw)
        else:
            out = D.icp_run(self.d_depth, self.code, self.d_pd, self.d_pn, self.camera, ZERO, twist, **kw)
        return (out + (None,))[:4]

    def robust(self, loss, twist, iterations=ITERATIONS, strides=STRIDES, residuals=True):
        """the robust entry point: (twist, records, residuals, intensity residuals or None, weights)"""
        from levelsetfusion_python_amd import device_icp as D
        kw = dict(self.schedule(iterations, strides), residuals=residuals, photometric_weight=self.lam)
        if self.pyramid:
            return D.icp_run_pyramid_robust(*self.pyr.buffers, self.levels, self.d_pd, self.d_pn, self.camera, ZERO,
                                            _device_loss(loss), twist, max_normal_angle=self.angle,
                                            pyramid_intensity=self.live and self.live.buffer,
                                            pred_intensity=self.pred and self.pred.buffer, **kw)
        return D.icp_run_robust(self.d_depth, self.code, self.d_pd, self.d_pn, self.camera, ZERO, _device_loss(loss),
                                twist, live_colour=self.d_image, pred_colour=self.d_pc, **kw)

    def restated(self, loss, twist, k, iterations=ITERATIONS, strides=STRIDES):
        """the restated iteration of schedule entry k at twist: (record, residuals, intensity residuals or None,
        weights, next twist)"""
        if self.pyramid:
            l = len(iterations) - 1 - k
            d, n, intr = self.lv[0][l], self.lv[1][l], self.lv[2][l]
            if self.photo:
                return RR.pyramid_photometric_iteration(loss, d, n, self.il[l], self.ip[l], intr, self.pd, self.pn,
                                                        self.K, twist, ZERO, self.lam, cos_max=self.cos)
            rec, res, weights, after = RR.iteration(loss, d, self.pd, self.pn, self.K, 1.0, twist, ZERO, 1,
                                                    I.MAX_DISTANCE, intr, n, self.cos)
        elif self.photo:
            return RR.photometric_iteration(loss, self.depth, self.image, self.pd, self.pn, self.pc, self.K, 1.0,
                                            twist, ZERO, self.lam, strides[k])
        else:
            rec, res, weights, after = RR.iteration(loss, self.depth, self.pd, self.pn, self.K, 1.0, twist, ZERO,
                                                    strides[k])
        return rec, res, None, weights, after

    def restated_run(self, loss, twist=None, iterations=ITERATIONS, strides=STRIDES):
        """the independent restated run: the records"""
        twist, records = np.zeros(6) if twist is None else np.array(twist, np.float64), []
        for k, count in enumerate(iterations):
            for _ in range(count):
                rec, _, _, _, twist = self.restated(loss, twist, k, iterations, strides)
                rec["level"] = k
                records.append(rec)
        return records


@functools.lru_cache(maxsize=None)
def _case(lsf, name):
    return Case(lsf, name)


def _check_record(got, want, photo):
    """a device record against a restated one: counts and outliers exactly, sums to SUM_RTOL of their terms'
    magnitudes, the twist to TWIST_ATOL"""
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert (r["count"], r["outliers"], r["skipped"], r["angle_rejected"]) == \
        (want["count"], want["outliers"], want["skipped"], want["angle_rejected"])
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["weight_sum"], want["weight_sum"], rtol=SUM_RTOL)
    if photo:
        assert r["photometric_count"] == want["photometric_count"]
        np.testing.assert_allclose(r["photometric_energy"], want["photometric_energy"], rtol=SUM_RTOL)
        np.testing.assert_allclose(r["photometric_weight_sum"], want["photometric_weight_sum"], rtol=SUM_RTOL)
    else:
        assert (r["photometric_count"], r["photometric_energy"], r["photometric_weight_sum"]) == (0, 0.0, 0.0)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    return r


def _check_images(got, want, photo):
    """(residuals, intensity residuals, weights) bit for bit; the weights are finite exactly where the residuals are"""
    res, ires, weights = (_host(t) for t in got)
    assert _bits_equal(res, want[0]) and _bits_equal(weights, want[2])
    assert np.array_equal(np.isfinite(weights), np.isfinite(res))
    if photo:
        assert _bits_equal(ires, want[1])
    else:
        assert ires is None and want[1] is None


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("name", CONFIGURATIONS)
def test_infinite_scales_are_the_plain_entry_points(lsf, name, kind):
    """twist, record slots 0 .. 60 and both residual images bit for bit; every weight is 1, nothing is an outlier"""
    c = _case(lsf, name)
    twist, records, res, ires = c.plain(None)
    got_twist, got, got_res, got_ires, weights = c.robust(RR.Loss(kind, np.inf, np.inf), None)
    assert len(records) == 14 and np.array_equal(got_twist, twist)
    assert np.array_equal(got[:, :61], records[:, :61])
    assert np.array_equal(got[:, 61], records[:, 56]) and np.all(got[:, 63] == 0) and np.all(records[:, 61:] == 0)
    assert np.array_equal(got[:, 62], records[:, 59])  # the photometric pairs, 0 without the term
    assert np.all(records[:, 56] > 1000) and np.all(records[:, 55] == 0)
    res, got_res = _host(res), _host(got_res)
    assert _bits_equal(got_res, res)
    weights = _host(weights)
    assert np.array_equal(weights[np.isfinite(res)], np.ones(int(np.isfinite(res).sum()), np.float32))
    assert np.isnan(weights[~np.isfinite(res)]).all()
    if c.photo:
        assert _bits_equal(_host(got_ires), _host(ires)) and np.all(records[:, 59] > 1000)
    else:
        assert got_ires is None


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("entry", [0, 2])
@pytest.mark.parametrize("name", CONFIGURATIONS)
def test_one_iteration_against_restatement(lsf, name, entry, kind):
    """one iteration of the coarsest and of the finest schedule entry (stride 4 and 1; pyramid level 2 and 0) from a
    start off the prediction's twist: the three images, the counts and the outliers bit for bit"""
    c, loss = _case(lsf, name), LOSSES[kind]
    iterations = tuple(1 if k == entry else 0 for k in range(3))
    twist, records, res, ires, weights = c.robust(loss, START, iterations)
    want, want_res, want_ires, want_weights, after = c.restated(loss, START, entry)
    r = _check_record(records[0], want, c.photo)
    assert r["level"] == entry and r["count"] > 500 and 0 < r["outliers"] < r["count"]
    assert 0 < r["weight_sum"] < r["count"]
    if c.photo:
        assert 0 < r["photometric_weight_sum"] < r["photometric_count"]
    _check_images((res, ires, weights), (want_res, want_ires, want_weights), c.photo)
    w = _host(weights)
    assert np.nanmin(w) < 0.5 and np.nanmax(w) == 1.0 if kind == "huber" else np.nanmin(w) == 0.0
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("name", CONFIGURATIONS)
def test_whole_run_against_restatement(lsf, name, kind):
    """iterations (4, 4, 6).  Every record is held to the independent restated run in its counts, outliers, level,
    skipped flag and twist, and its sums to the restated iteration taken at the twist the device itself entered the
    iteration with (the method of tests/test_gpu_photometric.py); the last iteration's images bit for bit against
    that iteration"""
    from levelsetfusion_python_amd import device_icp
    c, loss = _case(lsf, name), LOSSES[kind]
    twist, records, res, ires, weights = c.robust(loss, None)
    want = c.restated_run(loss)
    assert len(records) == len(want) == 14
    entered = np.zeros(6)
    for got, w in zip(records, want):
        r = device_icp.unpack_record(got)
        assert (r["count"], r["outliers"], r["angle_rejected"], r["skipped"], r["level"]) == \
            (w["count"], w["outliers"], w["angle_rejected"], w["skipped"], w["level"])
        np.testing.assert_allclose(r["twist"].ravel(), w["twist"], rtol=0, atol=TWIST_ATOL)
        own = c.restated(loss, entered, w["level"])
        _check_record(got, own[0], c.photo)
        entered = got[6:12].copy()
    _check_images((res, ires, weights), own[1:4], c.photo)
    np.testing.assert_allclose(twist, want[-1]["twist"], rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert all(w["skipped"] == 0 for w in want) and want[0]["outliers"] > 0


def _small_case(lsf, name, shape, f, levels=LEVELS, gate=True):
    K = np.array([[f, 0, (shape[1] - 1) / 2.0], [0, f, (shape[0] - 1) / 2.0], [0, 0, 1]], dtype=np.float32)
    return Case(lsf, name, K, shape, levels, gate)


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", ["strided", "photometric"])
def test_ragged_image(lsf, name, stride, kind):
    """37 x 29: not a multiple of 16, one partial tile per edge; stride 3 also clips the NaN cells of the three images
    at the right and the bottom edge"""
    c, loss = _small_case(lsf, name, (29, 37), 40.0), LOSSES[kind]
    _, records, res, ires, weights = c.robust(loss, START, (1,), (stride,))
    want = c.restated(loss, START, 0, (1,), (stride,))
    r = _check_record(records[0], want[0], c.photo)
    assert r["count"] > (400 if stride == 1 else 40)
    _check_images((res, ires, weights), want[1:4], c.photo)


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("name", ["strided", "pyramid photometric"])
def test_second_trip_of_the_capped_grid(lsf, name, kind):
    """272 x 256 at stride 1 (one pyramid level): 272 tiles against LSF_ICP_MAX_BLOCKS = 256 workgroups, so the first
    16 take a second tile"""
    from levelsetfusion_python_amd import _lib
    shape = (256, 272)
    assert ((shape[0] + 15) // 16) * ((shape[1] + 15) // 16) == 272 > _lib.ICP_MAX_BLOCKS
    c, loss = _small_case(lsf, name, shape, 300.0, 1), LOSSES[kind]
    _, records, res, ires, weights = c.robust(loss, START, (1,), (1,))
    want = c.restated(loss, START, 0, (1,), (1,))
    r = _check_record(records[0], want[0], c.photo)
    assert r["count"] > 40000 and r["outliers"] > 0
    _check_images((res, ires, weights), want[1:4], c.photo)
    assert np.isfinite(_host(res)[:, 256:]).sum() > 1000  # the second trip's tiles hold pairs


@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("gate", [False, True])
def test_coarsest_level_of_one_partial_tile(lsf, gate, kind):
    """a three-level pyramid of 37 x 29: level 2 is 9 x 7, a single partial tile, and level 1 (18 x 14) ragged.  On the
    wall, with the intensity term: the spheres' 9 x 7 level leaves the geometric A singular to rounding, and a step of
    such a solve cannot be compared to 1e-9.  Both instantiations of the gate"""
    c, loss = _small_case(lsf, "pyramid photometric", (29, 37), 40.0, gate=gate), LOSSES[kind]
    _, records, res, ires, weights = c.robust(loss, START, (1, 1, 0))
    first = c.restated(loss, START, 0, (1, 1, 0))
    assert tuple(first[1].shape) == (7, 9)
    _check_record(records[0], first[0], c.photo)
    want = c.restated(loss, records[0][6:12].copy(), 1, (1, 1, 0))
    r = _check_record(records[1], want[0], c.photo)
    assert tuple(res.shape) == (14, 18) and r["level"] == 1 and r["count"] > 50
    _check_images((res, ires, weights), want[1:4], c.photo)


def test_reruns_are_bit_identical(lsf):
    c = _case(lsf, "pyramid photometric")
    a, b = (c.robust(LOSSES["tukey"], None) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    for x, y in zip(a[2:], b[2:]):
        assert _bits_equal(_host(x), _host(y))


@pytest.mark.parametrize("name", ["strided", "pyramid"])
def test_tukey_with_every_weight_zero_skips_the_update(lsf, name):
    """a scale below every residual: A = 0, the solve is singular, the twist stays; nothing is NaN"""
    from levelsetfusion_python_amd import device_icp
    c = _case(lsf, name)
    twist, records, res, _, weights = c.robust(RR.Loss("tukey", 1e-12), START)
    assert np.array_equal(twist, START) and np.isfinite(records).all() and len(records) == 14
    for got in records:
        r = device_icp.unpack_record(got)
        assert r["skipped"] == 1 and r["count"] > 500 and r["weight_sum"] == 0.0 and r["energy"] == 0.0
        assert r["outliers"] >= r["count"] - 1  # a residual of exactly 0 would be the one inlier
        assert np.array_equal(r["twist"].ravel(), START) and not r["delta"].any() and not r["matrix_a"].any()
    w = _host(weights)
    assert np.array_equal(np.isfinite(w), np.isfinite(_host(res))) and np.nanmax(w) == 0.0


def test_projective_icp3d_interface(lsf):
    """the tracker picks the robust entry point in every configuration and keeps the weight image"""
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, ProjectiveIcp3d
    loss = LOSSES["tukey"]
    for name in CONFIGURATIONS:
        c = _case(lsf, name)
        kw = {}
        if c.pyramid:
            kw.update(pyramid=DepthPyramid(levels=LEVELS), max_normal_angle=GATE_ANGLE)
        if c.photo:
            kw.update(photometric_weight=LAMBDA)
            if c.pyramid:
                kw.update(intensity_pyramid=IntensityPyramid(LEVELS))
        tracker = ProjectiveIcp3d(c.camera, ITERATIONS, STRIDES, robust=_device_loss(loss), **kw)
        twist = tracker.optimize(np.array(c.depth), c.pd, c.pn, ZERO, residuals=True, colour_image=c.image,
                                 prediction_colour=c.pc)
        want_twist, records, res, ires, weights = c.robust(loss, None)
        assert np.array_equal(twist, want_twist) and len(tracker.last_records) == 14
        assert [r["outliers"] for r in tracker.last_records] == [int(r[63]) for r in records]
        assert tracker.last_records[-1]["weight_sum"] == records[-1][61] > 0
        assert _bits_equal(_host(tracker.last_residuals), _host(res))
        assert _bits_equal(_host(tracker.last_weights), _host(weights))
        assert (tracker.last_intensity_residuals is not None) == c.photo
        tracker.optimize(np.array(c.depth), c.pd, c.pn, ZERO, colour_image=c.image, prediction_colour=c.pc)
        assert tracker.last_residuals is None and tracker.last_weights is None


def test_sequence_with_a_moving_part(lsf, capsys):
    """three frames of the moving-part scene into a 64^3 model with a Tukey loss at 3 mm: the twists and the ICP records
    match the restated sequence, the model the restated fusion at the device's twists, and frame 1's pose is nearer the
    truth than the same sequence's without the loss"""
    from levelsetfusion_python_amd.rigid_opt import RobustLoss
    n, off, frames = 64, S.offset(64), M.sequence_frames(3)
    loss = RR.Loss("tukey", M.TUKEY_SCALE)
    seq = lsf.SequenceFusion3d(_camera(M.K), n, off, tracking_reference="icp",
                               icp_robust=RobustLoss("tukey", M.TUKEY_SCALE))
    plain = lsf.SequenceFusion3d(_camera(M.K), n, off, tracking_reference="icp")
    assert seq.icp_robust.kind == "tukey" and seq.icp.robust is seq.icp_robust and plain.icp_robust is None
    _, _, twists, _, hits, icp = RR.sequence(loss, frames, M.K, 1.0, (n,) * 3, off)
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        plain.integrate(depth)
        assert rec["prediction_hits"] == hits[k] and len(rec["rigid_records"]) == len(icp[k]) == (14 if k else 0)
        for got, want in zip(rec["rigid_records"], icp[k]):
            assert (got["count"], got["outliers"], got["level"], got["skipped"]) == \
                (want["count"], want["outliers"], want["level"], 0)
            np.testing.assert_allclose(got["weight_sum"], want["weight_sum"], rtol=1e-9)
            np.testing.assert_allclose(got["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
        np.testing.assert_allclose(seq.twists[-1], twists[k], rtol=0, atol=TWIST_ATOL)
        model_t, model_w, _ = F.fuse_depth(model_t, model_w, depth, M.K, 1.0, off, seq.twists[-1])
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
    assert rec["rigid_records"][-1]["outliers"] > 100
    robust_error, plain_error = M.pose_error(seq.twists[1], S.true_twist(1)), M.pose_error(plain.twists[1],
                                                                                         S.true_twist(1))
    with capsys.disabled():
        print("\nframe 1 pose error (m, rad): tukey %s, least squares %s" % (robust_error, plain_error))
    assert robust_error[0] < plain_error[0] and robust_error[1] < plain_error[1]
