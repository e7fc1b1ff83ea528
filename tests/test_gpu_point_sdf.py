"""GPU checks of point-to-SDF tracking (csrc/lsf_point_sdf.hip, rigid_opt.PointToSdf3d) against the numpy restatement
(tests/point_sdf_restatement.py), and of SequenceFusion3d(tracking_reference="sdf") against the restated sequence.  The
tolerances are tests/test_gpu_icp.py's: per-pixel values (the residual image, the weight image, the counts) bit for bit;
A, b, the energy and the weight sum, which the device reduces in a tree, to 1e-12 of the sum of their terms' magnitudes;
twists to 1e-9."""
import numpy as np
import pytest
import torch

import fusion_restatement as F
import fusion_scene as S
import point_sdf_restatement as P
import robust_icp_restatement as RR
from test_gpu_icp import NON_CUBIC, SUM_RTOL, TWIST_ATOL, _bits_equal, _camera, _live
from test_icp_host import SEQUENCE_ATOL_R, SEQUENCE_ATOL_T
from test_point_sdf_host import model, restated_sequence

pytestmark = pytest.mark.gpu

PERTURBED = np.array([0.002, -0.001, 0.0015, 0.004, -0.003, 0.002])
TUKEY = RR.Loss("tukey", 0.003)


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _model(volume):
    if volume == "48":
        return model() + (S.offset(48),)
    shape, off = NON_CUBIC
    return model(shape, tuple(off)) + (off,)


def _loss(loss):
    from levelsetfusion_python_amd.rigid_opt import RobustLoss
    return None if loss is None else RobustLoss(loss.kind, loss.scale)


def _run(t, w, live, ratio, off, twist, iterations=P.ITERATIONS, strides=P.STRIDES, loss=None, residuals=False,
         camera=None, **kw):
    from levelsetfusion_python_amd import device_point_sdf
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    depth, code = device_depth(live)
    return device_point_sdf.point_sdf_run(torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(np.array(w)).cuda(),
                                          depth, code, _camera(ratio) if camera is None else camera, off, twist,
                                          iterations=iterations, strides=strides, robust=_loss(loss),
                                          residuals=residuals, **kw)


def _check_record(got, want, robust=False):
    from levelsetfusion_python_amd import device_icp
    r = device_icp.unpack_record(got)
    assert r["count"] == want["count"] and r["skipped"] == want["skipped"]
    assert r["angle_rejected"] == want["no_sample"]  # slot 58: the pixels with a depth and no valid sample
    assert np.all(np.abs(r["matrix_a"] - want["A"]) <= SUM_RTOL * want["A_abs"])
    assert np.all(np.abs(r["vector_b"].ravel() - want["b"]) <= SUM_RTOL * want["b_abs"])
    np.testing.assert_allclose(r["energy"], want["energy"], rtol=SUM_RTOL)
    np.testing.assert_allclose(r["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
    assert r["photometric_count"] == 0 and r["photometric_energy"] == 0.0 and r["photometric_weight_sum"] == 0.0
    if robust:
        np.testing.assert_allclose(r["weight_sum"], want["weight_sum"], rtol=SUM_RTOL)
        assert r["outliers"] == want["outliers"]
    else:
        assert r["weight_sum"] == 0.0 and r["outliers"] == 0
    return r


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_one_iteration_against_restatement(lsf, stride):
    """640 x 480 has 1200 tiles at stride 1, against 256 workgroups: the grid-stride loop's later trips; 640 / 3 is
    ragged.  Residuals bit for bit (NaN where a pixel has no pair, or is off the stride), the counts exactly"""
    t, w, off = _model("48")
    live, ratio = _live(np.float32)
    start = S.true_twist(1) + PERTURBED
    twist, records, res, weights = _run(t, w, live, ratio, off, start, (1,), (stride,), residuals=True)
    want, want_res, _, after = P.iteration(t, w, live, S.K, ratio, start, off, stride)
    r = _check_record(records[0], want)
    assert r["level"] == 0 and r["count"] > 1000 and r["angle_rejected"] > 0 and weights is None
    assert _bits_equal(res.cpu().numpy(), want_res)
    np.testing.assert_allclose(twist, after, rtol=0, atol=TWIST_ATOL)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("volume", ["48", "non-cubic"])
def test_whole_run_against_restatement(lsf, volume, dtype):
    t, w, off = _model(volume)
    live, ratio = _live(dtype)
    twist, records, _, _ = _run(t, w, live, ratio, off, S.true_twist(1))
    want, want_twist, _, _ = P.track(t, w, live, S.K, ratio, S.true_twist(1), off)
    assert len(records) == len(want) == 14
    for got, rec in zip(records, want):
        assert _check_record(got, rec)["level"] == rec["level"]
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert np.array_equal(twist, records[-1][6:12])
    assert np.abs(twist - S.true_twist(2)).max() < 2e-3


def test_a_model_with_a_hole(lsf):
    """weight 0 in a block of voxels across the front of the central sphere: NaN exactly where the restatement has NaN"""
    t, w, off = _model("48")
    holed = np.array(w)
    holed[10:18, 20:28, 20:28] = 0.0
    live, ratio = _live(np.float32)
    start = S.true_twist(1) + PERTURBED
    _, records, res, _ = _run(t, holed, live, ratio, off, start, (1,), (1,), residuals=True)
    want, want_res, _, _ = P.iteration(t, holed, live, S.K, ratio, start, off)
    whole, whole_res, _, _ = P.iteration(t, w, live, S.K, ratio, start, off)
    lost = np.isfinite(whole_res) & np.isnan(want_res)
    assert lost.sum() > 500 and want["no_sample"] > whole["no_sample"]  # the hole takes pairs away
    got = res.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want_res)) and _bits_equal(got, want_res)
    _check_record(records[0], want)


def test_a_point_on_the_last_voxel_plane_has_no_pair(lsf):
    """pixel (cx, cy) at the zero twist has g_x = 0 exactly; with offset_x = -(n_x - 1) it lands on p_x = n_x - 1,
    where the sample has no upper corner.  Its left neighbour lands inside and pairs"""
    n, d, vs = (12, 10, 9), np.float32(0.5), 0.004  # extents z, y, x
    off = np.array([-(n[2] - 1.0), -n[1] / 2.0, float(d) / vs - n[0] / 2.0])
    z, y, x = np.meshgrid(np.arange(float(n[0])), np.arange(float(n[1])), np.arange(float(n[2])), indexing="ij")
    t = (0.001 * (x + 2.0 * y + 3.0 * z)).astype(np.float32)
    w = np.ones_like(t)
    live = np.zeros((242, 322), np.float32)
    live[240, 318:322] = d
    _, records, res, _ = _run(t, w, live, 1.0, off, np.zeros(6), (1,), (1,), residuals=True)
    want, want_res, _, _ = P.iteration(t, w, live, S.K, 1.0, np.zeros(6), off)
    got = res.cpu().numpy()
    assert np.isnan(got[240, 320]) and np.isnan(got[240, 321]) and np.isfinite(got[240, 319])
    assert want["count"] == 2 and want["no_sample"] == 2 and _bits_equal(got, want_res)
    # two pairs leave A without rank, so the solve is not compared: the counts are
    assert records[0][56] == 2 and records[0][58] == 2
    np.testing.assert_allclose(records[0][12], want["energy"], rtol=SUM_RTOL)


def test_reruns_are_bit_identical(lsf):
    t, w, off = _model("48")
    live, ratio = _live(np.uint16)
    a = _run(t, w, live, ratio, off, S.true_twist(1), loss=TUKEY, residuals=True)
    b = _run(t, w, live, ratio, off, S.true_twist(1), loss=TUKEY, residuals=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _bits_equal(a[2].cpu().numpy(), b[2].cpu().numpy()) and _bits_equal(a[3].cpu().numpy(), b[3].cpu().numpy())


@pytest.mark.parametrize("kind", ["huber", "tukey"])
def test_an_infinite_scale_is_the_plain_run(lsf, kind):
    t, w, off = _model("48")
    live, ratio = _live(np.float32)
    plain = _run(t, w, live, ratio, off, S.true_twist(1), residuals=True)
    robust = _run(t, w, live, ratio, off, S.true_twist(1), loss=RR.Loss(kind, np.inf), residuals=True)
    assert np.array_equal(plain[0], robust[0]) and np.array_equal(plain[1][:, :61], robust[1][:, :61])
    assert np.array_equal(robust[1][:, 61], plain[1][:, 56]) and not robust[1][:, 62:].any()
    res = robust[2].cpu().numpy()
    assert _bits_equal(res, plain[2].cpu().numpy()) and plain[3] is None
    weights = robust[3].cpu().numpy()
    assert np.array_equal(np.isnan(weights), np.isnan(res)) and np.all(weights[np.isfinite(res)] == 1.0)


def test_tukey_against_restatement(lsf):
    t, w, off = _model("48")
    live, ratio = _live(np.float32)
    twist, records, res, weights = _run(t, w, live, ratio, off, S.true_twist(1), loss=TUKEY, residuals=True)
    want, want_twist, want_res, want_weights = P.track(t, w, live, S.K, ratio, S.true_twist(1), off, loss=TUKEY)
    assert len(records) == len(want) == 14 and want[0]["outliers"] > 0 and want[-1]["weight_sum"] > 1000
    for got, rec in zip(records, want):
        assert _check_record(got, rec, robust=True)["level"] == rec["level"]
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert _bits_equal(res.cpu().numpy(), want_res) and _bits_equal(weights.cpu().numpy(), want_weights)


def test_point_to_sdf3d_interface(lsf):
    t, w, off = _model("48")
    live, ratio = _live(np.float64)
    tracker = lsf.PointToSdf3d(_camera(ratio), robust=_loss(TUKEY))
    twist = tracker.optimize(live, np.array(t), np.array(w), off, S.true_twist(1), residuals=True)
    want, want_twist, want_res, want_weights = P.track(t, w, live, S.K, ratio, S.true_twist(1), off, loss=TUKEY)
    assert twist.shape == (6,) and twist.dtype == np.float64
    np.testing.assert_allclose(twist, want_twist, rtol=0, atol=TWIST_ATOL)
    assert [r["count"] for r in tracker.last_records] == [r["count"] for r in want]
    assert [r["outliers"] for r in tracker.last_records] == [r["outliers"] for r in want]
    assert _bits_equal(tracker.last_residuals.cpu().numpy(), want_res)
    assert _bits_equal(tracker.last_weights.cpu().numpy(), want_weights)


def test_an_empty_model_keeps_the_twist(lsf):
    t, w, off = _model("48")
    live, ratio = _live(np.uint16)
    start = S.true_twist(1) + PERTURBED
    twist, records, res, _ = _run(t, np.zeros_like(w), live, ratio, off, start, (2, 1), (3, 1), residuals=True)
    assert np.array_equal(twist, start) and np.isnan(res.cpu().numpy()).all()
    want, _, _, _ = P.iteration(t, np.zeros_like(w), live, S.K, ratio, start, off)
    assert want["count"] == 0 and want["skipped"] == 1
    for got in records:
        assert got[55] == 1 and got[56] == 0 and not got[:6].any() and np.array_equal(got[6:12], start)
    assert records[2][58] == want["no_sample"] > 0 and records[2][57] == 1


def test_sequence_sdf_against_restatement(lsf, capsys):
    """48^3, four frames: each frame's tracking records (counts exact, twists to 1e-9), the model (bit for bit) and the
    fusion records match the restated sequence, within test_icp_host's sequence tolerance of it throughout"""
    n, count = 48, 4
    off = S.offset(n)
    frames = S.frames(count)
    seq = lsf.SequenceFusion3d(_camera(), n, off, tracking_reference="sdf")
    _, _, twists, fusion, sdf = restated_sequence(count, n)
    model_t, model_w = F.empty_model((n,) * 3)
    for k, depth in enumerate(frames):
        rec = seq.integrate(depth)
        assert rec["prediction_hits"] is None and seq.prediction is None
        assert len(rec["rigid_records"]) == len(sdf[k])
        for got, want in zip(rec["rigid_records"], sdf[k]):
            assert got["count"] == want["count"] and got["level"] == want["level"]
            assert got["angle_rejected"] == want["no_sample"]
            np.testing.assert_allclose(got["twist"].ravel(), want["twist"], rtol=0, atol=TWIST_ATOL)
        diff = np.abs(seq.twists[-1] - twists[k])
        assert diff[:3].max() <= SEQUENCE_ATOL_T and diff[3:].max() <= SEQUENCE_ATOL_R, diff
        np.testing.assert_allclose(seq.twists[-1], twists[k], rtol=0, atol=TWIST_ATOL)
        model_t, model_w, want_rec = F.fuse_depth(model_t, model_w, depth, S.K, 1.0, off, seq.twists[-1])
        assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), model_t)
        assert _bits_equal(seq.canonical.weight.cpu().numpy(), model_w)
        assert rec["fusion"]["fused"] == want_rec["fused"] == fusion[k]["fused"]
    err = np.abs(np.array(seq.twists) - np.array([S.true_twist(k) for k in range(count)]))
    with capsys.disabled():
        print("\n\"sdf\" tracking, |twist - truth| per frame (m, rad):\n", np.array2string(err, precision=6))


def test_sdf_sequence_takes_a_tracker_and_combines_with_carving(lsf):
    n = 32
    tracker = lsf.PointToSdf3d(_camera(), iterations=(2, 2), strides=(4, 2), robust=_loss(TUKEY))
    seq = lsf.SequenceFusion3d(_camera(), n, S.offset(n), tracking_reference="sdf", sdf_tracker=tracker, carve=True)
    assert seq.sdf_tracker is tracker
    for k, depth in enumerate(S.frames(2)):
        rec = seq.integrate(depth)
        assert len(rec["rigid_records"]) == (4 if k else 0) and "carved" in rec["fusion"]
    assert rec["rigid_records"][-1]["weight_sum"] > 0 and rec["rigid_records"][-1]["count"] > 1000
    still = lsf.SequenceFusion3d(_camera(), n, S.offset(n), tracking_reference="sdf", initial_twist=S.true_twist(1),
                                 sdf_tracker=lsf.PointToSdf3d(_camera(), iterations=(0,), strides=(1,)))
    for depth in S.frames(2):
        assert still.integrate(depth)["rigid_records"] == []
    assert all(np.array_equal(x, S.true_twist(1)) for x in still.twists)
