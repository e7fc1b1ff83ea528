"""GPU checks of tracking quality and relocalisation: lsf_reloc_encode and lsf_reloc_query (csrc/lsf_relocaliser.hip)
against the numpy restatement (tests/relocaliser_restatement.py) bit for bit -- coarse images, block counts, codes,
distances, nearest, records, the database after an append, and a second run of every call --, and
SequenceFusion3d(tracking_quality=, relocaliser=) over tests/moving_volume_scene.py in the fixed window: a kidnapped
camera (scene A), leaving the window and coming back (scene B), the gate alone, and the gate that nothing violates.
The encode kernel gives a wave to every coarse block and four to a workgroup: 5 x 7 blocks is nine workgroups with a
ragged last one, 37 x 53 over 5 x 7 makes blocks of 7 or 8 rows by 7 or 8 columns (49 to 64 pixels: fewer than a
wave's lanes, and exactly as many), 120 x 160 over 15 x 20 blocks of exactly one wave.  The distance kernel gives a wave
to every keyframe row and reads aligned 16-byte words: F = 70 and 500 put most rows off that alignment, and the last
row's last word reaches past the array unless capacity * F is a multiple of 16.  Every loop here stays in its first
trip; blocks of more pixels than lanes, more blocks or rows than the capped grid has waves, rows of more than 64 words
and more keys than the select kernel has lanes are in tests/test_gpu_second_trip.py, on the inputs of
tests/test_relocaliser_host.py."""
import math

import numpy as np
import pytest
import torch

import moving_volume_scene as MS
import relocaliser_restatement as R
from test_relocaliser_host import (COARSE, DECISIONS, DEPTH_RANGE, FERNS, HARVEST, MAX_RMS, MIN_PAIR_FRACTION, SCENE_A,
                                   SCENE_B, check_recovery, frame, pose_errors)
from test_relocaliser_host import depth_image as _depth_image
from test_relocaliser_host import query_case as _query_case

pytestmark = pytest.mark.gpu

PLAIN_KEYS = {"frame", "twist", "rigid_records", "nonrigid", "fusion", "prediction_hits"}


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- encode ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_colour", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.float64])
@pytest.mark.parametrize("shape, coarse_shape", [((37, 53), (5, 7)), ((120, 160), (15, 20))])
def test_encode_against_restatement(lsf, shape, coarse_shape, dtype, with_colour):
    from levelsetfusion_python_amd import device_relocaliser as D
    rng = np.random.default_rng(shape[0] + np.dtype(dtype).itemsize)
    depth, ratio = _depth_image(shape, coarse_shape, dtype, rng)
    colour = rng.integers(0, 256, shape + (3,)).astype(np.uint8) if with_colour else None
    want, want_counts, want_record = R.encode(depth, ratio, coarse_shape, (0.5, 3.5), colour)
    pixels = [(shape[0] // coarse_shape[0]) * ((j + 1) * shape[1] // coarse_shape[1] - j * shape[1] // coarse_shape[1])
              for j in (0, 1)]
    # the two blocks set by hand: one fewer than half does not count, exactly half does (both shapes make block (0, 1) even)
    assert (want_counts[0, 0] + 1) * 2 in (pixels[0], pixels[0] + 1) and want[0, 0, 0] == 0
    assert want_counts[0, 1] * 2 == pixels[1] and want[0, 1, 0] > 0
    assert 0 < want_record["valid_blocks"] < want_counts.size
    encode_twice_against(D, depth, ratio, coarse_shape, colour, want, want_counts, want_record)


def encode_twice_against(D, depth, ratio, coarse_shape, colour, want, want_counts, want_record):
    """two runs of lsf_reloc_encode over host inputs, each against the restated coarse bits, block counts and record"""
    from levelsetfusion_python_amd.tsdf.generation import device_depth
    d_depth = device_depth(depth)[0]
    d_colour = None if colour is None else _cuda(colour)
    runs = [D.encode(d_depth, coarse_shape, (0.5, 3.5), ratio, d_colour) for _ in range(2)]
    for coarse, counts, record in runs:
        assert np.array_equal(_bits(coarse), want.view(np.uint32))
        assert np.array_equal(counts.cpu().numpy(), want_counts)
        assert D.unpack_encode_record(record.cpu().numpy()) == want_record
    assert coarse.shape == tuple(coarse_shape) + ((1,) if colour is None else (4,))


def test_encode_refusals_on_the_device(lsf):
    from levelsetfusion_python_amd import device_relocaliser as D
    depth = torch.ones((12, 16), dtype=torch.float32, device="cuda")
    D.encode(depth, (3, 4), (0.5, 4.0))
    for bad in (dict(coarse_shape=(13, 4)), dict(coarse_shape=(3, 17)), dict(depth_range=(4.0, 0.5)),
                dict(depth_range=(0.5, 65.0)), dict(depth_unit_ratio=0.0),
                dict(colour=torch.zeros((12, 16), dtype=torch.uint8, device="cuda")),
                dict(coarse=torch.zeros((3, 4, 4), dtype=torch.float32, device="cuda")),
                dict(record=torch.zeros(2, dtype=torch.int64, device="cuda"))):
        kw = dict(coarse_shape=(3, 4), depth_range=(0.5, 4.0))
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            D.encode(depth, **kw)
    with pytest.raises((ValueError, TypeError)):
        D.encode(depth.cpu(), (3, 4), (0.5, 4.0))
    torch.cuda.synchronize()


# ---- query ----------------------------------------------------------------------------------------------------------------

def _run_query(D, coarse, table, rows, n, capacity, **kw):
    codes = np.zeros((capacity, rows.shape[1]), np.uint8)
    codes[:n] = rows[:n]
    want = R.query(coarse, table, codes, n, kw.get("candidates", 1), kw.get("harvest", False),
                   kw.get("harvest_differing", 1))
    for _ in range(2):  # the second run: bit-identical
        d_codes, d_n = _cuda(codes), torch.tensor([n], dtype=torch.int32, device="cuda")
        got = D.query(_cuda(coarse), *(_cuda(a) for a in table), d_codes, d_n, **kw)
        assert np.array_equal(got[0].cpu().numpy(), want[0])
        assert np.array_equal(got[1].cpu().numpy(), want[1])
        assert np.array_equal(got[2].cpu().numpy(), want[2]), (got[2].cpu().numpy(), want[2])
        assert np.array_equal(d_codes.cpu().numpy(), want[3]) and int(d_n.item()) == want[4]
    return want


@pytest.mark.parametrize("decisions", [1, 4, 8])
@pytest.mark.parametrize("ferns", [70, 500])
def test_query_against_restatement(lsf, ferns, decisions):
    from levelsetfusion_python_amd import device_relocaliser as D
    colour = decisions == 4
    assert (ferns * 131) % 16 != 0 and (ferns * 1) % 16 != 0  # rows off the 16-byte alignment, a ragged last word
    query_comparison(D, ferns, decisions, *_query_case(ferns, decisions, colour))


def query_comparison(D, ferns, decisions, coarse, table, rows):
    """lsf_reloc_query against the restatement over the 131 keyframes of a query_case"""
    code = R.frame_code(coarse, *table)
    assert code.max() < (1 << decisions) and code.any()
    # a database of 0, 1, 130 and `capacity` keyframes
    rec = _run_query(D, coarse, table, rows, 0, 131, candidates=4, harvest=True, harvest_differing=3)[2]
    assert rec.tolist() == [0] + [-1] * 8 + [0, 0, 0]  # an empty database takes the frame
    rec = _run_query(D, coarse, table, rows, 1, 131, candidates=4, harvest=True, harvest_differing=1)[2]
    assert rec.tolist() == [1, 0, -1, -1, -1, 0, -1, -1, -1, -1, 0, 0]  # candidates larger than n; distance 0 stays out
    want = _run_query(D, coarse, table, rows, 130, 131, candidates=4)
    assert want[2][9] == -1 and want[2][1] == 0 and (want[1][:130] >= 0).all() and want[1][130] == -1
    want = _run_query(D, coarse, table, rows, 131, 131, candidates=3, harvest=True, harvest_differing=1)
    assert want[2][9] == -1 and want[2][10] == 0  # keyframe 0 is the frame itself: not wanted, so not "full" either
    # without the nearest keyframes the smallest distance is that of keyframe 23 and its copy 57: the tie goes to 23
    far = rows[[k for k in range(131) if (k * 7) % (ferns + 1) >= (23 * 7) % (ferns + 1)]]
    n = len(far)
    want = _run_query(D, coarse, table, far, n, n, candidates=2)
    nearest = int(want[1][:n].min())
    twins = [k for k in range(n) if np.array_equal(far[k], rows[23])]
    assert len(twins) == 2 and want[2][1:3].tolist() == twins and want[2][5:7].tolist() == [nearest, nearest] and nearest > 0
    # harvest at exactly harvest_differing and one below; at exactly it with a full database: refused, flag set
    at = _run_query(D, coarse, table, far, n, n + 1, harvest=True, harvest_differing=nearest)
    assert at[2][9] == n and at[4] == n + 1 and np.array_equal(at[3][n], code)
    below = _run_query(D, coarse, table, far, n, n + 1, harvest=True, harvest_differing=nearest + 1)
    assert below[2][9] == -1 and below[2][10] == 0 and below[4] == n
    full = _run_query(D, coarse, table, far, n, n, harvest=True, harvest_differing=nearest)
    assert full[2][9] == -1 and full[2][10] == 1 and full[4] == n


def test_query_refusals_on_the_device(lsf):
    from levelsetfusion_python_amd import device_relocaliser as D
    coarse, table, rows = _query_case(70, 4, True)
    args = lambda: (_cuda(coarse), *(_cuda(a) for a in table), _cuda(rows), torch.tensor([3], dtype=torch.int32,
                                                                                         device="cuda"))
    D.query(*args())
    for bad in (dict(candidates=0), dict(candidates=5), dict(harvest=True, harvest_differing=0),
                dict(distances=torch.zeros(5, dtype=torch.int32, device="cuda")),
                dict(frame_code=torch.zeros(70, dtype=torch.int32, device="cuda"))):
        with pytest.raises((ValueError, TypeError)):
            D.query(*args(), **bad)
    a = list(args())
    a[1] = a[1][:, :0].contiguous()  # D = 0
    with pytest.raises((ValueError, TypeError)):
        D.query(*a)
    a = list(args())
    a[4] = torch.zeros(131 * 70 + 16, dtype=torch.uint8, device="cuda")[1:1 + 131 * 70].view(131, 70)  # off 16 bytes
    with pytest.raises((ValueError, TypeError)):
        D.query(*a)
    torch.cuda.synchronize()


def test_relocaliser_object(lsf):
    """fusion.Relocaliser over six frames of the pass: its table, codes, keyframes and twists equal the restated
    database's; reset empties it and keeps the table"""
    reloc = lsf.fusion.Relocaliser(FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST, 16, candidates=2, seed=5)
    db = R.Database(FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST, 16, candidates=2, seed=5)
    for k in (0, 2, 4, 6, 8, 3):
        coarse = reloc.encode(frame(k))
        assert np.array_equal(_bits(coarse), db.encode(frame(k), 1.0).view(np.uint32))
        got, want = reloc.query(coarse, harvest=True, twist=MS.true_twist(k)), db.query(db.encode(frame(k), 1.0), True,
                                                                                        MS.true_twist(k))
        assert {n: got[n] for n in want} == want and not got["full"]
    codes, twists = reloc.keyframes()
    assert len(codes) == db.n > 1 and np.array_equal(codes, db.codes[:db.n]) and np.array_equal(twists, db.twists)
    assert all(np.array_equal(a, b) for a, b in zip(reloc.table, db.table))
    with pytest.raises(ValueError):
        reloc.encode(frame(0), colour_image=np.zeros((MS.HEIGHT, MS.WIDTH, 3), np.uint8))  # drawn without colour
    reloc.reset()
    assert reloc.keyframes()[0].shape == (0, FERNS) and reloc.query(reloc.encode(frame(1)))["n"] == 0


# ---- the sequence ----------------------------------------------------------------------------------------------------------

def _camera():
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)


def _sequence(lsf, mode="icp", **kw):
    return lsf.SequenceFusion3d(_camera(), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                                narrow_band_width_voxels=MS.BAND, tracking_reference=mode, **kw)


def _relocaliser(lsf):
    return lsf.fusion.Relocaliser(FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST, max_keyframes=64)


def _run(seq, poses):
    """integrate the scene's frames; the model's weight bits after every frame"""
    weights = []
    for p in poses:
        seq.integrate(frame(p))
        weights.append(seq.canonical.weight.clone())
    return weights


def _unchanged(weights, k):
    return torch.equal(weights[k].view(torch.int32), weights[k - 1].view(torch.int32))


def _gate(lsf):
    return lsf.fusion.TrackingQuality(MIN_PAIR_FRACTION, MAX_RMS)


def test_scene_a_a_kidnapped_camera_is_relocalised(lsf, capsys):
    """true poses 0..12, two all-zero frames, then 3..6 in the fixed 48^3 window, "icp" mode.  With a relocaliser the
    blank frames are lost and leave the model's weight bit-equal, the frame at pose 3 is relocalised to a keyframe, every
    later frame tracks, and every fused frame after the recovery lies within MARGIN_T, MARGIN_R of the sequence's own
    error at the same true pose on its first visit.  Without the keywords the same frames end more than 10 cm away.
    Measured on an MI355X: after the recovery the poses 3..6 are 0.37, 0.36, 0.41, 0.43 mm and 1.98e-3, 2.05e-3,
    1.58e-3, 1.46e-3 rad from the truth, against 0.24, 0.33, 0.37, 0.38 mm and 1.67e-3, 2.88e-3, 2.68e-3, 2.49e-3 rad on
    their first visit: the largest excess is 0.14 mm and 0.31e-3 rad.  Without the keywords the last frame is 0.635 m
    and 1.73 rad off."""
    seq = _sequence(lsf, relocaliser=_relocaliser(lsf), tracking_quality=_gate(lsf))
    weights = _run(seq, SCENE_A)
    records = seq.frame_records
    states = [r["tracking_state"] for r in records]
    errors = pose_errors(SCENE_A, seq.twists)
    with capsys.disabled():
        print("\nscene A states:", states)
        print("scene A |twist - truth| per frame (m, rad):\n", np.array2string(errors, precision=6))
    assert len(seq.twists) == len(SCENE_A)
    assert states[:13] == ["tracking"] * 13 and states[13:15] == ["lost", "lost"]
    for k in (13, 14):
        assert records[k]["fusion"] is None and records[k]["keyframe"] is None and _unchanged(weights, k)
        assert np.array_equal(seq.twists[k], seq.twists[12]) and records[k]["tracking_quality"]["skipped"]
    assert not _unchanged(weights, 12) and not _unchanged(weights, 15)
    assert states[15] == "relocalised" and states[16:] == ["tracking"] * 3
    found = records[15]["relocalisation"]
    assert found["chosen"] is not None and found["chosen"] >= 0 and found["chosen"] in found["candidates"]
    assert records[0]["keyframe"] == 0 and records[0]["tracking_state"] == "tracking"
    assert set(records[0]) == PLAIN_KEYS | {"tracking_state", "tracking_quality", "keyframe", "relocalisation"}
    kept = [r["keyframe"] for r in records if r["keyframe"] is not None]
    assert kept == list(range(len(kept))) and 1 < len(kept) < 13 and len(seq.relocaliser.twists) == len(kept)
    excess = check_recovery(SCENE_A, states, [r["fusion"] is not None for r in records], errors)
    plain = _sequence(lsf)
    _run(plain, SCENE_A)
    plain_errors = pose_errors(SCENE_A, plain.twists)
    with capsys.disabled():
        print("scene A largest excess over the first visit: %.6f m %.6f rad; without the keywords the last frame is "
              "%.4f m %.4f rad off" % (excess[0], excess[1], plain_errors[-1][0], plain_errors[-1][1]))
    assert plain_errors[-1][0] > 0.1
    assert all(set(r) == PLAIN_KEYS for r in plain.frame_records)  # without the keywords: no new keys


def test_resume_after_keeps_the_first_good_frames_out_of_the_model(lsf):
    """scene A with resume_after=2 and two candidates: the relocalised frame and the good frame after it are tracked,
    keep their own twists and leave the weight bit-equal; fusion resumes with the frame after them"""
    reloc = lsf.fusion.Relocaliser(FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST, max_keyframes=64, candidates=2,
                                   resume_after=2)
    seq = _sequence(lsf, relocaliser=reloc, tracking_quality=_gate(lsf))
    weights = _run(seq, SCENE_A)
    records = seq.frame_records
    assert [r["tracking_state"] for r in records[13:]] == ["lost", "lost", "relocalised", "recovering", "tracking",
                                                          "tracking"]
    found = records[15]["relocalisation"]
    assert len(found["candidates"]) == 2 and found["distances"] == sorted(found["distances"])
    assert found["chosen"] in found["candidates"] and len(records[13]["relocalisation"]["candidates"]) == 2
    for k in (15, 16):
        assert records[k]["fusion"] is None and records[k]["keyframe"] is None and _unchanged(weights, k)
        assert not np.array_equal(seq.twists[k], seq.twists[k - 1])  # a good frame's own twist is kept
    assert not _unchanged(weights, 17) and records[17]["fusion"]["fused"] > 0
    check_recovery(SCENE_A, [r["tracking_state"] for r in records], [r["fusion"] is not None for r in records],
                   pose_errors(SCENE_A, seq.twists))


def test_scene_b_out_of_the_window_and_back(lsf, capsys):
    """true poses 0..28 then 27..10 in the fixed window.  The lost frames form one contiguous run that holds every frame
    whose true pose index is 24 or more, none of them changes the weight, the run ends with a relocalised frame, the last
    frame tracks, and the fused frames after the recovery lie within the margins of their pose's first visit.  Where the
    track is lost is not pinned: the pair fraction passes the gate of 0.25 between 0.262 and 0.246.
    Measured on an MI355X: frames 22..34 are lost (true poses 22..28..22), frame 35 (pose 21) is relocalised to keyframe
    10; the fused frames after it are at most 0.72 mm and 3.9e-3 rad from the truth (pose 20: 0.72 mm, 3.90e-3 rad against
    0.60 mm, 2.24e-3 rad on its first visit), and the largest excess over a first visit is 0.12 mm and 1.66e-3 rad."""
    seq = _sequence(lsf, relocaliser=_relocaliser(lsf), tracking_quality=_gate(lsf))
    weights = _run(seq, SCENE_B)
    records = seq.frame_records
    states = [r["tracking_state"] for r in records]
    errors = pose_errors(SCENE_B, seq.twists)
    with capsys.disabled():
        print("\nscene B states:", states)
        print("scene B |twist - truth| per frame (m, rad):\n", np.array2string(errors, precision=6))
    lost = [k for k, s in enumerate(states) if s == "lost"]
    assert lost and lost == list(range(lost[0], lost[-1] + 1))
    assert {k for k, p in enumerate(SCENE_B) if p >= 24} <= set(lost)
    assert all(_unchanged(weights, k) and records[k]["fusion"] is None for k in lost)
    assert all(np.array_equal(seq.twists[k], seq.twists[lost[0] - 1]) for k in lost)
    assert states[lost[-1] + 1] == "relocalised" and states[-1] == "tracking"
    assert set(states) == {"tracking", "lost", "relocalised"}
    excess = check_recovery(SCENE_B, states, [r["fusion"] is not None for r in records], errors)
    with capsys.disabled():
        print("scene B largest excess over the first visit: %.6f m %.6f rad" % (excess[0], excess[1]))


def test_quality_alone_freezes_the_model(lsf):
    """the 45-frame pass in the fixed window with tracking_quality only: from the first lost frame on every frame is
    lost, the weight stays bit-equal to its value after the last good frame, and so does the stored twist"""
    seq = _sequence(lsf, tracking_quality=_gate(lsf))
    weights = _run(seq, tuple(range(MS.FRAMES)))
    records = seq.frame_records
    states = [r["tracking_state"] for r in records]
    first = states.index("lost")
    assert 15 < first < 25 and states == ["tracking"] * first + ["lost"] * (MS.FRAMES - first)
    assert all(torch.equal(w.view(torch.int32), weights[first - 1].view(torch.int32)) for w in weights[first:])
    assert all(np.array_equal(t, seq.twists[first - 1]) for t in seq.twists[first:]) and len(seq.twists) == MS.FRAMES
    assert all(r["fusion"] is None for r in records[first:]) and all(r["fusion"] for r in records[:first])
    assert set(records[-1]) == PLAIN_KEYS | {"tracking_state", "tracking_quality"}
    q = records[first]["tracking_quality"]
    assert q["skipped"] or q["pair_fraction"] < MIN_PAIR_FRACTION or q["rms"] > MAX_RMS
    assert MIN_PAIR_FRACTION <= records[first - 1]["tracking_quality"]["pair_fraction"] < 0.3


@pytest.mark.parametrize("mode", ["icp", "sdf"])
def test_a_gate_that_nothing_violates_changes_nothing(lsf, mode):
    poses = tuple(range(8))
    plain, gated = _sequence(lsf, mode), _sequence(lsf, mode, tracking_quality=lsf.fusion.TrackingQuality(0.0))
    _run(plain, poses)
    _run(gated, poses)
    assert all(np.array_equal(a, b) for a, b in zip(plain.twists, gated.twists)) and len(gated.twists) == 8
    for name in ("tsdf", "weight"):
        assert torch.equal(getattr(plain.canonical, name).view(torch.int32),
                           getattr(gated.canonical, name).view(torch.int32))
    assert [r["tracking_state"] for r in gated.frame_records] == ["tracking"] * 8
    assert all(set(r) == PLAIN_KEYS for r in plain.frame_records)
    for a, b in zip(plain.frame_records, gated.frame_records):
        assert a["fusion"] == b["fusion"] and a["prediction_hits"] == b["prediction_hits"]
        assert b["tracking_quality"] is None or 0 < b["tracking_quality"]["pair_fraction"] <= 1
    assert math.isfinite(gated.frame_records[-1]["tracking_quality"]["rms"])
