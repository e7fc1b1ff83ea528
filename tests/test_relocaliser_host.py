"""Host checks of tracking quality and relocalisation (no GPU): properties of the numpy restatement
(tests/relocaliser_restatement.py) on the scene of tests/moving_volume_scene.py -- the fern distance grows along the pass,
a blank frame is far from everything, harvesting keeps a strict subset, and the restated sequence recovers from a
kidnapped camera (scene A) and from leaving the fixed window and coming back (scene B) where the sequence without the
keywords does not --, the refusals of lsf_reloc_encode and lsf_reloc_query that run before any launch, the host rules of
fusion.TrackingQuality and fusion.Relocaliser, and SequenceFusion3d's constructor refusals.  Also the inputs of the GPU
tests, and for those of tests/test_gpu_second_trip.py the assertions that they cross the kernels' caps with a visible
effect past them, from constants and the restatement."""
import ctypes
import functools
import inspect
import math
import os

import numpy as np
import pytest

import moving_volume_scene as MS
import relocaliser_restatement as R

# the scenes' settings: a 256-fern database over a 15 x 20 coarse image of the depths the scene has, and the gate
FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST = 256, 4, (15, 20), (0.48, 0.64), 0.2
MIN_PAIR_FRACTION, MAX_RMS = 0.25, 5e-4
SCENE_A = tuple(range(13)) + (None, None) + (3, 4, 5, 6)   # true pose per frame; None is an all-zero frame
SCENE_B = tuple(range(29)) + tuple(range(27, 9, -1))
MARGIN_T, MARGIN_R = 0.001, 0.002  # test_gpu_volume_shift.py's: a quarter of a voxel and the angle that moves as much


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@functools.lru_cache(maxsize=None)
def frame(pose):
    return np.zeros((MS.HEIGHT, MS.WIDTH), np.float32) if pose is None else MS.render(MS.true_twist(pose))


def database(**kw):
    return R.Database(FERNS, DECISIONS, COARSE, DEPTH_RANGE, HARVEST, 64, **kw)


@functools.lru_cache(maxsize=None)
def restated(scene, keywords):
    """the restated sequence over a scene's frames in the fixed window: (twists, frame dicts, weight)"""
    poses = {"A": SCENE_A, "B": SCENE_B}[scene]
    quality, db = ((MIN_PAIR_FRACTION, MAX_RMS), database()) if keywords else (None, None)
    _, weight, twists, frames = R.sequence([frame(p) for p in poses], MS.K, 1.0, (MS.WINDOW,) * 3, MS.WINDOW_OFFSET,
                                           quality, db, band=MS.BAND, voxel_size=MS.VOXEL)
    return twists, frames, weight


def pose_errors(poses, twists):
    """per frame (|translation error|, |rotation error|) against the true twist; NaN for a blank frame"""
    out = np.full((len(poses), 2), np.nan)
    for k, (p, t) in enumerate(zip(poses, twists)):
        if p is not None:
            e = np.asarray(t) - MS.true_twist(p)
            out[k] = np.linalg.norm(e[:3]), np.linalg.norm(e[3:])
    return out


def check_recovery(poses, states, fused, errors):
    """every fused frame after the relocalisation lies within the margins of the sequence's own error at the same true
    pose on its first visit; returns the largest excess over that error (translation, rotation)"""
    back = states.index("relocalised")
    first = {}
    for k in range(back):
        if poses[k] is not None and fused[k]:
            first.setdefault(poses[k], errors[k])
    excess = np.zeros(2)
    for k in range(back, len(poses)):
        if fused[k]:
            assert poses[k] in first, (k, poses[k])
            excess = np.maximum(excess, errors[k] - first[poses[k]])
            assert errors[k][0] <= first[poses[k]][0] + MARGIN_T and errors[k][1] <= first[poses[k]][1] + MARGIN_R, \
                (k, poses[k], errors[k], first[poses[k]])
    return excess


# ---- the ferns on the scene --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pass_codes(count=16):
    table = R.fern_table(FERNS, DECISIONS, COARSE, DEPTH_RANGE, False, 0)
    return [R.frame_code(R.encode(frame(k), 1.0, COARSE, DEPTH_RANGE)[0], *table) for k in range(count)]


def test_the_distance_from_frame_0_grows_over_the_first_frames():
    codes = pass_codes()
    d = [int((c != codes[0]).sum()) for c in codes]
    # strictly over the first ten frames (6 cm of travel); then it levels off, the spheres 9 cm apart repeating
    assert d[0] == 0 and all(b > a for a, b in zip(d[:10], d[1:10])) and min(d[10:]) >= d[9] > 4 * d[1], d
    assert max(d) < 0.9 * FERNS  # still the same scene: nearer than a blank frame is to anything


def test_a_blank_frame_differs_from_every_frame_in_nearly_all_ferns():
    table = R.fern_table(FERNS, DECISIONS, COARSE, DEPTH_RANGE, False, 0)
    coarse, counts, record = R.encode(frame(None), 1.0, COARSE, DEPTH_RANGE)
    assert not coarse.any() and not counts.any() and record == {"counting": 0, "valid_blocks": 0}
    blank = R.frame_code(coarse, *table)
    assert not blank.any()
    far = [int((c != blank).sum()) for c in pass_codes()]
    # a fern agrees with the blank frame only when all four of its tests fail; the pass's own frames are never as far apart
    assert min(far) >= 0.9 * FERNS, far
    assert min(far) > max(int((c != pass_codes()[0]).sum()) for c in pass_codes())


def test_harvesting_at_a_fifth_keeps_a_strict_subset_of_the_frames():
    db = database()
    kept = [db.query(db.encode(frame(k), 1.0), harvest=True, twist=MS.true_twist(k))["appended"] for k in range(16)]
    ids = [k for k in kept if k is not None]
    assert kept[0] == 0 and ids == list(range(len(ids))) and 1 < len(ids) < 16, kept
    assert db.n == len(ids) == len(db.twists) and R.harvest_differing(HARVEST, FERNS) == 52
    # a frame that is a keyframe already is at distance 0 from it and is not kept again
    again = db.query(db.encode(frame(0), 1.0), harvest=True, twist=MS.true_twist(0))
    assert again == {"nearest": [0], "distances": [0], "appended": None}


def test_query_rules_on_small_tables():
    table = (np.array([[0, 1], [1, 1], [7, 0]], np.int32), np.zeros((3, 2), np.uint8),
             np.array([[0.5, 0.5], [0.5, 2.0], [0.1, 0.1]], np.float32))
    coarse = np.array([[[1.0], [0.75]]], np.float32)  # a 1 x 2 image; location 7 lies outside it
    code = R.frame_code(coarse, *table)
    assert code.tolist() == [3, 1, 2]  # fern 2: the outside test gives 0, location 0 gives bit 1
    assert R.frame_code(np.array([[[0.0], [0.75]]], np.float32), *table).tolist() == [2, 1, 0]  # no depth, no bit
    codes = np.array([[3, 1, 0], [3, 1, 2], [3, 1, 2], [0, 0, 0]], np.uint8)
    _, d, rec, after, n = R.query(coarse, table, codes, 3, candidates=4, harvest=True, differing=1)
    assert d.tolist() == [1, 0, 0, -1] and rec.tolist() == [3, 1, 2, 0, -1, 0, 0, 1, -1, -1, 0, 0]  # the tie: lower id
    assert n == 3 and np.array_equal(after, codes)
    _, d, rec, after, n = R.query(coarse, table, codes, 1, candidates=2, harvest=True, differing=1)
    assert rec.tolist() == [1, 0, -1, -1, -1, 1, -1, -1, -1, 1, 0, 0] and n == 2 and after[1].tolist() == [3, 1, 2]
    _, _, rec, _, n = R.query(coarse, table, codes, 1, harvest=True, differing=2)
    assert rec[9] == -1 and rec[10] == 0 and n == 1  # one below the distance that appends
    _, _, rec, after, n = R.query(coarse, table, codes[:1], 1, harvest=True, differing=1)
    assert rec[9] == -1 and rec[10] == 1 and n == 1 and np.array_equal(after, codes[:1])  # full
    _, d, rec, _, n = R.query(coarse, table, codes, 0, candidates=3, harvest=True, differing=3)
    assert d.tolist() == [-1] * 4 and rec.tolist() == [0] + [-1] * 8 + [0, 0, 0] and n == 1  # an empty database appends


def test_encode_rules_on_a_small_image():
    depth = np.zeros((5, 7), np.float32)
    depth[:2, :3] = [[1.0, 1.5, 0.0], [2.0, 9.0, 0.1]]       # rows [0, 2) x columns [0, 3): three of six count
    depth[2:, 3:] = 1.25
    depth[2, 3:] = 0                                          # rows [2, 5) x columns [3, 7): eight of twelve
    depth[:2, 3:5] = [[1.0, np.nan], [np.inf, 0.0]]           # rows [0, 2) x columns [3, 7): one of eight
    colour = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    coarse, counts, record = R.encode(depth, 1.0, (2, 2), (0.5, 4.0), colour)
    assert counts.tolist() == [[3, 1], [0, 8]] and record == {"counting": 12, "valid_blocks": 2}
    assert coarse[0, 0, 0] == np.float32(1.5) and coarse[1, 1, 0] == np.float32(1.25)
    assert not coarse[0, 1].any() and not coarse[1, 0].any()
    assert coarse[0, 0, 1:].tolist() == [(0 + 3 + 21) / 3.0 + c for c in range(3)]
    assert R.encode(depth, 1.0, (2, 2), (0.5, 4.0))[0].shape == (2, 2, 1)
    depth[0, 0] = 0  # one fewer than half
    assert R.encode(depth, 1.0, (2, 2), (0.5, 4.0))[0][0, 0, 0] == 0
    mm = np.array([[1000, 1001], [0, 65535]], np.uint16)
    assert R.encode(mm, 0.001, (1, 1), (0.5, 4.0))[0][0, 0, 0] == np.float32((1048576 + 1049625) / 2 / 2.0 ** 20)


# ---- the restated sequence ----------------------------------------------------------------------------------------------

def test_the_restated_sequence_recovers_from_a_kidnapped_camera():
    twists, frames, _ = restated("A", True)
    states = [f["state"] for f in frames]
    assert states == ["tracking"] * 13 + ["lost", "lost", "relocalised"] + ["tracking"] * 3
    assert not frames[13]["fused"] and not frames[14]["fused"] and all(f["fused"] for f in frames[15:])
    assert np.array_equal(twists[13], twists[12]) and np.array_equal(twists[14], twists[12])
    assert frames[15]["relocalisation"]["chosen"] in frames[15]["relocalisation"]["candidates"]
    errors = pose_errors(SCENE_A, twists)
    check_recovery(SCENE_A, states, [f["fused"] for f in frames], errors)
    assert errors[-1][0] < 0.001 and errors[-1][1] < 0.004
    plain = pose_errors(SCENE_A, restated("A", False)[0])
    assert plain[-1][0] > 0.1 and plain[-1][0] > 6 * 0.1 and plain[-1][1] > 1.0, plain[-1]  # the contrast: 0.6 m, 1.7 rad


def test_the_restated_sequence_recovers_from_leaving_the_window():
    twists, frames, _ = restated("B", True)
    states = [f["state"] for f in frames]
    lost = [k for k, s in enumerate(states) if s == "lost"]
    assert lost == list(range(lost[0], lost[-1] + 1))  # one contiguous run
    assert set(k for k, p in enumerate(SCENE_B) if p >= 24) <= set(lost)
    assert states[lost[-1] + 1] == "relocalised" and states[-1] == "tracking"
    assert not any(frames[k]["fused"] for k in lost)
    assert all(np.array_equal(twists[k], twists[lost[0] - 1]) for k in lost)
    errors = pose_errors(SCENE_B, twists)
    check_recovery(SCENE_B, states, [f["fused"] for f in frames], errors)
    assert errors[-1][0] < 0.001 and errors[-1][1] < 0.004
    plain = pose_errors(SCENE_B, restated("B", False)[0])
    assert plain[-1][0] > 0.1 and plain[-1][1] > 1.0, plain[-1]


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------

def _host(n, dtype=np.uint8):
    """a 64-byte aligned host buffer: the checks under test return before anything reads it"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 64, np.uint8)
    at = (-raw.ctypes.data) % 64
    return raw[at:at + n * np.dtype(dtype).itemsize].view(dtype)


def test_refusals_through_the_c_abi_that_need_no_device(lsf):
    """every argument is checked on the host side of the C call before any launch, so each of these returns
    LSF_ERR_BAD_ARGUMENT (-1) without a card; the buffers are host memory that no check dereferences"""
    from levelsetfusion_python_amd import device_relocaliser as D
    L = lsf._lib
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    depth, coarse, counts, record = _host(12 * 16, np.float32), _host(3 * 4 * 4, np.float32), _host(12, np.int32), \
        _host(12, np.int32)
    colour = _host(12 * 16 * 3)

    def encode(change=None, **override):
        p = D.encode_params((12, 16), (3, 4), (0.5, 4.0))
        for name, value in (change or {}).items():
            setattr(p, name, value)
        a = dict(depth=ptr(depth), dtype=1, colour=None, coarse=ptr(coarse), counts=ptr(counts), record=ptr(record))
        a.update(override)
        return L.lib.lsf_reloc_encode(a["depth"], a["dtype"], a["colour"], a["coarse"], a["counts"], a["record"],
                                      ctypes.byref(p), None)

    for bad in (dict(coarse_height=13), dict(coarse_width=17), dict(coarse_height=0), dict(depth_near=4.0),
                dict(depth_near=5.0), dict(depth_far=64.5), dict(depth_near=0.0), dict(depth_near=math.nan),
                dict(depth_far=math.inf), dict(depth_unit_ratio=0.0), dict(channels=4), dict(channels=2), dict(height=0)):
        assert encode(bad) == -1, bad
    for bad in (dict(depth=None), dict(coarse=None), dict(counts=None), dict(record=None), dict(dtype=3),
                dict(colour=ptr(colour)),                       # colour with channels 1
                dict(coarse=ptr(depth)),                        # overlap
                dict(coarse=ctypes.c_void_p(coarse.ctypes.data + 2))):
        assert encode(**bad) == -1, bad
    assert L.lib.lsf_reloc_encode(ptr(depth), 1, None, ptr(coarse), ptr(counts), ptr(record), None, None) == -1

    ferns, decisions, capacity = 70, 4, 5
    loc, chan, thr = _host(ferns * 8, np.int32), _host(ferns * 8), _host(ferns * 8, np.float32)
    codes, n, code, dist = _host(capacity * ferns), _host(1, np.int32), _host(ferns), _host(capacity, np.int32)

    def query(change=None, **override):
        p = D.query_params((3, 4), 1, ferns, decisions, capacity, 1, True, 15)
        for name, value in (change or {}).items():
            setattr(p, name, value)
        a = dict(coarse=ptr(coarse), loc=ptr(loc), chan=ptr(chan), thr=ptr(thr), codes=ptr(codes), n=ptr(n),
                 code=ptr(code), dist=ptr(dist), record=ptr(record))
        a.update(override)
        return L.lib.lsf_reloc_query(a["coarse"], a["loc"], a["chan"], a["thr"], a["codes"], a["n"], a["code"], a["dist"],
                                     a["record"], ctypes.byref(p), None)

    for bad in (dict(decisions=0), dict(decisions=9), dict(candidates=0), dict(candidates=5), dict(ferns=0),
                dict(ferns=L.RELOC_MAX_FERNS + 1), dict(capacity=0), dict(harvest=2), dict(harvest_differing=0),
                dict(channels=3), dict(coarse_width=0)):
        assert query(bad) == -1, bad
    for name in ("coarse", "loc", "chan", "thr", "codes", "n", "code", "dist", "record"):  # a NULL table, a NULL anything
        assert query(**{name: None}) == -1, name
    assert query(codes=ctypes.c_void_p(codes.ctypes.data + 4)) == -1   # the rows are read as 16-byte words
    assert query(dist=ptr(record)) == -1                               # overlap
    assert query(dict(capacity=2 ** 30, ferns=4096)) == -2             # LSF_ERR_BAD_DIMS


def test_wrapper_rules_that_need_no_device(lsf):
    from levelsetfusion_python_amd import device_relocaliser as D
    assert D.harvest_differing_of(0.2, 500) == 101 and D.harvest_differing_of(0.2, 256) == 52
    assert D.harvest_differing_of(0.0, 70) == 1 == R.harvest_differing(0.0, 70)
    for bad in (-0.1, 1.0, math.nan):
        with pytest.raises(ValueError):
            D.harvest_differing_of(bad, 100)
    for bad in ((0.0, 1.0), (2.0, 1.0), (1.0, 1.0), (0.5, 65.0), (0.5, math.inf), (0.5,), 3.0):
        with pytest.raises((ValueError, TypeError)):
            D.depth_range_of(bad)
    for bad in ((0, 4), (3, 4, 5), (2.5, 4), 7):
        with pytest.raises((ValueError, TypeError)):
            D.coarse_shape_of(bad)
    with pytest.raises(ValueError):
        D.encode_params((12, 16), (13, 4), (0.5, 4.0))
    with pytest.raises(ValueError):
        D.encode_params((12, 16), (3, 4), (0.5, 4.0), depth_unit_ratio=0)
    for bad in (dict(decisions=0), dict(decisions=9), dict(candidates=0), dict(candidates=5), dict(ferns=0),
                dict(ferns=4097), dict(capacity=0), dict(channels=2)):
        kw = dict(coarse_shape=(3, 4), channels=1, ferns=70, decisions=4, capacity=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.query_params(**kw)
    rec = np.array([3, 1, 2, -1, -1, 0, 4, -1, -1, -1, 1, 0], np.int32)
    assert D.unpack_query_record(rec) == {"n": 3, "nearest": [1, 2], "distances": [0, 4], "appended": None,
                                          "full": True}


def test_tracking_quality(lsf):
    Q = lsf.fusion.TrackingQuality
    q = Q()
    assert q.min_pair_fraction == 0.25 and q.max_rms == math.inf
    rec = {"count": 1200, "energy": 1200 * 1e-6, "skipped": 0}
    for stride, shape in ((1, (60, 80)), (2, (120, 160)), (4, (240, 320))):
        v = q.judge(rec, shape, stride)
        assert v == R.judge(rec, shape, stride) and v["good"] and v["pair_fraction"] == 0.25
        assert abs(v["rms"] - 1e-3) < 1e-15
    assert not q.judge(dict(rec, count=1199), (60, 80), 1)["good"]
    assert not q.judge(dict(rec, skipped=1), (60, 80), 1)["good"]
    assert not Q(max_rms=9e-4).judge(rec, (60, 80), 1)["good"] and Q(max_rms=1e-3 + 1e-12).judge(rec, (60, 80), 1)["good"]
    assert q.judge(None, (60, 80), 1) == {"good": True, "pair_fraction": None, "rms": None, "skipped": False}
    empty = Q(min_pair_fraction=0).judge({"count": 0, "energy": 0.0, "skipped": 1}, (60, 80), 1)
    assert empty == {"good": False, "pair_fraction": 0.0, "rms": 0.0, "skipped": True}
    for bad in (dict(min_pair_fraction=-0.1), dict(min_pair_fraction=1.5), dict(min_pair_fraction=math.nan),
                dict(max_rms=-1.0), dict(max_rms=math.nan)):
        with pytest.raises(ValueError):
            Q(**bad)


def test_relocaliser_host_rules(lsf):
    from levelsetfusion_python_amd.fusion import relocaliser as M
    Rl = lsf.fusion.Relocaliser
    r = Rl()
    assert (r.ferns, r.decisions, r.coarse_shape, r.depth_range) == (500, 4, (30, 40), (0.2, 4.0))
    assert (r.max_keyframes, r.candidates, r.resume_after, r.harvest_differing) == (1024, 1, 0, 101)
    assert r.keyframes()[0].shape == (0, 500) and r.keyframes()[1].shape == (0, 6)
    for bad in (dict(ferns=0), dict(ferns=4097), dict(decisions=9), dict(decisions=0), dict(coarse_shape=(0, 4)),
                dict(depth_range=(1.0, 0.5)), dict(depth_range=(0.2, 65.0)), dict(harvest_threshold=1.0),
                dict(max_keyframes=0), dict(candidates=5), dict(candidates=0), dict(resume_after=-1),
                dict(resume_after=1.5)):
        with pytest.raises(ValueError):
            Rl(**bad)
    with pytest.raises(ValueError):
        r.query(None)  # nothing encoded yet
    for colour in (False, True):
        mine = M.fern_table(70, 8, (5, 7), (0.3, 2.0), colour, 11)
        want = R.fern_table(70, 8, (5, 7), (0.3, 2.0), colour, 11)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(mine, want))
        loc, chan, thr = mine
        assert loc.min() >= 0 and loc.max() < 35 and chan.max() == (3 if colour else 0)
        assert np.all((thr[chan == 0] >= 0.3) & (thr[chan == 0] <= 2.0)) and np.all((thr >= 0) & (thr <= 255))
    assert not np.array_equal(M.fern_table(70, 8, (5, 7), (0.3, 2.0), False, 12)[0], loc)

    class Tracker:
        pyramid, strides, iterations = None, (4, 2, 1), (4, 5, 10)
    assert [M.level_stride(Tracker, k) for k in range(3)] == [4, 2, 1]
    Tracker.pyramid = object()
    assert [M.level_stride(Tracker, k) for k in range(3)] == [4, 2, 1]  # pyramid level 2, 1, 0
    Tracker.iterations = (4, 5)
    assert [M.level_stride(Tracker, k) for k in range(2)] == [2, 1]


def test_header_binding_exports_and_documents_agree(lsf):
    header = open(lsf._build.ABI_HEADER).read()
    L = lsf._lib
    for macro, value in (("LSF_RELOC_MAX_BLOCKS", L.RELOC_MAX_BLOCKS), ("LSF_RELOC_MAX_FERNS", L.RELOC_MAX_FERNS),
                         ("LSF_RELOC_MAX_DECISIONS", L.RELOC_MAX_DECISIONS),
                         ("LSF_RELOC_MAX_CANDIDATES", L.RELOC_MAX_CANDIDATES),
                         ("LSF_RELOC_ENCODE_RECORD_WORDS", L.RELOC_ENCODE_RECORD_WORDS),
                         ("LSF_RELOC_QUERY_RECORD_WORDS", L.RELOC_QUERY_RECORD_WORDS)):
        assert "#define %s %d\n" % (macro, value) in header, macro
    assert "#define LSF_RELOC_MAX_DEPTH 64.0\n" in header and L.RELOC_MAX_DEPTH == 64.0
    assert R.MAX_CANDIDATES == L.RELOC_MAX_CANDIDATES and (L.RELOC_MAX_DECISIONS, L.RELOC_MAX_CANDIDATES) == (8, 4)
    assert "lsf_relocaliser.hip" in lsf._build.SOURCES and L.ABI_VERSION == 4
    for name, args in (("lsf_reloc_encode", 8), ("lsf_reloc_query", 11)):
        assert name + "(" in header and len(L.PROTOTYPES[name][1]) == args
    assert ctypes.sizeof(L.RelocParams) == 8 * 3 + 4 * 12 and L.RelocParams.height.offset == 24
    assert {"Relocaliser", "TrackingQuality"} <= set(lsf.fusion.__all__)
    parameters = inspect.signature(lsf.fusion.SequenceFusion3d.__init__).parameters
    assert "tracking_quality" in parameters and "relocaliser" in parameters
    root = os.path.join(os.path.dirname(lsf._build.ABI_HEADER), "..")
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "Tracking quality and relocalisation" in doc and "lsf_reloc_query" in doc and "lsf_reloc_encode" in doc
    assert "Relocaliser" in open(os.path.join(root, "README.md")).read()
    assert "lsf_relocaliser.hip" in open(os.path.join(root, "DESIGN.md")).read()


def _camera(lsf):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)


# ---- the inputs of the GPU tests, and what their shapes cross ---------------------------------------------------------------
# tests/test_gpu_relocaliser.py and the relocaliser sections of tests/test_gpu_second_trip.py draw their inputs here, so
# that what is assumed about them -- which cap a shape crosses, and that work with a visible effect lies past it -- is
# checked without a card.  The constants mirror csrc/lsf_relocaliser.hip.

RELOC_MAX_BLOCKS = 1024  # LSF_RELOC_MAX_BLOCKS (include/lsf_hip.h): workgroups of the encode and the distance kernel
RELOC_BLOCK = 256        # kBlock (csrc/lsf_device.h): the lanes of the one-workgroup record and select kernels
RELOC_WAVE = 64          # kWave: the lanes that walk a block's pixels, and a row's 16-byte words
RELOC_BLOCK_WAVES = RELOC_BLOCK // RELOC_WAVE  # kBlockWaves: coarse blocks, or keyframe rows, per workgroup
RELOC_WAVES = RELOC_MAX_BLOCKS * RELOC_BLOCK_WAVES  # the waves of a capped grid: blocks or rows of the first trip
RELOC_WORD = 16          # the bytes of a word of the distance kernel: a row's first trip ends before its byte 64 * 16
RELOC_MAX_FERNS = 4096   # LSF_RELOC_MAX_FERNS: the LDS copy of the frame's code


def depth_image(shape, coarse_shape, dtype, rng):
    """metres in [0.3, 3.9] with zeros, values outside [0.5, 3.5], a NaN and an inf (float types), and two blocks set by
    hand: block (0, 1) with exactly half of its pixels counting (the next whole number when they are odd), block (0, 0)
    with one fewer"""
    h, w = shape
    d = rng.uniform(0.3, 3.9, shape)
    d[rng.random(shape) < 0.15] = 0.0
    d[rng.random(shape) < 0.05] = 7.5
    ch, cw = coarse_shape
    for j, fewer in ((0, 1), (1, 0)):
        rows, cols = slice(0, h // ch), slice(j * w // cw, (j + 1) * w // cw)
        block = np.zeros(((h // ch), cols.stop - cols.start))
        n = block.size // 2 - fewer if block.size % 2 == 0 else (block.size + 1) // 2 - fewer
        block.reshape(-1)[:n] = rng.uniform(0.6, 3.0, n)
        d[rows, cols] = block
    if dtype == np.uint16:
        return np.round(d * 1000.0).astype(np.uint16), 0.001
    d = d.astype(dtype)
    d[h // 2, w // 2], d[h // 2, w // 2 + 1] = np.nan, np.inf
    return d, 1.0


def block_slices(shape, coarse_shape, i, j):
    (h, w), (ch, cw) = shape, coarse_shape
    return slice(i * h // ch, (i + 1) * h // ch), slice(j * w // cw, (j + 1) * w // cw)


def block_pixels(shape, coarse_shape):
    """int (ch, cw): the pixels of every coarse block, from the slices the restatement cuts"""
    ch, cw = coarse_shape
    size = lambda s: s.stop - s.start
    return np.array([[size(block_slices(shape, coarse_shape, i, j)[0]) * size(block_slices(shape, coarse_shape, i, j)[1])
                      for j in range(cw)] for i in range(ch)])


PIXEL_LOOP_IMAGES = (((37, 53), (2, 3)), ((480, 640), (30, 40)))  # (frame, coarse image): blocks of several waves
LATE_BLOCKS = ((-1, -1), (-1, 0))  # the last block of the coarse image and the first of its last row


def pixel_loop_image(shape, coarse_shape, dtype):
    """depth_image with two more blocks set by hand, pixels counted row-major inside a block as the kernel's lanes walk
    them: the last block has zeros in its first RELOC_WAVE pixels and counting depths in all the others, so everything
    that counts there lies in a later trip, and the first block of the last row keeps only pixels of its last trip.
    Returns (depth, ratio)."""
    rng = np.random.default_rng(shape[0] + np.dtype(dtype).itemsize)
    depth, ratio = depth_image(shape, coarse_shape, dtype, rng)
    for (i, j), keep_from in zip(LATE_BLOCKS, (RELOC_WAVE, None)):
        at = block_slices(shape, coarse_shape, i % coarse_shape[0], j % coarse_shape[1])
        flat = depth[at].reshape(-1)  # a copy: the block is not contiguous
        first = (len(flat) - 1) // RELOC_WAVE * RELOC_WAVE if keep_from is None else keep_from
        flat[:first] = 0
        if keep_from is not None:
            flat[first:] = (rng.uniform(0.6, 3.0, len(flat) - first) / ratio).astype(flat.dtype)
        depth[at] = flat.reshape(depth[at].shape)
    return depth, ratio


def check_pixel_loop_image(shape, coarse_shape, depth, ratio, want, want_counts):
    """the crossing of `for (p = lane; p < pixels; p += kWave)` and its effect, from the restatement's outputs"""
    pixels = block_pixels(shape, coarse_shape)
    assert pixels.min() > RELOC_WAVE  # every block takes a second trip
    trips = -(-pixels // RELOC_WAVE)
    if shape == (37, 53):
        assert sorted(set(trips.reshape(-1))) == [5, 6] and np.all(pixels % RELOC_WAVE != 0)  # a ragged last trip
        # two workgroups, the second with two of its four waves idle
        assert pixels.size == RELOC_BLOCK_WAVES + 2
    else:
        assert np.all(pixels == 4 * RELOC_WAVE) and pixels.size <= RELOC_WAVES  # the header's case: four whole trips
    with np.errstate(invalid="ignore"):
        d = R.scaled_depth(depth, ratio)
        counting = (d >= 0.5) & (d <= 3.5)
    (i, j), (k, l) = LATE_BLOCKS
    late = counting[block_slices(shape, coarse_shape, i % coarse_shape[0], j % coarse_shape[1])].reshape(-1)
    # a kernel that stops after one trip counts nothing here and writes 0; the block is valid
    assert not late[:RELOC_WAVE].any() and want_counts[i, j] == late.sum() and want[i, j, 0] > 0
    last = counting[block_slices(shape, coarse_shape, k % coarse_shape[0], l % coarse_shape[1])].reshape(-1)
    start = (len(last) - 1) // RELOC_WAVE * RELOC_WAVE
    assert start >= RELOC_WAVE and not last[:start].any() and want_counts[k, l] == last[start:].sum() > 0
    assert want[k, l, 0] == 0  # fewer than half: the count alone shows the last trip


BLOCK_LOOP_COARSE = (65, 64)
BLOCK_LOOP_IMAGES = ((65, 64), (131, 129))  # one pixel per block; blocks of 2 or 3 rows by 2 or 3 columns


def check_block_loop_image(shape, want, want_counts, want_record):
    """the crossing of the encode kernel's `b += waves` and its effect, from the restatement's outputs"""
    pixels = block_pixels(shape, BLOCK_LOOP_COARSE)
    assert RELOC_WAVES < pixels.size <= RELOC_WAVES + RELOC_WAVE  # the first 64 waves take a second block
    assert (pixels.min(), pixels.max()) == ((1, 1) if shape == BLOCK_LOOP_IMAGES[0] else (4, 9))
    valid, counts = (want[..., 0] > 0).reshape(-1), want_counts.reshape(-1)
    for side in (slice(0, RELOC_WAVES), slice(RELOC_WAVES, None)):  # valid and invalid blocks on both sides
        assert valid[side].any() and not valid[side].all()
    # the record's sums include the blocks past the cap
    assert want_record["counting"] == counts.sum() > counts[:RELOC_WAVES].sum()
    assert want_record["valid_blocks"] == valid.sum() > valid[:RELOC_WAVES].sum()


LATE_ROWS = (5, 11)  # keyframes of query_case(late=True) that differ from the frame only past a row's first trip


@functools.lru_cache(maxsize=None)
def query_case(ferns, decisions, colour, late=False):
    """a coarse image with empty blocks, a table that also points outside it, and 131 keyframe codes around the frame's.
    With late, the keyframes LATE_ROWS differ from the frame only at byte >= 64 * 16 of their row (in every later trip
    where the row has one)"""
    rng = np.random.default_rng(ferns * 10 + decisions)
    ch, cw, c = 6, 9, 4 if colour else 1
    coarse = rng.uniform(0.5, 3.5, (ch, cw, c)).astype(np.float32)
    if colour:
        coarse[..., 1:] = rng.uniform(0, 255, (ch, cw, 3)).astype(np.float32)
    coarse[rng.random((ch, cw)) < 0.2] = 0
    table = list(R.fern_table(ferns, decisions, (ch, cw), (0.5, 3.5), colour, 3))
    table[0][0, 0], table[0][1, 0] = ch * cw, -1  # outside: bit 0
    if not colour:
        table[1][2, 0] = 1                        # a channel the image does not have: bit 0
    code = R.frame_code(coarse, *table)
    rows = np.repeat(code[None, :], 131, axis=0)
    for k in range(131):  # keyframe k differs in (k * 7) % (ferns + 1) ferns: distances in no order
        flip = rng.permutation(ferns)[:(k * 7) % (ferns + 1)]
        rows[k, flip] ^= rng.integers(1, 1 << decisions, len(flip)).astype(np.uint8)
    rows[57] = rows[23]  # two keyframes with equal codes
    if late:
        first = RELOC_WAVE * RELOC_WORD
        for k, flip in zip(LATE_ROWS, (np.arange(first, ferns, max(1, (ferns - first) // 40)), np.arange(first, ferns)[:3])):
            rows[k] = code
            rows[k, flip] ^= 1
    return coarse, tuple(table), rows


def check_word_loop_case(ferns, coarse, table, rows):
    """the crossing of the distance kernel's `w += kWave` and its effect.  Row k is read as the 16-byte words from byte
    k F - (k F) % 16 on, 64 of them in a trip: the first trip ends at or before byte 1024 of the row"""
    first = RELOC_WAVE * RELOC_WORD
    assert first < ferns <= RELOC_MAX_FERNS
    code = R.frame_code(coarse, *table)
    want = R.query(coarse, table, rows, len(rows))[1]
    for k in LATE_ROWS:  # a kernel that stops after the first trip reports 0 for them
        assert np.array_equal(rows[k, :first], code[:first]) and want[k] > 0
        assert want[k] < (23 * 7) % (ferns + 1)  # nearer than the twins the comparison's tie rests on
    if ferns == RELOC_MAX_FERNS:  # rows aligned, four whole trips, each of the later three with a differing fern
        assert ferns % RELOC_WORD == 0 and ferns == 4 * first
        assert all((rows[LATE_ROWS[0], t * first:(t + 1) * first] != code[t * first:(t + 1) * first]).any()
                   for t in (1, 2, 3))
    else:  # rows off the alignment, a ragged last word, a last word that reaches past the array
        assert ferns % RELOC_WORD and (len(rows) * ferns) % RELOC_WORD


ROW_LOOP_CAPACITY, ROW_LOOP_FERNS = 4101, 70
# per case: keyframe -> its distance.  "spread": the four nearest lie in the select kernel's first trip (k < 256), in a
# later one, and in the distance kernel's second trip (k >= 4096), and the tie of 4000 and 4097 straddles that cap;
# "far-first": the overall nearest is the last row (outside the database when n is one below the capacity), the tie of
# 150 and 4096 has one twin in each kernel's first trip and one past both caps
ROW_LOOP_CASES = {"spread": {3000: 2, 4098: 3, 100: 4, 4000: 5, 4097: 5},
                  "far-first": {4100: 1, 150: 2, 4096: 2, 2000: 3}}
ROW_LOOP_TWINS = {"spread": (4000, 4097), "far-first": (150, 4096)}


@functools.lru_cache(maxsize=None)
def row_loop_case(name):
    """(coarse, table, rows uint8 (ROW_LOOP_CAPACITY, 70)): every keyframe 10 to 70 ferns from the frame, except the
    near ones of ROW_LOOP_CASES[name]; the twins have equal codes"""
    coarse, table, _ = query_case(ROW_LOOP_FERNS, 4, True)
    code = R.frame_code(coarse, *table)
    rng = np.random.default_rng(len(name))
    rows = np.repeat(code[None, :], ROW_LOOP_CAPACITY, axis=0)
    near = ROW_LOOP_CASES[name]
    for k in range(ROW_LOOP_CAPACITY):
        flip = rng.permutation(ROW_LOOP_FERNS)[:near.get(k, int(rng.integers(10, ROW_LOOP_FERNS + 1)))]
        rows[k, flip] ^= rng.integers(1, 16, len(flip)).astype(np.uint8)
    a, b = ROW_LOOP_TWINS[name]
    rows[b] = rows[a]
    rows.setflags(write=False)
    return coarse, table, rows


def check_row_loop_case(name, coarse, table, rows):
    """the crossing of the distance kernel's `k += waves` and the select kernel's `k += kBlock`, and their effect"""
    capacity, ferns = rows.shape
    assert capacity > RELOC_WAVES + RELOC_BLOCK_WAVES and capacity > RELOC_BLOCK and (capacity * ferns) % RELOC_WORD
    near = ROW_LOOP_CASES[name]
    _, distances, record, _, _ = R.query(coarse, table, rows, capacity, candidates=4)
    assert {k: int(distances[k]) for k in near} == near and int(np.sort(distances)[len(near)]) >= 10
    ids = record[1:5].tolist()
    a, b = ROW_LOOP_TWINS[name]
    assert a < RELOC_WAVES <= b and distances[a] == distances[b] and np.array_equal(rows[a], rows[b])
    if name == "spread":
        assert ids == [3000, 4098, 100, 4000]  # the tie goes to the lower id, 4097 stays out
    else:
        assert ids == [4100, 150, 4096, 2000]
        assert R.query(coarse, table, rows, capacity - 1, candidates=4)[2][1:5].tolist()[:3] == [150, 4096, 2000]
    # a select kernel that looked at its first 256 keys only, or distances that stopped at row 4096, give other ids
    assert any(k < RELOC_BLOCK for k in ids) and any(RELOC_BLOCK <= k < RELOC_WAVES for k in ids)
    assert any(k >= RELOC_WAVES for k in ids)
    return int(record[5])


MANY_KEYFRAMES = dict(ferns=128, decisions=4, coarse_shape=(6, 8), depth_range=(0.5, 3.5), harvest_threshold=0.2,
                      max_keyframes=300, candidates=4, seed=9)
MANY_FRAMES, MANY_FRAME_SHAPE = 280, (24, 32)
MANY_AGAIN = (3, 150, 260, 279)  # frames shown a second time, without harvest


@functools.lru_cache(maxsize=None)
def many_frames():
    """MANY_FRAMES depth frames of one random depth per coarse block (blocks of 4 x 4 pixels) with some blocks empty: two of
    them agree in about a fifth of their ferns, so every one is harvested"""
    rng = np.random.default_rng(31)
    ch, cw = MANY_KEYFRAMES["coarse_shape"]
    out = []
    for _ in range(MANY_FRAMES):
        blocks = rng.uniform(0.5, 3.5, (ch, cw))
        blocks[rng.random((ch, cw)) < 0.1] = 0.0
        frame = np.kron(blocks, np.ones((MANY_FRAME_SHAPE[0] // ch, MANY_FRAME_SHAPE[1] // cw))).astype(np.float32)
        frame.setflags(write=False)
        out.append(frame)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def many_keyframes_restated():
    """the restated database over many_frames() with harvest, then MANY_AGAIN without: (per frame the restated coarse
    image, per query the restated dict, the database)"""
    db = R.Database(**MANY_KEYFRAMES)
    coarse = [db.encode(f, 1.0) for f in many_frames()]
    twists = [np.full(6, k, np.float64) for k in range(MANY_FRAMES)]
    found = [db.query(c, True, t) for c, t in zip(coarse, twists)]
    found += [db.query(coarse[k]) for k in MANY_AGAIN]
    return coarse, found, db


def test_the_second_trip_inputs_cross_their_caps(lsf):
    """what tests/test_gpu_second_trip.py assumes about its relocaliser inputs, from constants and the restatement"""
    L = lsf._lib
    assert (RELOC_MAX_BLOCKS, RELOC_MAX_FERNS) == (L.RELOC_MAX_BLOCKS, L.RELOC_MAX_FERNS)
    assert RELOC_WAVES == 4096 and RELOC_BLOCK_WAVES == 4
    for shape, coarse_shape in PIXEL_LOOP_IMAGES:
        for dtype in (np.float32, np.uint16):
            depth, ratio = pixel_loop_image(shape, coarse_shape, dtype)
            want, want_counts, _ = R.encode(depth, ratio, coarse_shape, (0.5, 3.5))
            check_pixel_loop_image(shape, coarse_shape, depth, ratio, want, want_counts)
    for shape in BLOCK_LOOP_IMAGES:
        depth, ratio = depth_image(shape, BLOCK_LOOP_COARSE, np.float32, np.random.default_rng(shape[0]))
        check_block_loop_image(shape, *R.encode(depth, ratio, BLOCK_LOOP_COARSE, (0.5, 3.5)))
    for ferns, decisions in ((1030, 8), (RELOC_MAX_FERNS, 1)):
        check_word_loop_case(ferns, *query_case(ferns, decisions, False, True))
    for name in ROW_LOOP_CASES:
        assert check_row_loop_case(name, *row_loop_case(name)) == min(ROW_LOOP_CASES[name].values())
    _, found, db = many_keyframes_restated()
    assert db.n == MANY_FRAMES > RELOC_BLOCK and [f["appended"] for f in found[:MANY_FRAMES]] == list(range(MANY_FRAMES))
    again = found[MANY_FRAMES:]
    assert [f["nearest"][0] for f in again] == list(MANY_AGAIN) and all(f["distances"][0] == 0 for f in again)
    assert max(MANY_AGAIN) >= RELOC_BLOCK > min(MANY_AGAIN)  # nearest keyframes in the select kernel's second trip too


def test_sequence_constructor_refusals(lsf):
    """SequenceFusion3d refuses before it allocates, so these need no card"""
    F = lsf.fusion
    make = lambda **kw: lsf.SequenceFusion3d(_camera(lsf), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                                             narrow_band_width_voxels=MS.BAND, **kw)
    for mode in ("model", "raycast"):
        with pytest.raises(ValueError, match="icp"):
            make(tracking_reference=mode, tracking_quality=F.TrackingQuality())
        with pytest.raises(ValueError, match="icp"):
            make(tracking_reference=mode, relocaliser=F.Relocaliser())
    with pytest.raises(ValueError, match="icp"):
        make(relocaliser=F.Relocaliser())  # the default mode is "model"
    policy = F.MovingVolume(MS.THRESHOLD, MS.ANCHOR)
    with pytest.raises(ValueError, match="out of scope"):
        make(tracking_reference="icp", relocaliser=F.Relocaliser(), moving_volume=policy)
    for bad in (0.25, "lost", dict(min_pair_fraction=0.25), F.Relocaliser()):
        with pytest.raises(ValueError, match="TrackingQuality"):
            make(tracking_reference="icp", tracking_quality=bad)
    for bad in (True, "ferns", F.TrackingQuality()):
        with pytest.raises(ValueError, match="Relocaliser"):
            make(tracking_reference="sdf", relocaliser=bad)
