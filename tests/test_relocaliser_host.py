"""Host checks of tracking quality and relocalisation (no GPU): properties of the numpy restatement
(tests/relocaliser_restatement.py) on the scene of tests/moving_volume_scene.py -- the fern distance grows along the pass,
a blank frame is far from everything, harvesting keeps a strict subset, and the restated sequence recovers from a
kidnapped camera (scene A) and from leaving the fixed window and coming back (scene B) where the sequence without the
keywords does not --, the refusals of lsf_reloc_encode and lsf_reloc_query that run before any launch, the host rules of
fusion.TrackingQuality and fusion.Relocaliser, and SequenceFusion3d's constructor refusals."""
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
