"""GPU checks of the moving volume: lsf_volume_shift (csrc/lsf_volume_shift.hip) against the numpy restatement
(tests/volume_shift_restatement.py) bit for bit as uint32, the wrapper's refusals, CanonicalVolume.shift's buffer swap,
the streamed chunks as a partition of the mesh, fusion in a moved window against fusion in a fixed volume, and
SequenceFusion3d(moving_volume=) over the analytic scene of tests/moving_volume_scene.py.
The kernel's unit of work is a row (z, y): a wave per row, LSF_VOLUME_SHIFT_BLOCK_ROWS rows per workgroup, at most
LSF_VOLUME_SHIFT_MAX_BLOCKS workgroups.  (33, 34, 70) has 1122 rows and so runs several workgroups inside the grid's
first trip; (65, 127, 7) has more rows than one trip holds and runs the stride loop's second."""
import functools

import numpy as np
import pytest
import torch

import moving_volume_scene as MS
import volume_shift_restatement as V
from test_gpu_mesh import _sphere
from test_volume_shift_host import PREFIX, _special_volume, always_inside

pytestmark = pytest.mark.gpu

SHIFT_MAX_BLOCKS, SHIFT_BLOCK_ROWS = 2048, 4  # LSF_VOLUME_SHIFT_MAX_BLOCKS, LSF_VOLUME_SHIFT_BLOCK_ROWS (include/lsf_hip.h)
FIRST_TRIP_ROWS = SHIFT_MAX_BLOCKS * SHIFT_BLOCK_ROWS
VOLUMES = ((2, 2, 2), (5, 7, 9), (3, 4, 67), (33, 34, 70), (65, 127, 7))  # (Z, Y, X)
GARBAGE = 0x5a5a5a5a  # what the destinations hold before the call: every voxel must be written


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _camera():
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _shifts(shape):
    """(sx, sy, sz): zero, +-1 per axis, aligned and misaligned rows, three axes at once, one layer retained, and
    everything reset by one axis"""
    z, y, x = shape
    out = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (4, 0, 0), (3, 0, 0),
           (2, -3, 1), (x - 1, 0, 0), (0, -(y - 1), 0), (0, 0, z - 1), (-(x - 1), y - 1, 0),
           (x, 0, 0), (0, -y, 0), (0, 0, z), (x + 5, 0, 0), (0, y + 5, 0), (0, 0, -(z + 5))]
    return out


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    rng = np.random.default_rng(sum(shape))
    arrays = (_special_volume(shape, rng), _special_volume(shape, rng), _special_volume(shape, rng, (4,)))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _garbage(shape, extra=()):
    return torch.full(tuple(shape) + tuple(extra), GARBAGE, dtype=torch.int32, device="cuda").view(torch.float32)


def _offset_view(a, words):
    """a device copy of float32 array `a` that starts `words` floats past a 16-byte boundary"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[words:words + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.data_ptr() % 16 == 4 * words and view.is_contiguous()
    return view


def test_the_listed_volumes_sit_where_the_docstring_says():
    rows = [z * y for z, y, _ in VOLUMES]
    assert rows[3] == 1122 and SHIFT_BLOCK_ROWS < rows[3] < FIRST_TRIP_ROWS
    assert FIRST_TRIP_ROWS < rows[4] < 2 * FIRST_TRIP_ROWS
    assert VOLUMES[2][2] > 64 and VOLUMES[2][2] % 2 == 1 and VOLUMES[3][2] > 64


@pytest.mark.parametrize("with_colour", [False, True])
@pytest.mark.parametrize("shape", VOLUMES)
def test_kernel_against_restatement(lsf, shape, with_colour):
    from levelsetfusion_python_amd import device_volume_shift as D
    t, w, c = _inputs(shape)
    dt, dw = (torch.from_numpy(np.array(a)).cuda() for a in (t, w))
    dc = torch.from_numpy(np.array(c)).cuda() if with_colour else None
    for s in _shifts(shape):
        ot, ow = _garbage(shape), _garbage(shape)
        oc = _garbage(shape, (4,)) if with_colour else None
        D.shift(dt, dw, dc, ot, ow, oc, s)
        want_t, want_w, want_c = V.shift_model(t, w, c if with_colour else None, s)
        assert np.array_equal(_u32(ot), want_t.view(np.uint32)), s
        assert np.array_equal(_u32(ow), want_w.view(np.uint32)), s
        if with_colour:
            assert np.array_equal(_u32(oc), want_c.view(np.uint32)), s
        if s == (0, 0, 0):
            assert np.array_equal(_u32(ot), t.view(np.uint32))
    assert np.array_equal(_u32(dt), t.view(np.uint32)) and np.array_equal(_u32(dw), w.view(np.uint32))  # read only


@pytest.mark.parametrize("side", ["source", "destination"])
def test_views_four_bytes_past_a_16_byte_boundary(lsf, side):
    from levelsetfusion_python_amd import device_volume_shift as D
    shape = (5, 7, 9)
    t, w, c = _inputs(shape)
    for s in ((3, 0, 0), (4, 0, 0), (2, -3, 1), (0, 0, 0)):
        if side == "source":
            dt, dw = _offset_view(t, 1), _offset_view(w, 1)
            ot, ow = _garbage(shape), _garbage(shape)
        else:
            dt, dw = (torch.from_numpy(np.array(a)).cuda() for a in (t, w))
            ot, ow = _offset_view(np.zeros(shape, np.float32), 1), _offset_view(np.zeros(shape, np.float32), 1)
        dc, oc = torch.from_numpy(np.array(c)).cuda(), _garbage(shape, (4,))
        D.shift(dt, dw, dc, ot, ow, oc, s)
        want_t, want_w, want_c = V.shift_model(t, w, c, s)
        assert np.array_equal(_u32(ot), want_t.view(np.uint32)) and np.array_equal(_u32(ow), want_w.view(np.uint32))
        assert np.array_equal(_u32(oc), want_c.view(np.uint32))
    dt, dw = (torch.from_numpy(np.array(a)).cuda() for a in (t, w))
    with pytest.raises(ValueError):  # a colour record is one 16-byte access
        D.shift(dt, dw, _offset_view(c, 1), _garbage(shape), _garbage(shape), _garbage(shape, (4,)), (1, 0, 0))
    with pytest.raises(ValueError):
        D.shift(dt, dw, torch.from_numpy(np.array(c)).cuda(), _garbage(shape), _garbage(shape),
                _offset_view(c, 1), (1, 0, 0))


def test_refusals(lsf):
    from levelsetfusion_python_amd import _lib as L, device_volume_shift as D
    import ctypes
    shape = (4, 5, 6)
    new = lambda *extra: torch.zeros(shape + extra, dtype=torch.float32, device="cuda")
    t, w, ot, ow = new(), new(), new(), new()
    D.shift(t, w, None, ot, ow, None, (1, 0, 0))
    for bad in ((t, w, None, t, ow, None),            # aliased source and destination
                (t, w, None, ot, w, None),
                (t, w, None, ot, ot, None),           # two destinations are one
                (t, w, new(4), ot, ow, None),         # one colour missing
                (t, w, None, ot, ow, new(4)),
                (t, w, None, new()[:3], ow, None),    # mismatched shapes
                (t, new()[:, :4], None, ot, ow, None),
                (t, w, new(3), ot, ow, new(3)),
                (t, w, None, ot.cpu(), ow, None),     # a CPU tensor
                (t.cpu(), w, None, ot, ow, None),
                (t.double(), w, None, ot, ow, None)):
        with pytest.raises((ValueError, TypeError)):
            D.shift(*bad, (1, 0, 0))
    colour = new(4)
    with pytest.raises(ValueError):
        D.shift(t, w, colour, ot, ow, colour, (1, 0, 0))
    flat = torch.zeros((5, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):  # a 2-D volume
        D.shift(flat, flat.clone(), None, flat.clone(), flat.clone(), None, (1, 0, 0))
    for bad in ((0.5, 0, 0), (1, 0), (1, 0, 0, 0)):
        with pytest.raises(ValueError):
            D.shift(t, w, None, ot, ow, None, bad)
    D.shift(t, w, None, ot, ow, None, np.array([1, -1, 0], np.int64))  # integral numpy ints are accepted
    # the C entry's own checks, past the wrapper
    p = D.params(shape, (1, 0, 0))
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    call = lambda *a: L.lib.lsf_volume_shift(*a, ctypes.byref(p), None)
    assert call(ptr(t), ptr(w), None, ptr(t), ptr(ow), None) == -1
    assert call(ptr(t), ptr(w), ptr(colour), ptr(ot), ptr(ow), None) == -1
    assert call(ptr(t), ptr(w), None, ptr(ot), ptr(ow), ptr(colour)) == -1
    assert call(ptr(t), ptr(w), ctypes.c_void_p(colour.data_ptr() + 4), ptr(ot), ptr(ow), ptr(new(4))) == -1
    assert call(ptr(t), ptr(w), None, ctypes.c_void_p(t.data_ptr() + 16), ptr(ow), None) == -1  # partial overlap
    torch.cuda.synchronize()


def test_canonical_volume_shift_swaps_its_buffers(lsf):
    shape = (5, 7, 9)
    t, w, c = _inputs(shape)
    vol = lsf.fusion.CanonicalVolume(shape, colour=True)
    for dst, a in ((vol.tsdf, t), (vol.weight, w), (vol.colour, c)):
        dst.copy_(torch.from_numpy(np.array(a)))
    before = (vol.tsdf, vol.weight, vol.colour)
    off, chunks = vol.shift((0, 0, 0), [1.5, -2, 3])
    assert chunks == [] and np.array_equal(off, [1.5, -2, 3]) and vol._spare is None  # no launch, no allocation
    assert all(x is y for x, y in zip(before, (vol.tsdf, vol.weight, vol.colour)))
    off, chunks = vol.shift((2, -3, 1), [1.5, -2, 3])
    assert chunks == [] and off.dtype == np.float64 and np.array_equal(off, [3.5, -5, 4])
    first = {x.data_ptr() for x in (vol.tsdf, vol.weight, vol.colour)}
    spare = {x.data_ptr() for x in vol._spare}
    assert spare == {x.data_ptr() for x in before} and not (first & spare)
    want = V.shift_model(t, w, c, (2, -3, 1))
    for got, a in zip((vol.tsdf, vol.weight, vol.colour), want):
        assert np.array_equal(_u32(got), a.view(np.uint32))
    off, _ = vol.shift(np.array([-1, 1, 0]), off)
    assert np.array_equal(off, [2.5, -4, 4])
    assert {x.data_ptr() for x in (vol.tsdf, vol.weight, vol.colour)} == spare  # swapped back: nothing new
    assert {x.data_ptr() for x in vol._spare} == first
    want = V.shift_model(*want, (-1, 1, 0))
    for got, a in zip((vol.tsdf, vol.weight, vol.colour), want):
        assert np.array_equal(_u32(got), a.view(np.uint32))
    with pytest.raises(ValueError):
        lsf.fusion.CanonicalVolume((8, 8)).shift((1, 0, 0), [0, 0, 0])
    with pytest.raises(ValueError):
        lsf.fusion.CanonicalVolume(shape).shift((1, 0, 0), [0, 0, 0], colours=True)


# ---- streaming is a partition of the mesh ------------------------------------------------------------------------------

def _triangles(mesh, coloured):
    """(F, 9) float64 positions and (F, 9) colours of a mesh's triangles, the vertices of each triangle and then the
    triangles in lexicographic order of their positions (keys rounded to a micrometre: a thousandth of what separates
    two vertices here, a thousand times a float32 step)"""
    v, f = mesh[0].astype(np.float64), mesh[1]
    col = mesh[-1].astype(np.float64) if coloured else np.zeros_like(v)
    tri = np.concatenate([v[f], col[f]], axis=2)  # (F, 3, 6)
    key = np.round(tri[..., :3] * 1e6)
    out = np.empty_like(tri)
    for i in range(len(tri)):
        out[i] = tri[i][np.lexsort(key[i].T[::-1])]
    flat = out.reshape(len(out), 18)
    order = np.lexsort(np.round(out[..., :3] * 1e6).reshape(len(out), 9).T[::-1])
    flat = flat[order].reshape(-1, 3, 6)
    return flat[..., :3].reshape(-1, 9), flat[..., 3:].reshape(-1, 9)


@functools.lru_cache(maxsize=None)
def _sphere_pair():
    n = 24
    live = np.minimum(_sphere(n, (8.3, 9.1, 10.2), 5.4), _sphere(n, (15.2, 14.3, 12.9), 4.7))
    rng = np.random.default_rng(5)
    colour = rng.uniform(0, 255, (n, n, n, 4)).astype(np.float32)
    colour[..., 3] = rng.choice(np.array([0, 1, 2.5], np.float32), (n, n, n))
    return live, colour


def _pair_volume(lsf):
    live, colour = _sphere_pair()
    vol = lsf.fusion.CanonicalVolume(live.shape, colour=True)
    vol.integrate_volume(live)
    vol.colour.copy_(torch.from_numpy(colour))
    vol.weight[:9, :10, :9] = 0  # a corner through the first sphere's surface: min_weight decides there
    return vol


@pytest.mark.parametrize("coloured", [False, True])
def test_streamed_chunks_and_the_new_window_partition_the_mesh(lsf, coloured):
    off = np.array([-11.5, -12.0, 100.25])
    voxel = 0.004
    unweighted = None
    for s in ((5, 0, 0), (0, -7, 0), (0, 0, 7), (6, -7, 8), (-6, 5, -1), (24, 0, 0), (0, 0, -23), (-30, 2, 0)):
        vol = _pair_volume(lsf)
        whole = vol.extract_mesh(off, voxel, colours=coloured)
        if unweighted is None:
            vol.weight.fill_(1.0)
            unweighted = len(vol.extract_mesh(off, voxel)[1])
            vol = _pair_volume(lsf)
        assert 0 < len(whole[1]) < unweighted  # the weight-0 corner removed faces
        new_off, chunks = vol.shift(s, off, voxel, stream_mesh=True, colours=coloured)
        assert np.array_equal(new_off, off + np.array(s, np.float64)) and len(chunks) <= 3
        window = vol.extract_mesh(new_off, voxel, colours=coloured)
        parts = list(chunks) + [window]
        assert all(len(p) == len(whole) for p in parts) and all(len(c[1]) > 0 for c in chunks)
        assert sum(len(p[1]) for p in parts) == len(whole[1]), s  # face counts: exactly equal
        merged = lsf.fusion.merge_meshes(parts)
        assert len(merged[1]) == len(whole[1]) and merged[1].max() < len(merged[0])
        got_p, got_c = _triangles(merged, coloured)
        want_p, want_c = _triangles(whole, coloured)
        # positions to one float32 step: both round a float64 sum whose association differs by the box's origin
        step = np.spacing(np.abs(want_p).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got_p - want_p) <= step), s
        assert np.array_equal(got_c, want_c), s
        if max(abs(v) for v in s) >= 23:
            assert len(window[1]) == 0 and len(chunks) == 1  # nothing is retained: the one chunk is the whole volume
        else:
            assert len(window[1]) > 0 and len(chunks) >= 1
    vol = _pair_volume(lsf)
    _, chunks = vol.shift((6, -7, 8), off, voxel, stream_mesh=True, normals=True, colours=True)
    assert all(len(c) == 4 and c[2].dtype == np.float32 and c[3].dtype == np.uint8 for c in chunks) and chunks


# ---- shifting does not change what is fused ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frames(count):
    depth = [MS.render(MS.true_twist(k)) for k in range(count)]
    return depth, [MS.paint(d, MS.true_twist(k)) for k, d in enumerate(depth)]


def test_shifting_does_not_change_what_is_fused(lsf):
    depth, images = _frames(PREFIX)
    n, camera = MS.WINDOW, _camera()
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR, stream_mesh=False)
    window = lsf.fusion.CanonicalVolume(n, colour=True)
    off, offsets, shifts = MS.WINDOW_OFFSET.copy(), [], []
    for k in range(PREFIX):
        offsets.append(off.copy())
        window.integrate_depth(depth[k], camera, MS.true_twist(k), off, MS.VOXEL, MS.BAND, carve=True,
                               colour_image=images[k])
        if k < PREFIX - 1:
            s = policy.shift_for(MS.true_twist(k), off, (n,) * 3, MS.VOXEL)
            shifts.append(s)
            off, _ = window.shift(s, off, MS.VOXEL)
    assert sum(s != (0, 0, 0) for s in shifts) >= 2
    lo = np.min(offsets, axis=0)
    big_shape = tuple(int(v) for v in (np.max(offsets, axis=0) - lo + n)[::-1])
    big = lsf.fusion.CanonicalVolume(big_shape, colour=True)
    for k in range(PREFIX):
        big.integrate_depth(depth[k], camera, MS.true_twist(k), lo, MS.VOXEL, MS.BAND, carve=True,
                            colour_image=images[k])
    at = np.round(off - lo).astype(int)
    assert np.array_equal(at, off - lo)  # the offsets differ by whole voxels
    part = (slice(at[2], at[2] + n), slice(at[1], at[1] + n), slice(at[0], at[0] + n))
    keep = always_inside(offsets, off, n)
    # the band of one frame: what the last frame alone fuses into an empty window, without carving
    alone = lsf.fusion.CanonicalVolume(n).integrate_depth(depth[-1], camera, MS.true_twist(PREFIX - 1), off, MS.VOXEL,
                                                          MS.BAND)
    fused = lsf.fusion.unpack_record(alone.cpu().numpy())["fused"]
    assert int(keep.sum()) > fused > 0, (int(keep.sum()), fused)  # more than the band of one frame
    for name in ("tsdf", "weight", "colour"):
        a, b = _u32(getattr(big, name)[part]), _u32(getattr(window, name))
        assert np.array_equal(a[keep], b[keep]), name
    assert float(window.weight.cpu().numpy()[keep].max()) == PREFIX  # some of them saw every frame
    assert not np.array_equal(_u32(big.weight[part])[~keep], _u32(window.weight)[~keep])  # and the rest did not


# ---- end to end ------------------------------------------------------------------------------------------------------------

MARGIN_T, MARGIN_R = 0.001, 0.002  # a quarter of a voxel, and the angle that moves the anchor's depth by as much


def _pose_errors(twists):
    err = np.array(twists) - np.array([MS.true_twist(k) for k in range(len(twists))])
    return np.linalg.norm(err[:, :3], axis=1), np.linalg.norm(err[:, 3:], axis=1)


@functools.lru_cache(maxsize=None)
def _fixed_run(big):
    """SequenceFusion3d(tracking_reference="icp") over the scene WITHOUT a moving volume: in the window's first box, or
    (big) in a fixed volume that holds the whole path"""
    import levelsetfusion_python_amd as lsf
    depth, _ = _frames(MS.FRAMES)
    shape, off = (MS.WINDOW,) * 3, MS.WINDOW_OFFSET
    if big:
        extent = int(np.ceil(abs(MS.true_twist(MS.FRAMES - 1)[0]) / MS.VOXEL)) + 16
        shape = (MS.WINDOW + 16, MS.WINDOW + 32, MS.WINDOW + extent)
        off = MS.WINDOW_OFFSET - np.array([8, 16, 8], np.float64)
    seq = lsf.SequenceFusion3d(_camera(), shape, off, voxel_size=MS.VOXEL, narrow_band_width_voxels=MS.BAND,
                               tracking_reference="icp")
    for d in depth:
        seq.integrate(d)
    return seq


def test_a_sequence_in_a_moving_volume(lsf, capsys):
    """(i) the window shifts at least twice and the last frame still fuses and predicts; (ii) the same sequence in the
    same box without a moving volume ends with nothing to predict or fuse: as the camera leaves the box the prediction
    shrinks to a strip at the image's edge, the solve on it throws the pose off (frame 23 here, at a third of the
    pixels), and from frame 25 on the prediction has no hit, the tracker no pair and the fusion no voxel, for good;
    (iii) per frame the pose error against the
    true twists exceeds that of the same tracker in a fixed volume holding the whole path by at most MARGIN_T,
    MARGIN_R -- a quarter of a voxel and the angle that moves a point at the anchor's depth by as much: the window
    holds less of the scene than the fixed volume, and a quarter of a voxel is what leaves the fused surface within
    the rounding of one voxel; (iv), (v) the streamed faces add up.
    Measured on an MI355X, largest over the frames: moving window 1.07 mm and 2.9e-3 rad, fixed volume 0.99 mm and
    3.7e-3 rad; the largest excess of a frame is 0.19 mm in translation and none in rotation
    (profiles/moving_volume_cost.md has the run's own figures)."""
    depth, _ = _frames(MS.FRAMES)
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR)
    seq = lsf.SequenceFusion3d(_camera(), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="icp", moving_volume=policy)
    for d in depth:
        rec = seq.integrate(d)
        assert isinstance(rec["shift"], tuple) and len(rec["shift"]) == 3 and "streamed_faces" in rec
    records = seq.frame_records
    moved = [r["shift"] for r in records if r["shift"] != (0, 0, 0)]
    assert len(moved) >= 2 and records[-1]["fusion"]["fused"] > 0 and records[-1]["prediction_hits"] > 0  # (i)
    assert np.array_equal(seq.initial_array_offset, MS.WINDOW_OFFSET)
    assert np.array_equal(seq.array_offset, MS.WINDOW_OFFSET + np.sum([r["shift"] for r in records], axis=0))
    assert seq.array_offset[0] - MS.WINDOW_OFFSET[0] > MS.WINDOW  # it ended outside the first box
    small = _fixed_run(False)
    last = small.frame_records[-1]
    assert last["prediction_hits"] == 0 or last["fusion"]["fused"] == 0  # (ii)
    assert set(last) == {"frame", "twist", "rigid_records", "nonrigid", "fusion", "prediction_hits"}
    assert small.streamed_meshes == []
    fixed = _fixed_run(True)
    (mt, mr), (ft, fr) = _pose_errors(seq.twists), _pose_errors(fixed.twists)
    with capsys.disabled():
        print("\nmoving volume, |twist - truth| largest over the frames: moving %.6f m %.6f rad, fixed %.6f m %.6f rad"
              % (mt.max(), mr.max(), ft.max(), fr.max()))
        print("per frame, moving - fixed:\n", np.array2string(np.stack([mt - ft, mr - fr]), precision=6))
    assert np.all(mt <= ft + MARGIN_T) and np.all(mr <= fr + MARGIN_R), (mt - ft, mr - fr)  # (iii)
    window = seq.extract_mesh()
    merged = seq.extract_mesh(include_streamed=True)
    assert len(seq.streamed_meshes) >= 2 and len(window[1]) > 0
    assert len(merged[1]) == len(window[1]) + sum(len(c[1]) for c in seq.streamed_meshes)  # (iv)
    assert len(merged[0]) == len(window[0]) + sum(len(c[0]) for c in seq.streamed_meshes)
    assert merged[1].max() == len(merged[0]) - 1 or merged[1].max() < len(merged[0])
    assert sum(r["streamed_faces"] for r in records) == sum(len(c[1]) for c in seq.streamed_meshes) > 0  # (v)
    for bad in (dict(normals=True), dict(colours=True), dict(min_weight=1.0), dict(iso=0.1), dict(as_tensor=True)):
        with pytest.raises(ValueError):
            seq.extract_mesh(include_streamed=True, **bad)
    with pytest.raises(ValueError):
        small.extract_mesh(include_streamed=True)


def test_sdf_mode_in_a_moving_volume(lsf):
    """one short run with one shift: it completes, the record keys are there and the pairs stay above zero"""
    depth, _ = _frames(MS.FRAMES)
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR, stream_mesh=False)
    seq = lsf.SequenceFusion3d(_camera(), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="sdf", moving_volume=policy)
    shifted = []
    for k, d in enumerate(depth[:12]):  # until two frames after the first shift
        rec = seq.integrate(d)
        assert {"shift", "streamed_faces", "fusion", "rigid_records"} <= set(rec) and rec["prediction_hits"] is None
        shifted += [k] if rec["shift"] != (0, 0, 0) else []
        if shifted and k == shifted[0] + 2:
            break
    assert len(shifted) == 1 and len(seq.frame_records) == shifted[0] + 3 and seq.streamed_meshes == []
    assert all(r["streamed_faces"] == 0 for r in seq.frame_records)
    for r in seq.frame_records[shifted[0] + 1:]:
        assert r["rigid_records"] and all(x["count"] > 0 for x in r["rigid_records"]) and r["fusion"]["fused"] > 0
