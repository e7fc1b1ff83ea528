"""GPU checks of the moving volume's brick store: lsf_volume_bricks_count / _gather / _scatter
(csrc/lsf_volume_bricks.hip) against the numpy restatement (tests/volume_bricks_restatement.py) bit for bit as uint32,
CanonicalVolume.shift(brick_store=) there and back, a window wandering through a dense numpy world, assemble, and a
SequenceFusion3d whose camera leaves and returns (the trajectory of tests/test_volume_bricks_host.py).
The kernels' unit of work is a brick per wave, LSF_VOLUME_BRICKS_BLOCK_BRICKS per workgroup.  (33, 34, 70) has whole
interior bricks, bricks cut by every face of the window and x-rows that take the 16-byte path; (3, 4, 67) is all
cut bricks; (2, 2, 2) sits inside one brick or, at g = (-3, 5, 13), across two."""
import functools

import numpy as np
import pytest
import torch

import moving_volume_scene as MS
import volume_bricks_restatement as B
from test_volume_bricks_host import RETURN_K, frames_since_overlap_began, return_twists, shared_voxels, window_trail
from test_volume_bricks_host import inputs as _inputs
from test_volume_bricks_host import random_bricks as _random_bricks
from test_volume_bricks_host import shifts as _shifts
from test_volume_shift_host import _special_volume

pytestmark = pytest.mark.gpu

VOLUMES = ((2, 2, 2), (5, 7, 9), (3, 4, 67), (33, 34, 70))  # (Z, Y, X)
ORIGINS = ((0, 0, 0), (-3, 5, 13), (-8, 16, -9))            # g = (gx, gy, gz)
GARBAGE = 0x5a5a5a5a  # what the outputs hold before a call: every word must be written


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _garbage(shape, dtype=torch.float32):
    t = torch.full(tuple(shape), GARBAGE, dtype=torch.int32, device="cuda")
    if dtype == torch.int32:
        return t
    if dtype == torch.uint8:
        return torch.full(tuple(shape), 0x5a, dtype=torch.uint8, device="cuda")
    if dtype == torch.int64:
        return torch.full(tuple(shape), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    return t.view(torch.float32)


def _count(D, dw, shape, g, s):
    nb = int(np.prod(D.brick_grid(shape, g)[1]))
    flags, offsets = _garbage((nb,), torch.int32), _garbage((nb,), torch.int32)
    total = _garbage((1,), torch.int64)
    D.count(dw, flags, offsets, total, g, s)
    return flags, offsets, total


@pytest.mark.parametrize("with_colour", [False, True])
@pytest.mark.parametrize("shape", VOLUMES)
def test_count_and_gather_against_restatement(lsf, shape, with_colour):
    rows, touched_unflagged = count_and_gather_against_restatement(shape, ORIGINS, _shifts(shape), with_colour)
    assert rows > 0
    if shape == VOLUMES[-1]:
        assert touched_unflagged > 0  # the blobs: bricks that a shift touches and that hold no data there


def count_and_gather_against_restatement(shape, origins, shifts, with_colour):
    """lsf_volume_bricks_count and _gather over _inputs(shape) at every origin and shift, outputs that start as
    garbage, against B.count and B.gather; returns (the rows gathered, the touched bricks left unflagged) over all"""
    from levelsetfusion_python_amd import device_volume_bricks as D
    t, w, c = _inputs(shape)
    c = c if with_colour else None
    dt, dw, dc = _dev(t), _dev(w), _dev(c)
    rows = touched_unflagged = 0
    for g in origins:
        coords_all = B.grid_coords(shape, g)
        for s in shifts:
            flags, offsets, total = _count(D, dw, shape, g, s)
            want_flags, want_offsets, want_total = B.count(w, g, s)
            assert np.array_equal(flags.cpu().numpy(), want_flags), (g, s)
            assert np.array_equal(offsets.cpu().numpy(), want_offsets), (g, s)
            k = int(total.item())
            assert k == want_total, (g, s)
            cube = (k, 8, 8, 8)
            out = (_garbage((k, 3), torch.int32), _garbage(cube), _garbage(cube),
                   _garbage(cube + (4,)) if with_colour else None, _garbage((k, 64), torch.uint8))
            D.gather(dt, dw, dc, flags, offsets, k, *out, g, s)
            want = B.gather(t, w, c, g, s)
            assert np.array_equal(out[0].cpu().numpy(), want[0]), (g, s)
            assert np.array_equal(_u32(out[1]), want[1]) and np.array_equal(_u32(out[2]), want[2]), (g, s)
            if with_colour:
                assert np.array_equal(_u32(out[3]), want[3]), (g, s)
            assert np.array_equal(out[4].cpu().numpy(), want[4]), (g, s)
            rows += k
            touched = D.leaving_mask(shape, g, s, coords_all).reshape(len(coords_all), -1).any(axis=1)
            touched_unflagged += int(np.sum(touched & (want_flags == 0)))
    for dev, host in ((dt, t), (dw, w)) + (((dc, c),) if with_colour else ()):
        assert np.array_equal(_u32(dev), host.view(np.uint32))  # read only
    return rows, touched_unflagged


def scatter_against_restatement(bricks, dev_bricks, shape, g, shifts, with_colour):
    """lsf_volume_bricks_scatter of the host rows `bricks` (dev_bricks: their device copies) into fresh copies of
    _inputs(shape) under every shift, against B.scatter"""
    from levelsetfusion_python_amd import device_volume_bricks as D
    t, w, c = _inputs(shape)
    c = c if with_colour else None
    for s in shifts:
        dt, dw, dc = _dev(t), _dev(w), _dev(c)  # what the contract does not name keeps these bits
        D.scatter(*dev_bricks, dt, dw, dc, g, s)
        want = B.scatter(*bricks, t, w, c, g, s)
        assert np.array_equal(_u32(dt), want[0]) and np.array_equal(_u32(dw), want[1]), (g, s)
        if with_colour:
            assert np.array_equal(_u32(dc), want[2]), (g, s)
        changed = _u32(dt) != t.view(np.uint32)
        assert not np.any(changed & ~B.entering(shape, s))


@pytest.mark.parametrize("with_colour", [False, True])
@pytest.mark.parametrize("shape", VOLUMES)
def test_scatter_against_restatement(lsf, shape, with_colour):
    from levelsetfusion_python_amd import device_volume_bricks as D
    rng = np.random.default_rng(17)
    for g in ORIGINS:
        bricks = _random_bricks(shape, g, rng, with_colour)
        dev_bricks = tuple(_dev(a) for a in bricks)
        scatter_against_restatement(bricks, dev_bricks, shape, g, _shifts(shape), with_colour)
        # all entering: a dense volume assembled from bricks equals the store's to_volume of the box
        store = lsf.fusion.BrickStore(colour=with_colour)
        store.merge(*bricks)
        dt = torch.ones(shape, dtype=torch.float32, device="cuda")
        dw = torch.zeros(shape, dtype=torch.float32, device="cuda")
        dc = torch.zeros(shape + (4,), dtype=torch.float32, device="cuda") if with_colour else None
        D.scatter(*dev_bricks, dt, dw, dc, g, (shape[2], 0, 0))
        want = store.to_volume(g, tuple(a + n for a, n in zip(g, shape[::-1])))
        for got, a in zip((dt, dw, dc), want):
            assert np.array_equal(_u32(got), a.view(np.uint32)), g
    for dev, host in zip(dev_bricks[1:3], bricks[1:3]):
        assert np.array_equal(_u32(dev), host.view(np.uint32))  # read only


def test_wrapper_refusals(lsf):
    from levelsetfusion_python_amd import device_volume_bricks as D
    shape, g, s = (5, 7, 9), (-3, 5, 13), (1, 0, 0)
    new = lambda *extra: torch.zeros(shape + extra, dtype=torch.float32, device="cuda")
    t, w = new(), new()
    nb = int(np.prod(D.brick_grid(shape, g)[1]))
    flags, offsets = torch.zeros(nb, dtype=torch.int32, device="cuda"), torch.zeros(nb, dtype=torch.int32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    D.count(w, flags, offsets, total, g, s)
    for bad in ((w, flags, flags, total), (w, flags[:-1], offsets, total), (w, flags.long(), offsets, total),
                (w, flags, offsets, total.int()), (w.cpu(), flags, offsets, total), (w, flags.cpu(), offsets, total),
                (w[0], flags, offsets, total)):
        with pytest.raises((ValueError, TypeError)):
            D.count(*bad, g, s)
    with pytest.raises(ValueError):
        D.count(w, flags, offsets, total, (0.5, 0, 0), s)
    rows = lambda k: [torch.zeros((k, 3), dtype=torch.int32, device="cuda"),
                      torch.zeros((k, 8, 8, 8), dtype=torch.float32, device="cuda"),
                      torch.zeros((k, 8, 8, 8), dtype=torch.float32, device="cuda"), None,
                      torch.zeros((k, 64), dtype=torch.uint8, device="cuda")]
    D.gather(t, w, None, flags, offsets, 0, *rows(0), g, s)  # nothing to do, nothing launched
    good = rows(2)
    D.scatter(*good, t, w, None, g, s)
    for i, wrong in ((1, good[1][:1]), (0, good[0].long()), (4, good[4].int()), (1, good[1].cpu())):
        bad = list(good)
        bad[i] = wrong
        with pytest.raises((ValueError, TypeError)):
            D.scatter(*bad, t, w, None, g, s)
    with pytest.raises(ValueError):  # one colour missing
        D.scatter(*good, t, w, new(4), g, s)
    with pytest.raises(ValueError):
        D.gather(t, w, None, flags, offsets, 2, *good[:3], torch.zeros((2, 8, 8, 8, 4), device="cuda"), good[4], g, s)
    with pytest.raises(ValueError):  # more rows than the grid has bricks
        D.gather(t, w, None, flags, offsets, nb + 1, *rows(nb + 1), g, s)
    big, big_w = (torch.zeros((16, 16, 16), dtype=torch.float32, device="cuda") for _ in range(2))
    D.scatter(*good, big, big_w, None, (0, 0, 0), s)
    with pytest.raises(ValueError):  # the window's own buffer as a brick row
        D.scatter(good[0], big.view(-1)[:1024].view(2, 8, 8, 8), good[2], None, good[4], big, big_w, None, (0, 0, 0), s)
    torch.cuda.synchronize()


# ---- CanonicalVolume.shift(brick_store=) --------------------------------------------------------------------------------

def _filled_volume(lsf, shape, colour=True):
    t, w, c = _inputs(shape)
    vol = lsf.fusion.CanonicalVolume(shape, colour=colour)
    for dst, a in ((vol.tsdf, t), (vol.weight, w)) + (((vol.colour, c),) if colour else ()):
        dst.copy_(torch.from_numpy(np.array(a)))
    return vol


@pytest.mark.parametrize("shift", [(2, -3, 1), (0, 40, 0)])
def test_round_trip(lsf, shift):
    vol, store, off = round_trip(lsf, VOLUMES[-1], shift)
    # refusals with a device
    with pytest.raises(ValueError):
        vol.shift((1, 0, 0), off + [0.5, 0, 0], brick_store=store)
    with pytest.raises(ValueError):
        vol.shift((1, 0, 0), off, brick_store=lsf.fusion.BrickStore())
    with pytest.raises(ValueError):
        lsf.fusion.CanonicalVolume((8, 8)).shift((1, 0), [0, 0, 0], brick_store=store)


def round_trip(lsf, shape, shift, g=(0, 0, 0)):
    """_inputs(shape) out of a window at lattice origin g by `shift` and back through CanonicalVolume.shift(brick_store=):
    the store's counts, every data voxel back bit for bit, every other voxel that left empty; and the same pair of
    shifts without a store, which loses what left.  Returns (the volume, the store, the window's array_offset)"""
    t, w, c = _inputs(shape)
    data = B.holds_data(w)
    off = np.array([1.5, -2.0, 3.25])
    back = tuple(-v for v in shift)
    vol, store = _filled_volume(lsf, shape), lsf.fusion.BrickStore(colour=True)
    if g != (0, 0, 0):  # a lattice fixed earlier, elsewhere: the window lies at g in it
        assert store.lattice_origin(off - g) == (0, 0, 0) and store.lattice_origin(off) == tuple(g)
    off1, chunks = vol.shift(shift, off, brick_store=store)
    assert chunks == [] and np.array_equal(off1, off + shift) and np.array_equal(store.origin, off - g)
    leaving = B.leaving(shape, shift)
    assert store.last == {"bricks_out": len(store), "voxels_out": int((leaving & data).sum()), "bricks_in": 0,
                          "voxels_in": 0}
    assert store.voxel_count == int((leaving & data).sum()) > 0
    workspaces = vol._bricks
    off2, _ = vol.shift(back, off1, brick_store=store)
    assert np.array_equal(off2, off) and vol._bricks is workspaces  # allocated once
    assert store.last["bricks_out"] == 0 and store.last["voxels_in"] == int((leaving & data).sum())
    assert len(store) == 0 and store.voxel_count == 0
    lost = False
    for got, a, empty in zip((vol.tsdf, vol.weight, vol.colour), (t, w, c), B.EMPTY):
        got, a = _u32(got), a.view(np.uint32)
        assert np.array_equal(got[data], a[data])
        assert np.all(got[leaving & ~data] == empty) and np.array_equal(got[~leaving], a[~leaving])
    # the same pair of shifts without a store: what left is gone
    plain = _filled_volume(lsf, shape)
    plain.shift(back, plain.shift(shift, off)[0])
    for got, a, empty in zip((plain.tsdf, plain.weight, plain.colour), (t, w, c), B.EMPTY):
        got, a = _u32(got), a.view(np.uint32)
        assert np.all(got[leaving] == empty) and np.array_equal(got[~leaving], a[~leaving])
        lost |= bool(np.any(got[leaving & data] != a[leaving & data]))
    assert lost
    return vol, store, off


def test_a_wandering_window_against_a_dense_world(lsf):
    n_world, shape = 64, (24, 20, 28)  # the world is lattice [-32, 32)^3; the window (Z, Y, X)
    n = np.array(shape[::-1])
    rng = np.random.default_rng(23)
    world = [np.full((n_world,) * 3, B.EMPTY[0], np.uint32), np.zeros((n_world,) * 3, np.uint32),
             np.zeros((n_world,) * 3 + (4,), np.uint32)]
    origin = np.array([0.5, -0.25, 2.0])
    pos = np.array([10, 12, 8])  # the window's first voxel in the world array, (x, y, z)
    vol, store = lsf.fusion.CanonicalVolume(shape, colour=True), lsf.fusion.BrickStore(colour=True)
    assert store.lattice_origin(origin) == (0, 0, 0)
    off = origin + (pos - 32)
    # a brick partly out, further out, partly back; all of z out and back; all of x out
    steps = ((3, 0, 0), (4, 0, 0), (-5, 0, 0), (0, -7, 2), (9, 9, 9), (-12, -3, -10), (0, 0, 30), (0, 0, -30),
             (14, 20, 0), (-23, 0, 5), (30, -10, -3), (-15, 5, 7))
    part = lambda p: (slice(p[2], p[2] + shape[0]), slice(p[1], p[1] + shape[1]), slice(p[0], p[0] + shape[2]))
    seen_in = seen_out = 0
    for s in steps:
        # random records with weight > 0 into random window voxels, a blob among them, in both copies
        mask = rng.random(shape) < 0.03
        lo = [int(rng.integers(0, m - 6)) for m in shape]
        mask[lo[0]:lo[0] + 6, lo[1]:lo[1] + 6, lo[2]:lo[2] + 6] = True
        values = [_special_volume(shape, rng), (rng.random(shape).astype(np.float32) + 0.5),
                  _special_volume(shape, rng, (4,))]
        for dst, full, v in zip((vol.tsdf, vol.weight, vol.colour), world, values):
            full[part(pos)][mask] = v.view(np.uint32)[mask]
            dst[torch.from_numpy(mask).cuda()] = torch.from_numpy(v).cuda()[torch.from_numpy(mask).cuda()]
        off, _ = vol.shift(s, off, brick_store=store)
        pos = pos + np.array(s)
        assert np.all(pos >= 0) and np.all(pos + n <= n_world)
        seen_out += store.last["voxels_out"]
        seen_in += store.last["voxels_in"]
        for got, full in zip((vol.tsdf, vol.weight, vol.colour), world):
            assert np.array_equal(_u32(got), full[part(pos)]), s  # window == world slice
        outside = np.ones((n_world,) * 3, bool)
        outside[part(pos)] = False
        stored = store.to_volume((-32,) * 3, (32,) * 3)
        for a, full, empty in zip(stored, world, B.EMPTY):
            a = a.view(np.uint32)
            assert np.array_equal(a[outside], full[outside]), s  # to_volume == world outside the window
            assert np.all(a[~outside] == empty), s                # no stored voxel is valid inside the window
        assert store.voxel_count == int((B.holds_data(world[1]) & outside).sum()), s
    assert seen_in > 0 and seen_out > seen_in
    tsdf, weight, colour, box_offset = vol.assemble(store, off)
    lo, hi = store.bounds()
    lo = np.minimum(lo, pos - 32)
    hi = np.maximum(hi, pos - 32 + n)
    assert np.array_equal(box_offset, origin + lo) and tuple(tsdf.shape) == tuple(int(v) for v in (hi - lo)[::-1])
    box = (slice(lo[2] + 32, hi[2] + 32), slice(lo[1] + 32, hi[1] + 32), slice(lo[0] + 32, hi[0] + 32))
    has = np.nonzero(B.holds_data(world[1]))
    assert all(b.start <= i.min() and i.max() < b.stop for b, i in zip(box, has))  # the box holds all the data
    for got, full in zip((tsdf, weight, colour), world):
        assert np.array_equal(_u32(got), full[box])
    with pytest.raises(ValueError):
        vol.assemble(store, off, max_voxels=int(np.prod(hi - lo)) - 1)
    plain = lsf.fusion.CanonicalVolume(shape)  # a store never used and empty: the window alone
    a, b, none, o = plain.assemble(lsf.fusion.BrickStore(), [0.5, 0, 0])
    assert tuple(a.shape) == shape and none is None and np.array_equal(o, [0.5, 0, 0]) and float(b.sum()) == 0


# ---- a sequence that returns ----------------------------------------------------------------------------------------------

def _camera():
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=MS.K), depth_unit_ratio=1.0)


@functools.lru_cache(maxsize=None)
def _return_frames():
    out = [MS.render(MS.true_twist(k)) for k in range(RETURN_K + 1)]
    return out + out[::-1]


def _run(lsf, keep_tsdf):
    policy = lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR, stream_mesh=False, keep_tsdf=keep_tsdf)
    seq = lsf.SequenceFusion3d(_camera(), MS.WINDOW, MS.WINDOW_OFFSET, voxel_size=MS.VOXEL,
                               narrow_band_width_voxels=MS.BAND, tracking_reference="icp", moving_volume=policy)
    for d in _return_frames():
        seq.integrate(d)
    rel, final = window_trail(seq.frame_records, [r["shift"] for r in seq.frame_records])
    R, last_apart = frames_since_overlap_began(rel)
    # what the weight bound rests on: no voxel of the final window was inside the window during the last frame apart
    assert shared_voxels(rel[last_apart] - final) == 0 and shared_voxels(final) * 2 >= MS.WINDOW ** 3
    return seq, R


def test_a_sequence_that_returns(lsf, capsys):
    """with keep_tsdf the voxels of the first position come back with the weight of the first visit; without it the
    window starts from nothing there.  R is the number of frames fused since the window last began to overlap its first
    position; a voxel gains at most 1 per frame, so without a store no weight exceeds R."""
    assert len(return_twists()) == len(_return_frames()) == 2 * RETURN_K + 2
    seq, R = _run(lsf, True)
    records = seq.frame_records
    out = [k for k, r in enumerate(records) if r["bricks_out"] > 0]
    back = [k for k, r in enumerate(records) if r["bricks_in"] > 0]
    assert out and back and back[-1] > out[0]
    assert isinstance(seq.brick_store, lsf.fusion.BrickStore) and not seq.brick_store.colour
    above = int((seq.canonical.weight > R).sum().item())
    plain, R_plain = _run(lsf, False)
    assert plain.brick_store is None and "bricks_out" not in plain.frame_records[-1]
    above_plain = int((plain.canonical.weight > R_plain).sum().item())
    with capsys.disabled():
        print("\na sequence that returns: R = %d (without a store %d), voxels with weight > R: %d with keep_tsdf, %d "
              "without; %d bricks stored at the end" % (R, R_plain, above, above_plain, len(seq.brick_store)))
    assert above > 0 and above_plain == 0
    # one mesh of the whole map: it reaches beyond the final window on the side the camera came from (+x)
    n = MS.WINDOW
    window_top = (seq.array_offset[0] + n - 1) * MS.VOXEL
    verts, faces = seq.extract_mesh(include_streamed=True)
    window_verts, window_faces = seq.extract_mesh()
    assert len(faces) > len(window_faces) > 0 and faces.max() < len(verts)
    assert window_verts[:, 0].max() <= window_top + 1e-6 < verts[:, 0].max() - 8 * MS.VOXEL
    tv, tf, tn = seq.extract_mesh(include_streamed=True, normals=True, as_tensor=True, min_weight=1.0, iso=0.05)
    assert tv.is_cuda and tn.shape == tv.shape and 0 < len(tf) and tf.dtype == torch.int32
    with pytest.raises(ValueError):
        seq.extract_mesh(include_streamed=True, colours=True)  # the sequence has no colour
    with pytest.raises(ValueError):
        lsf.fusion.MovingVolume(MS.THRESHOLD, MS.ANCHOR, stream_mesh=True, keep_tsdf=True)
    with pytest.raises(ValueError):
        plain.extract_mesh(include_streamed=True)  # nothing was streamed and nothing kept
