"""Host checks of the moving volume's brick store (no GPU): the lattice arithmetic for negative origins, the restated
gather and scatter as inverses of each other, fusion.BrickStore's merge / clear / to_volume rules against the restated
store (with the restated kernels in place of the card), the refusals that need no device, the header's macros, and the
out-and-back trajectory tests/test_gpu_volume_bricks.py fuses: the window leaves its first position completely and
returns onto most of it.  Also the inputs the GPU tests share, and the window of 8450 bricks that
tests/test_gpu_second_trip.py takes past the kernels' capped grids: that it crosses them, with flagged bricks and changed
words past the cap, is asserted here from constants and the restatement."""
import functools
import itertools
import os

import numpy as np
import pytest

import moving_volume_scene as MS
import volume_bricks_restatement as B
import volume_shift_restatement as V
from test_volume_shift_host import _special_volume


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def blobby_weights(shape, rng, a, largest=6):
    """`a` with about half of its voxels zeroed in blobs (boxes of up to `largest` voxels a side), so that whole bricks
    a shift touches hold no data; returns a copy"""
    a = a.copy()
    zero = np.zeros(shape, bool)
    zeroed = 0  # zero.sum(), kept along: the mean of a large volume is not taken once per blob
    while zeroed / zero.size < 0.5:
        lo = [int(rng.integers(0, n)) for n in shape]
        hi = [min(n, l + int(rng.integers(1, largest + 1))) for n, l in zip(shape, lo)]
        box = zero[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        zeroed += box.size - int(box.sum())
        box[...] = True
    a[zero] = 0.0
    return a


def shifts(shape):
    """(sx, sy, sz): one per sign and axis, a diagonal, and one that makes everything leave"""
    return [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2, -3, 1), (0, -(shape[1] + 5), 1)]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """tsdf, weight, colour with NaN payloads, +-inf and -0.0; about half of the weights zero in blobs"""
    rng = np.random.default_rng(sum(shape) + 1)
    arrays = (_special_volume(shape, rng),
              blobby_weights(shape, rng, _special_volume(shape, rng), largest=max(6, min(shape) // 2 + 1)),
              _special_volume(shape, rng, (4,)))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def random_bricks(shape, g, rng, with_colour):
    """a brick for every brick of the window's grid and two outside it, in a shuffled order: special values, random
    validity bytes, some rows wholly valid"""
    coords = B.grid_coords(shape, g)
    outside = np.array([coords.min(axis=0) - 1, coords.max(axis=0) + [1, 0, 0]], np.int32)
    coords = rng.permutation(np.concatenate([coords, outside]))
    k = len(coords)
    valid = rng.integers(0, 256, (k, 64)).astype(np.uint8)
    valid[rng.random((k, 64)) < 0.4] = 255
    valid[rng.random((k, 64)) < 0.1] = 0
    return (coords, _special_volume((k, 8, 8, 8), rng), _special_volume((k, 8, 8, 8), rng),
            _special_volume((k, 8, 8, 8), rng, (4,)) if with_colour else None, valid)


# ---- a window of more bricks than the capped grids have waves --------------------------------------------------------------
# tests/test_gpu_second_trip.py runs the brick kernels on this window; what it assumes -- which cap the grid crosses, and
# that work with a visible effect lies past it -- is checked here without a card.  The constants mirror
# csrc/lsf_volume_bricks.hip.

BRICKS_MAX_BLOCKS = 2048    # LSF_VOLUME_BRICKS_MAX_BLOCKS (include/lsf_hip.h)
BRICKS_BLOCK_BRICKS = 4     # LSF_VOLUME_BRICKS_BLOCK_BRICKS: a wave per brick, or per row of a scatter
BRICKS_WAVES = BRICKS_MAX_BLOCKS * BRICKS_BLOCK_BRICKS  # bricks, or rows, of a capped grid's first trip
SCAN_BLOCK, SCAN_ITEMS = 1024, 8  # kScanBlock, kScanItems: the one-workgroup scan takes 8192 flags per trip
SCAN_TRIP = SCAN_BLOCK * SCAN_ITEMS
BIG_SHAPE, BIG_ORIGIN = (2, 515, 515), (-3, 5, 7)  # (Z, Y, X), g: a 65 x 65 x 2 grid
# an x-shift; a y-shift whose leaving rows end in the bricks of the grid's last y rows, the topmost of them with a single
# leaving row; a diagonal that makes the whole first z layer leave; the shift that makes everything leave
BIG_SHIFTS = ((1, 0, 0), (0, -25, 0), (2, -3, 1), (0, -(BIG_SHAPE[1] + 5), 1))
BIG_Y_SHIFT, BIG_ALL_SHIFT = BIG_SHIFTS[1], BIG_SHIFTS[3]


def touched_bricks(shape, g, s):
    """bool [nbricks]: the bricks that hold a voxel inside the window that leaves under s, data or not"""
    return B._cut(B._pad(B.leaving(shape, s), shape, g, False)).reshape(-1, B.BRICK ** 3).any(axis=1)


@functools.lru_cache(maxsize=None)
def big_window_counts():
    """per shift of BIG_SHIFTS the restated (flags, offsets, total) of inputs(BIG_SHAPE), after the assertions of the
    crossing: the grid against the capped launch and the scan's trip, and flagged bricks past both"""
    first, counts = B.brick_grid(BIG_SHAPE, BIG_ORIGIN)
    nbricks = int(np.prod(counts))
    assert counts == (65, 65, 2) and nbricks == 8450 and int(np.prod(BIG_SHAPE)) == 530450
    assert BRICKS_WAVES == SCAN_TRIP == 8192 < nbricks  # the flag and gather kernels' stride, the scan's second trip
    # every brick is cut by a face of the window or is one of its two one-voxel z layers: none is whole
    assert BIG_SHAPE[0] == 2 and BIG_ORIGIN[2] % B.BRICK == B.BRICK - 1 and counts[2] == 2
    # the scan's second trip: whole threads, one partial thread, idle ones
    rest = nbricks - SCAN_TRIP
    assert rest // SCAN_ITEMS == 32 and rest % SCAN_ITEMS == 2 and -(-rest // SCAN_ITEMS) < SCAN_BLOCK
    w = inputs(BIG_SHAPE)[1]
    out = {}
    for s in BIG_SHIFTS:
        flags, offsets, total = B.count(w, BIG_ORIGIN, s)
        touched = touched_bricks(BIG_SHAPE, BIG_ORIGIN, s)
        assert np.all(touched[flags == 1])
        out[s] = (flags, offsets, total)
    flags, offsets, total = out[BIG_Y_SHIFT]
    touched = touched_bricks(BIG_SHAPE, BIG_ORIGIN, BIG_Y_SHIFT)
    # flagged bricks past the cap, and, the blobs, touched bricks without data there
    assert flags[BRICKS_WAVES:].sum() >= 100 and np.any(touched[BRICKS_WAVES:] & (flags[BRICKS_WAVES:] == 0))
    assert offsets[BRICKS_WAVES] == flags[:BRICKS_WAVES].sum() > 0  # what the scan carries into its second trip
    flags, offsets, total = out[BIG_ALL_SHIFT]
    assert np.all(touched_bricks(BIG_SHAPE, BIG_ORIGIN, BIG_ALL_SHIFT))
    assert BRICKS_WAVES < total < nbricks  # gather writes slots >= 8192; the blobs leave some bricks without data
    assert flags[SCAN_TRIP:].sum() > 200 and offsets[SCAN_TRIP] > 8000  # a dropped carry restarts these from 0
    for s in (BIG_SHIFTS[0], BIG_SHIFTS[2]):
        assert out[s][0][BRICKS_WAVES:].sum() > 0 and 0 < out[s][0][:BRICKS_WAVES].sum() < BRICKS_WAVES
    return out


@functools.lru_cache(maxsize=None)
def big_window_bricks(with_colour):
    """random_bricks for the big window's grid: more rows than the scatter kernel's capped grid has waves"""
    bricks = random_bricks(BIG_SHAPE, BIG_ORIGIN, np.random.default_rng(29), with_colour)
    assert len(bricks[0]) == 8452 > BRICKS_WAVES
    for a in bricks:
        if a is not None:
            a.setflags(write=False)
    return bricks


def test_the_big_window_crosses_the_caps(lsf):
    """what tests/test_gpu_second_trip.py assumes about the big window, from constants and the restatement"""
    L = lsf._lib
    assert (BRICKS_MAX_BLOCKS, BRICKS_BLOCK_BRICKS) == (L.VOLUME_BRICKS_MAX_BLOCKS, L.VOLUME_BRICKS_BLOCK_BRICKS)
    source = open(os.path.join(os.path.dirname(lsf._build.ABI_HEADER), "..", "levelsetfusion-python_amd", "csrc",
                               "lsf_volume_bricks.hip")).read()
    assert "constexpr int kScanBlock = %d;" % SCAN_BLOCK in source and "constexpr int kScanItems = %d;" % SCAN_ITEMS in source
    big_window_counts()
    # the scatter's rows past the cap: under the shifts that make a z layer or everything enter they change more than
    # 1000 words, so a stride that stops short of them fails
    t, w, _ = inputs(BIG_SHAPE)
    bricks = big_window_bricks(False)
    first_trip = tuple(a if a is None else a[:BRICKS_WAVES] for a in bricks)
    for s in BIG_SHIFTS[2:]:
        whole, part = B.scatter(*bricks, t, w, None, BIG_ORIGIN, s), B.scatter(*first_trip, t, w, None, BIG_ORIGIN, s)
        assert int((whole[0] != part[0]).sum() + (whole[1] != part[1]).sum()) > 1000, s


def test_lattice_arithmetic_for_negative_origins(lsf):
    from levelsetfusion_python_amd import device_volume_bricks as D
    # floor, not truncation: voxel v of a window at g is lattice voxel g + v, in brick floor((g + v) / 8), place mod 8
    for a, brick, place in ((-3, -1, 5), (-8, -1, 0), (-9, -2, 7), (-1, -1, 7), (0, 0, 0), (7, 0, 7), (8, 1, 0),
                            (-16, -2, 0), (-17, -3, 7)):
        assert B.floor_div(a) == brick and a - 8 * brick == place and 0 <= place < 8
    # a window of 4 voxels at g = -3 covers lattice -3 .. 0: bricks -1 and 0; at -8: -8 .. -5, brick -1 alone; at -9:
    # -9 .. -6: bricks -2 and -1.  (Z, Y, X) = (4, 4, 4), the same g on every axis
    for g, first, count in ((-3, -1, 2), (-8, -1, 1), (-9, -2, 2), (0, 0, 1), (5, 0, 2), (13, 1, 2)):
        want = ((first,) * 3, (count,) * 3)
        assert B.brick_grid((4, 4, 4), (g,) * 3) == want == D.brick_grid((4, 4, 4), (g,) * 3)
    shape, g = (4, 5, 6), (-3, 5, 13)
    # x: -3 .. 2, bricks -1, 0; y: 5 .. 9, bricks 0, 1; z: 13 .. 16, bricks 1, 2
    assert B.brick_grid(shape, g) == ((-1, 0, 1), (2, 2, 2)) == D.brick_grid(shape, g)
    assert np.array_equal(D.grid_coords(shape, g), B.grid_coords(shape, g))
    assert B.grid_coords(shape, g).tolist() == [[-1, 0, 1], [0, 0, 1], [-1, 1, 1], [0, 1, 1],
                                                [-1, 0, 2], [0, 0, 2], [-1, 1, 2], [0, 1, 2]]
    rng = np.random.default_rng(0)
    mask = rng.random((3, 8, 8, 8)) < 0.5
    assert np.array_equal(D.pack_valid(mask), B.pack_valid(mask))
    assert np.array_equal(D.unpack_valid(B.pack_valid(mask)), mask) and np.array_equal(B.unpack_valid(D.pack_valid(mask)), mask)
    one = np.zeros((1, 8, 8, 8), bool)
    one[0, 2, 3, 5] = True  # zl 2, yl 3, xl 5: byte 19, bit 5
    assert D.pack_valid(one)[0, 19] == 32 and D.pack_valid(one).sum() == 32


def test_restated_gather_then_scatter_is_the_identity_on_data(lsf):
    from levelsetfusion_python_amd import device_volume_bricks as D
    shape, g = (4, 5, 6), (-3, 5, 13)
    rng = np.random.default_rng(11)
    tsdf, colour = _special_volume(shape, rng), _special_volume(shape, rng, (4,))
    weight = blobby_weights(shape, rng, _special_volume(shape, rng))
    data = B.holds_data(weight)
    assert 0 < data.sum() < data.size
    per_axis = lambda n: (0, 1, -1, 2, -2, n - 1, -(n - 1), n, -(n + 5))
    coords_all = B.grid_coords(shape, g)
    unflagged_touched = False
    for s in itertools.product(per_axis(6), per_axis(5), per_axis(4)):
        leaving = B.leaving(shape, s)
        assert np.array_equal(leaving, B.entering(shape, tuple(-v for v in s)))  # what -s copies nothing into
        # a voxel leaves when the shifted copy holds it nowhere: mark every voxel and look for the marks
        marks = np.arange(1, leaving.size + 1, dtype=np.uint32).reshape(shape)
        assert np.array_equal(leaving, ~np.isin(marks, V.shift_array(marks, s, np.uint32(0)).view(np.uint32)))
        flags, offsets, total = B.count(weight, g, s)
        coords, bt, bw, bc, valid = B.gather(tsdf, weight, colour, g, s)
        assert len(coords) == total and np.array_equal(coords, coords_all[flags == 1])
        assert np.array_equal(offsets[flags == 1], np.arange(total))
        # the flagged bricks are exactly those that hold a leaving voxel with data: by the lattice rule, voxel by voxel
        held = set()
        for z, y, x in zip(*np.nonzero(leaving & data)):
            held.add((B.floor_div(g[0] + x), B.floor_div(g[1] + y), B.floor_div(g[2] + z)))
        assert held == set(map(tuple, coords.tolist())), s
        assert int(B.unpack_valid(valid).sum()) == int((leaving & data).sum())
        touched = D.leaving_mask(shape, g, s, coords_all).reshape(len(coords_all), -1).any(axis=1)
        assert np.all(touched[flags == 1])
        unflagged_touched |= bool(np.any(touched & (flags == 0)))
        assert np.array_equal(D.entering_bricks(shape, g, tuple(-v for v in s)), coords_all[touched])
        # the shifted window, then the opposite shift: what left re-enters; the scatter puts it back
        moved = V.shift_model(tsdf, weight, colour, s)
        back = V.shift_model(*moved, tuple(-v for v in s))
        # after shift -s the window is at g again; the voxels that entered under -s are the ones that left under s
        got = B.scatter(coords, bt, bw, bc, valid, *back, g, tuple(-v for v in s))
        for a, b, empty in zip(got, (tsdf, weight, colour), B.EMPTY):
            a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a[data], b[data]), s
            assert np.all(a[leaving & ~data] == empty), s      # left without data: back as the empty voxel
            assert np.array_equal(a[~leaving], b[~leaving]), s   # never left
    assert unflagged_touched  # the blobs leave some touched bricks without data


def _restated_shift(window, g, s, store, restated):
    """one shift with a store, the card's part by the restatement: `store` is the package's BrickStore, `restated` the
    restated one; returns the new window and g"""
    from levelsetfusion_python_amd import device_volume_bricks as D
    tsdf, weight, colour = window
    shape = weight.shape
    rows = B.gather(tsdf, weight, colour, g, s)
    store.merge(*rows)
    restated.merge(*rows)
    moved = V.shift_model(tsdf, weight, colour, s)
    g2 = tuple(a + b for a, b in zip(g, s))
    coords, bt, bw, bc, valid = store.lookup(D.entering_bricks(shape, g2, s))
    # the one-pass lookup CanonicalVolume.shift uses finds the same bricks with the same contents
    one_pass = store.lookup_entering(*D.entering_flags(shape, g2, s))
    order = [one_pass[0].tolist().index(c) for c in coords.tolist()]
    assert len(one_pass[0]) == len(coords)
    for a, b in zip(one_pass, (coords, bt, bw, bc, valid)):
        assert np.array_equal(a[order].view(np.uint8), b.view(np.uint8))
    taken = D.entering_mask(shape, g2, s, coords) & D.unpack_valid(valid)
    # the restated side: the entering voxels that are valid, brick by brick, from the restated rule
    want_taken = B._cut(B._pad(B.entering(shape, s), shape, g2, False))
    index = {tuple(c): i for i, c in enumerate(B.grid_coords(shape, g2).tolist())}
    for c, m, v in zip(coords.tolist(), taken, B.unpack_valid(valid)):
        assert np.array_equal(m, want_taken[index[tuple(c)]] & v)
    new = B.scatter(coords, bt, bw, bc, valid, *moved, g2, s)
    store.clear_valid(coords, taken)
    restated.clear([c for c in coords.tolist()], list(taken))
    return tuple(a.view(np.float32) for a in new), g2


def test_brick_store_semantics_with_the_restatement_for_the_card(lsf):
    BrickStore = lsf.fusion.BrickStore
    shape = (9, 10, 11)
    rng = np.random.default_rng(5)
    world_lo, world_hi = (-24, -24, -24), (40, 40, 40)
    store, restated = BrickStore(colour=True), B.Store(colour=True)
    assert len(store) == 0 and store.bounds() is None and store.voxel_count == 0 and store.nbytes == 0
    assert store.coords().shape == (0, 3) and store.coords().dtype == np.int32
    assert store.lattice_origin([0.25, -1.5, 3.0]) == (0, 0, 0) and np.array_equal(store.origin, [0.25, -1.5, 3.0])
    assert store.lattice_origin([-2.75, 3.5, 16.0]) == (-3, 5, 13)
    window = (_special_volume(shape, rng), blobby_weights(shape, rng, _special_volume(shape, rng)),
              _special_volume(shape, rng, (4,)))
    start = tuple(a.copy() for a in window)
    g = (-3, 5, 13)
    # out partially, further, back in part, back entirely; a brick is merged into twice (overwrite + OR) on the way
    trail = ((3, 0, 0), (2, -1, 0), (-4, 0, 0), (-1, 1, 0), (0, 0, -5), (0, 0, 5), (20, 0, 0), (-20, 0, 0))
    seen_partial = seen_drop = False
    for s in trail:
        before = len(store)
        window, g = _restated_shift(window, g, s, store, restated)
        assert np.array_equal(store.coords(), restated.coords()) and store.voxel_count == restated.voxel_count()
        c = store.coords()
        assert np.array_equal(c, c[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))])  # ascending (z, y, x)
        got, want = store.to_volume(world_lo, world_hi), restated.to_volume(world_lo, world_hi)
        for a, b in zip(got, want):
            assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b)
        # the contract: nothing inside the window is valid in the store
        inside = store.to_volume(g, tuple(a + n for a, n in zip(g, shape[::-1])))
        assert np.all(inside[1].view(np.uint32) == 0) and np.all(inside[0] == 1) and np.all(inside[2].view(np.uint32) == 0)
        if len(store):
            lo, hi = store.bounds()
            assert lo == tuple(int(v) for v in c.min(axis=0) * 8) and hi == tuple(int(v) for v in (c.max(axis=0) + 1) * 8)
            assert store.nbytes == len(store) * (12 + 64 + 512 * 24)
        seen_partial |= 0 < store.voxel_count < 512 * len(store)
        seen_drop |= len(store) < before
    assert seen_partial and seen_drop
    # the trail sums to zero: everything with data is back, bit for bit, the rest is empty, the store is empty
    assert g == (-3, 5, 13) and len(store) == 0 and store.bounds() is None
    data = B.holds_data(start[1])
    for a, b, empty in zip(window, start, B.EMPTY):
        assert np.array_equal(a.view(np.uint32)[data], b.view(np.uint32)[data])
        assert np.all(a.view(np.uint32)[~data] == empty)
    # merge: valid voxels overwrite, validity is ORed, the rest of a stored brick stays
    st = BrickStore()
    t1, w1 = np.full((1, 8, 8, 8), 0.5, np.float32), np.full((1, 8, 8, 8), 2.0, np.float32)
    m1, m2 = np.zeros((1, 8, 8, 8), bool), np.zeros((1, 8, 8, 8), bool)
    m1[0, 0, 0, :4], m2[0, 0, 0, 2:6] = True, True
    assert st.merge([[2, -1, 0]], t1, w1, None, B.pack_valid(m1)) == 4
    assert st.merge([[2, -1, 0]], t1 * 0.5, w1 * 2, None, B.pack_valid(m2)) == 4
    assert len(st) == 1 and st.voxel_count == 6 and st.coords().tolist() == [[2, -1, 0]]
    t, w = st.to_volume((16, -8, 0), (24, 0, 8))
    assert t[0, 0].tolist() == [0.5, 0.5, 0.25, 0.25, 0.25, 0.25, 1, 1] and w[0, 0].tolist() == [2, 2, 4, 4, 4, 4, 0, 0]
    assert np.all(t[1:] == 1) and np.all(w[1:] == 0)
    st.clear_valid([[2, -1, 0]], m1)
    assert st.voxel_count == 2 and st.to_volume((16, -8, 0), (24, 0, 8))[1][0, 0].tolist() == [0, 0, 0, 0, 4, 4, 0, 0]
    st.clear_valid([[2, -1, 0]], m2)
    assert len(st) == 0
    st.merge([[2, -1, 0], [-5, 0, 0], [0, 0, -1]], np.repeat(t1, 3, 0), np.repeat(w1, 3, 0), None,
             np.repeat(B.pack_valid(m1), 3, 0))
    assert st.coords().tolist() == [[0, 0, -1], [2, -1, 0], [-5, 0, 0]] and st.bounds() == ((-40, -8, -8), (24, 8, 8))
    assert st.last == {"bricks_out": 0, "voxels_out": 0, "bricks_in": 0, "voxels_in": 0}
    st.clear()
    assert len(st) == 0 and st.voxel_count == 0
    with pytest.raises(ValueError):
        BrickStore(colour=True).merge([[0, 0, 0]], t1, w1, None, B.pack_valid(m1))


def _hostless_volume(lsf, shape, colour):
    """a CanonicalVolume that was never given device buffers: the refusals below come before any of them is touched"""
    vol = object.__new__(lsf.fusion.CanonicalVolume)
    vol.shape, vol.colour, vol.tsdf, vol.weight, vol._spare, vol._bricks = shape, (object() if colour else None), None, \
        None, None, None
    return vol


def test_refusals_that_need_no_device(lsf):
    import ctypes
    from levelsetfusion_python_amd import device_volume_bricks as D
    BrickStore, MV = lsf.fusion.BrickStore, lsf.fusion.MovingVolume
    st = BrickStore()
    vol = _hostless_volume(lsf, (8, 8, 8), colour=False)
    with pytest.raises(ValueError):  # no lattice yet, but not a store
        vol.shift((1, 0, 0), [0, 0, 0], brick_store={})
    with pytest.raises(ValueError):  # colour mismatch, both ways
        vol.shift((1, 0, 0), [0, 0, 0], brick_store=BrickStore(colour=True))
    with pytest.raises(ValueError):
        _hostless_volume(lsf, (8, 8, 8), colour=True).shift((1, 0, 0), [0, 0, 0], brick_store=st)
    assert st.origin is None
    assert st.lattice_origin([0.5, 0.25, -7.0]) == (0, 0, 0)
    for bad in ([1.0, 0.25, -7.0], [0.5, 0.75, -7.0], [0.5, 0.25, -7.5], [0.5 + 1e-9, 0.25, -7.0], [np.nan, 0.25, -7.0]):
        with pytest.raises(ValueError):  # a fractional g
            vol.shift((1, 0, 0), bad, brick_store=st)
        with pytest.raises(ValueError):
            vol.assemble(st, bad)
    assert st.lattice_origin([-3.5, 8.25, -7.0]) == (-4, 8, 0)
    with pytest.raises(ValueError):
        D.origin_of((0.5, 0, 0))
    with pytest.raises(ValueError):
        D.params((8, 8), (0, 0, 0))
    with pytest.raises(ValueError):
        D.params((8, 8, 8), (2 ** 31 - 8, 0, 0))  # |g| + n leaves int32
    with pytest.raises(ValueError):
        D.params((8, 8, 8), (-(2 ** 31 - 8), 0, 0))
    p = D.params((3, 4, 5), (-3, 5, 13), (7, -8, 9))
    assert [getattr(p, n) for n, _ in p._fields_] == [3, 4, 5, -3, 5, 13, 7, -8, 9]
    # assemble: the box of window and store against max_voxels, before a buffer is made
    t1, w1 = np.zeros((1, 8, 8, 8), np.float32), np.ones((1, 8, 8, 8), np.float32)
    st.merge([[40, 0, 0]], t1, w1, None, np.full((1, 64), 255, np.uint8))
    with pytest.raises(ValueError):
        vol.assemble(st, [0.5, 0.25, -7.0], max_voxels=8 * 8 * 328 - 1)  # x from 0 to 328
    with pytest.raises(ValueError):
        vol.assemble(st, [0.5, 0.25, -7.0], max_voxels=1000)
    far = BrickStore()
    far.lattice_origin([0, 0, 0])
    far.merge([[2 ** 20, 2 ** 20, 0]], t1, w1, None, np.full((1, 64), 255, np.uint8))
    with pytest.raises(ValueError):  # beyond int32 whatever max_voxels says
        vol.assemble(far, [0, 0, 0], max_voxels=2 ** 62)
    # the policy
    with pytest.raises(ValueError) as e:
        MV(4.0, (0, 0, 0.5), keep_tsdf=True)  # stream_mesh keeps its default
    assert "stream_mesh=False" in str(e.value)
    with pytest.raises(ValueError):
        MV(4.0, (0, 0, 0.5), stream_mesh=True, keep_tsdf=True)
    assert MV(4.0, (0, 0, 0.5), stream_mesh=False, keep_tsdf=True).keep_tsdf
    assert not MV(4.0, (0, 0, 0.5)).keep_tsdf and MV(4.0, (0, 0, 0.5)).stream_mesh
    # the entry points with NULLs
    L = lsf._lib
    assert L.lib.lsf_volume_bricks_count(None, None, None, None, None, None) == -1
    assert L.lib.lsf_volume_bricks_gather(*([None] * 5), 0, *([None] * 7)) == -1
    assert L.lib.lsf_volume_bricks_scatter(*([None] * 5), 0, *([None] * 5)) == -1
    assert L.lib.lsf_volume_bricks_count(None, None, None, None, ctypes.byref(p), None) == -1
    assert L.lib.lsf_volume_bricks_gather(*([None] * 5), 0, *([None] * 5), ctypes.byref(p), None) == -1
    assert L.lib.lsf_volume_bricks_scatter(*([None] * 5), 0, *([None] * 3), ctypes.byref(p), None) == -1


def test_header_binding_and_sources_agree(lsf):
    header = open(lsf._build.ABI_HEADER).read()
    assert "#define LSF_VOLUME_BRICK %d\n" % lsf._lib.VOLUME_BRICK in header and lsf._lib.VOLUME_BRICK == B.BRICK
    assert "#define LSF_VOLUME_BRICKS_MAX_BLOCKS %d\n" % lsf._lib.VOLUME_BRICKS_MAX_BLOCKS in header
    assert "#define LSF_VOLUME_BRICKS_BLOCK_BRICKS %d\n" % lsf._lib.VOLUME_BRICKS_BLOCK_BRICKS in header
    assert "lsf_volume_bricks.hip" in lsf._build.SOURCES
    for name, args in (("lsf_volume_bricks_count", 6), ("lsf_volume_bricks_gather", 13),
                       ("lsf_volume_bricks_scatter", 11)):
        assert name + "(" in header and len(lsf._lib.PROTOTYPES[name][1]) == args
    assert "BrickStore" in lsf.fusion.__all__ and lsf._lib.ABI_VERSION == 4


# ---- the trajectory of the GPU test: out along x until the window shares no voxel with its first position, and back ----

RETURN_K = 38  # true_twist(k) for k = 0 .. RETURN_K, then RETURN_K .. 0: the smallest K that does what is asserted below


def return_twists(K=RETURN_K):
    return [MS.true_twist(k) for k in list(range(K + 1)) + list(range(K, -1, -1))]


def window_trail(twists, shifts=None):
    """the window's offset DURING each frame, relative to its first (whole voxels), and the one after the last frame;
    the shifts are the policy's under `twists` unless given"""
    off, rel = MS.WINDOW_OFFSET.copy(), []
    for k, twist in enumerate(twists):
        rel.append(np.round(off - MS.WINDOW_OFFSET).astype(int))
        s = V.policy_shift(MS.ANCHOR, MS.THRESHOLD, twist, off, (MS.WINDOW,) * 3, MS.VOXEL) if shifts is None \
            else shifts[k]
        off = off + np.array(s, np.float64)
    return rel, np.round(off - MS.WINDOW_OFFSET).astype(int)


def shared_voxels(rel, n=MS.WINDOW):
    """the voxels a window displaced by rel = (x, y, z) shares with the undisplaced one"""
    return int(np.prod(np.clip(n - np.abs(rel), 0, None)))


def frames_since_overlap_began(rel):
    """R: the frames fused since the window last began to overlap its first position -- those after the last frame
    during which it shared no voxel with it; and that frame"""
    apart = [k for k, r in enumerate(rel) if shared_voxels(r) == 0]
    return len(rel) - 1 - apart[-1], apart[-1]


def test_the_window_leaves_its_first_position_and_returns():
    rel, final = window_trail(return_twists())
    assert len(rel) == 2 * RETURN_K + 2
    apart = [k for k, r in enumerate(rel) if shared_voxels(r) == 0]
    assert apart and apart[0] <= RETURN_K + 1  # it has left completely by the turn (twist K is fused twice)
    assert shared_voxels(final) * 2 >= MS.WINDOW ** 3 and shared_voxels(rel[-1]) * 2 >= MS.WINDOW ** 3
    R, last_apart = frames_since_overlap_began(rel)
    assert 0 < R < RETURN_K
    # every voxel of the final window was outside the window during the last frame apart, so without a store none of
    # them can have been fused into more than R times: the two boxes share nothing
    assert shared_voxels(rel[last_apart] - rel[-1]) == 0
    # a smaller K does not leave the first position
    shorter, _ = window_trail(return_twists(RETURN_K - 1))
    assert all(shared_voxels(r) > 0 for r in shorter)
