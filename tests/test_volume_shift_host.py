"""Host checks of the moving volume (no GPU): the numpy restatement of the shift composes, the leaving-box decomposition
is a partition (restated and the package's), the policy equals hand-computed cases, the arguments that can be refused
without a device are, merge_meshes concatenates, and the analytic scene (tests/moving_volume_scene.py) does what the GPU
tests rely on: the window shifts more than once, ends away from where it began, and a short prefix keeps more voxels
inside every window than one frame's band holds."""
import itertools

import numpy as np
import pytest

import fusion_restatement as F
import moving_volume_scene as MS
import volume_shift_restatement as V


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _special_volume(shape, rng, extra=()):
    """random float32 with two NaN payloads, +-inf and -0.0 planted"""
    a = rng.standard_normal(shape + tuple(extra)).astype(np.float32)
    flat = a.reshape(-1).view(np.uint32)
    specials = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000], np.uint32)
    at = rng.choice(flat.size, size=min(flat.size, 2 * specials.size), replace=False)
    flat[at] = np.resize(specials, at.size)
    return a


def test_the_restated_shift_composes():
    rng = np.random.default_rng(3)
    shape = (5, 7, 9)
    a = _special_volume(shape, rng)
    for s1, s2 in (((1, 0, 0), (2, 0, 0)), ((2, -3, 1), (-1, 1, 1)), ((0, 4, 0), (3, -2, -1)), ((-2, 0, 3), (2, 0, -3))):
        twice = V.shift_array(V.shift_array(a, s1, V.TSDF_FILL), s2, V.TSDF_FILL).view(np.uint32)
        total = tuple(p + q for p, q in zip(s1, s2))
        once = V.shift_array(a, total, V.TSDF_FILL).view(np.uint32)
        # a destination voxel v holds source v + s1 + s2 through both steps when v + s2 and v + s1 + s2 are inside
        both = V.retained_mask(shape, s2) & V.shift_array(V.retained_mask(shape, s1).astype(np.float32), s2,
                                                          np.uint32(0)).astype(bool)
        assert both.any() and np.array_equal(twice[both], once[both])
        assert np.all(twice[~both] == V.TSDF_FILL)
    zero = V.shift_array(a, (0, 0, 0), V.TSDF_FILL)
    assert np.array_equal(zero.view(np.uint32), a.view(np.uint32))
    assert np.all(V.shift_array(a, (9, 0, 0), V.WEIGHT_FILL).view(np.uint32) == 0)


def _cover(shape, boxes):
    count = np.zeros(tuple(n - 1 for n in shape), np.int64)
    for (x0, x1), (y0, y1), (z0, z1) in boxes:
        assert x0 < x1 and y0 < y1 and z0 < z1
        count[z0:z1, y0:y1, x0:x1] += 1
    return count


def test_the_leaving_boxes_are_a_partition_of_the_leaving_cells(lsf):
    from levelsetfusion_python_amd import device_volume_shift as D
    shape = (4, 5, 6)  # Z, Y, X
    per_axis = lambda n: (0, 1, -1, 2, -2, n - 1, -(n - 1), n, -(n + 5))  # one layer retained, and all of it leaving
    seen_three = seen_whole = False
    for s in itertools.product(per_axis(6), per_axis(5), per_axis(4)):
        boxes = V.leaving_boxes(shape, s)
        assert boxes == D.leaving_boxes(shape, s), s
        assert len(boxes) <= 3
        leaving = V.leaving_cell_mask(shape, s)
        count = _cover(shape, boxes)
        assert np.array_equal(count, leaving.astype(np.int64)), s  # disjoint, and with the retained cells every cell once
        if s == (0, 0, 0):
            assert boxes == []
        seen_three |= len(boxes) == 3
        seen_whole |= boxes == [((0, 5), (0, 4), (0, 3))]
    assert seen_three and seen_whole
    assert D.leaving_boxes(shape, (6, 0, 0)) == [((0, 5), (0, 4), (0, 3))]
    assert D.leaving_boxes(shape, (2, -3, 1)) == [((0, 2), (0, 4), (0, 3)), ((2, 5), (1, 4), (0, 3)),
                                                  ((2, 5), (0, 1), (0, 1))]


def test_the_policy_against_hand_computed_cases(lsf):
    mv = lsf.fusion.MovingVolume(4.0, (0.0, 0.0, 0.5))
    shape, voxel = (32, 32, 32), 0.004
    off = np.array([-15.5, -15.5, 125 - 15.5])  # centre = (0, 0, 125) voxels: the anchor at twist 0
    assert mv.shift_for(np.zeros(6), off, shape, voxel) == (0, 0, 0)
    # the camera at world x = 0.0152 m: d_x = 3.8 voxels, inside the threshold; at 0.0192 m: 4.8, truncated to 4
    assert mv.shift_for([-0.0152, 0, 0, 0, 0, 0], off, shape, voxel) == (0, 0, 0)
    assert mv.shift_for([-0.0192, 0, 0, 0, 0, 0], off, shape, voxel) == (4, 0, 0)
    # one axis past the threshold re-centres all three, each truncated towards zero
    assert mv.shift_for([-0.0192, 0.0108, -0.0068, 0, 0, 0], off, shape, voxel) == (4, -2, 1)
    # a camera turned by +90 degrees about y: X_cam = R X, R = [[0,0,1],[0,1,0],[-1,0,0]], so the anchor (0, 0, 0.5) is
    # the world point R^T (0, 0, 0.5) = (-0.5, 0, 0): with the centre at (0.25, 0, 125.25) d = (-125.25, 0, -125.25)
    quarter = [0, 0, 0, 0, np.pi / 2, 0]
    assert mv.shift_for(quarter, off + [0.25, 0, 0.25], shape, voxel) == (-125, 0, -125)
    # the float32 rounding of the twist: f is a float32 value, t64 a quarter of a float32 step above it, and the
    # window's centre puts the threshold between the two; the policy must see f, which stays
    f, step = float(np.float32(0.016)), float(np.spacing(np.float32(0.016)))
    t64 = f + 0.25 * step
    assert t64 > f and float(np.float32(t64)) == f
    centre_x = (f + 0.125 * step) / voxel - 4.0
    off_r = off + [centre_x, 0, 0]
    assert f / voxel - centre_x < 4.0 < t64 / voxel - centre_x
    assert mv.shift_for([-t64, 0, 0, 0, 0, 0], off_r, shape, voxel) == (0, 0, 0)
    assert mv.shift_for([-(f + 1.25 * step), 0, 0, 0, 0, 0], off_r, shape, voxel) == (4, 0, 0)
    for twist in (np.zeros(6), [-0.0192, 0.0108, -0.0068, 0, 0, 0], quarter, [-t64, 0, 0, 0, 0, 0],
                  [0.03, -0.02, 0.01, 0.1, -0.2, 0.05]):
        for o in (off, off_r):
            assert mv.shift_for(twist, o, shape, voxel) == V.policy_shift((0, 0, 0.5), 4.0, twist, o, shape, voxel)
    # a non-cubic window: the centre is per axis
    assert mv.shift_for(np.zeros(6), [-15.5, -7.5, 125 - 3.5], (8, 16, 32), voxel) == (0, 0, 0)
    assert mv.shift_for(np.zeros(6), [-15.5, -7.5, 125 - 3.5 - 6], (8, 16, 32), voxel) == (0, 0, 6)


def test_refusals_that_need_no_device(lsf):
    from levelsetfusion_python_amd import device_volume_shift as D
    MV = lsf.fusion.MovingVolume
    for bad in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            MV(bad, (0, 0, 0.5))
    with pytest.raises(TypeError):
        MV(4.0)  # no default anchor: no depth is right across scenes
    for bad in ((0, 0), (0, 0, np.nan), (0, 0, 0, 1)):
        with pytest.raises(ValueError):
            MV(4.0, bad)
    with pytest.raises(ValueError):
        MV(4.0, (0, 0, 0.5), min_weight=np.nan)
    with pytest.raises(ValueError):
        MV(4.0, (0, 0, 0.5)).shift_for(np.zeros(6), [0, 0, 0], (8, 8), 0.004)
    assert D.shift_of(np.array([1, -2, 3], np.int64)) == (1, -2, 3) and D.shift_of((np.int32(4), 0, 0)) == (4, 0, 0)
    assert D.shift_of((2.0, 0.0, -1.0)) == (2, 0, -1)
    for bad in ((0.5, 0, 0), (1, 2), (1, 2, 3, 4), (np.nan, 0, 0), ("a", 0, 0), (2 ** 31, 0, 0)):
        with pytest.raises(ValueError):
            D.shift_of(bad)
    with pytest.raises(ValueError):
        D.params((8, 8), (1, 0, 0))
    with pytest.raises(ValueError):
        D.params((2048, 2048, 2048), (1, 0, 0))
    p = D.params((3, 4, 5), (7, -8, 9))
    assert (p.depth, p.height, p.width, p.shift_x, p.shift_y, p.shift_z) == (3, 4, 5, 7, -8, 9)
    with pytest.raises(ValueError):  # refused before anything touches a device
        lsf.SequenceFusion3d(None, 8, [0, 0, 0], moving_volume=(4.0, (0, 0, 0.5)))
    header = open(lsf._build.ABI_HEADER).read()
    assert "#define LSF_VOLUME_SHIFT_MAX_BLOCKS %d\n" % lsf._lib.VOLUME_SHIFT_MAX_BLOCKS in header
    assert "#define LSF_VOLUME_SHIFT_BLOCK_ROWS %d\n" % lsf._lib.VOLUME_SHIFT_BLOCK_ROWS in header
    assert "lsf_volume_shift.hip" in lsf._build.SOURCES
    assert lsf._lib.lib.lsf_volume_shift(None, None, None, None, None, None, None, None) == -1


def test_merge_meshes(lsf):
    merge = lsf.fusion.merge_meshes
    v1, f1 = np.arange(9, dtype=np.float32).reshape(3, 3), np.array([[0, 1, 2]], np.int32)
    v2, f2 = np.arange(12, dtype=np.float32).reshape(4, 3) + 100, np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f = merge([(v1, f1), none, (v2, f2)])
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, np.concatenate([v1, v2])) and np.array_equal(f, [[0, 1, 2], [3, 4, 5], [4, 5, 6]])
    n1, n2 = np.ones((3, 3), np.float32), np.zeros((4, 3), np.float32)
    c1, c2 = np.full((3, 3), 7, np.uint8), np.full((4, 3), 9, np.uint8)
    out = merge([(v1, f1, n1, c1), (v2, f2, n2, c2)])
    assert len(out) == 4 and np.array_equal(out[2], np.concatenate([n1, n2])) and out[3].dtype == np.uint8
    assert np.array_equal(out[3], np.concatenate([c1, c2]))
    assert len(merge([(v1, f1, c1)])) == 3 and merge([(v1, f1, c1)])[2].dtype == np.uint8
    for mixed in ([(v1, f1), (v2, f2, n2)], [(v1, f1, n1), (v2, f2, c2)], [(v1, f1, n1, c1), (v2, f2, n2)], []):
        with pytest.raises(ValueError):
            merge(mixed)


def _window_trail(count):
    """the window's offset DURING each of `count` frames under the true twists, and the shift after each"""
    off, offsets, shifts = MS.WINDOW_OFFSET.copy(), [], []
    for k in range(count):
        offsets.append(off.copy())
        s = V.policy_shift(MS.ANCHOR, MS.THRESHOLD, MS.true_twist(k), off, (MS.WINDOW,) * 3, MS.VOXEL)
        shifts.append(s)
        off = off + np.array(s, np.float64)
    return offsets, shifts, off


def always_inside(offsets, final_offset, n):
    """bool (Z, Y, X) over the final window: the voxels whose world voxel lay inside the window at every frame"""
    keep = np.ones((n, n, n), bool)
    for off in offsets:
        lo = np.round(off - final_offset).astype(int)  # whole voxels: this window's origin in the final window
        axes = []
        for j in (2, 1, 0):  # z, y, x
            i = np.arange(n)
            axes.append((i >= lo[j]) & (i < lo[j] + n))
        keep &= axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]
    return keep


PREFIX = 13  # the frames of the "shifting does not change what is fused" test


def test_the_scene_does_what_the_gpu_tests_rely_on():
    offsets, shifts, final = _window_trail(MS.FRAMES)
    moved = [s for s in shifts if s != (0, 0, 0)]
    assert len(moved) >= 2 and all(max(abs(v) for v in s) >= int(MS.THRESHOLD) for s in moved)
    assert final[0] - MS.WINDOW_OFFSET[0] > MS.WINDOW  # the last window shares no voxel with the first
    # the last camera sees nothing of the first window: every corner of it projects left of the image
    m = V.R.matrix3d(MS.true_twist(MS.FRAMES - 1))
    corners = np.array(list(itertools.product((0, MS.WINDOW - 1), repeat=3)), np.float64)
    cam = ((corners + MS.WINDOW_OFFSET) * MS.VOXEL) @ m[:3, :3].T + m[:3, 3]
    assert np.all(cam[:, 2] > 0) and np.all(MS.K[0, 0] * cam[:, 0] / cam[:, 2] + MS.K[0, 2] < -1)
    # a short prefix keeps more voxels inside every window than one frame fuses
    offsets, shifts, final = _window_trail(PREFIX)
    assert sum(s != (0, 0, 0) for s in shifts[:-1]) >= 2
    kept = int(always_inside(offsets, final - np.array(shifts[-1], np.float64), MS.WINDOW).sum())
    t, w = F.empty_model((MS.WINDOW,) * 3)
    band = F.fuse_depth(t, w, MS.render(MS.true_twist(PREFIX - 1)), MS.K, 1.0, offsets[-1], MS.true_twist(PREFIX - 1),
                        band=MS.BAND, voxel_size=MS.VOXEL)[2]["fused"]
    assert kept > band > 0, (kept, band)
