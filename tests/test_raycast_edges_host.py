"""CPU checks of the ray-caster's edge scenes (tests/raycast_edge_scene.py): the unclipped brute-force march
(tests/raycast_bruteforce.py) equals the clipped restatement (tests/raycast_restatement.py) bit for bit on every scene,
and every scene meets the condition that tests/test_gpu_raycast_edges.py relies on.  The conditions are conditions, not
measurements: if one fails, the scene changes.  numpy only."""
import numpy as np
import pytest

import photometric_restatement as P
import raycast_bruteforce as BF
import raycast_edge_scene as ES

FINITE = ES.finite_cases()


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _case(name):
    return next(c for c in ES.all_cases() if c.name == name)


@pytest.mark.parametrize("case", FINITE, ids=repr)
def test_the_unclipped_march_equals_the_restatement(case):
    """the clip, the pad, the first and last step and the step cap of the restatement change no depth bit and no hit"""
    ref = ES.reference(case)
    assert ref.hits == ref.restated_hits
    assert _bits_equal(ref.depth, ref.restated_depth)
    assert np.array_equal(ref.hit, ref.restated_depth > 0)  # s_hit >= step: a finite hit's depth is positive
    assert np.all(np.isnan(ref.s_hit) == ~ref.hit) and np.all(ref.s_hit[ref.hit].astype(np.float32) == ref.depth[ref.hit])


def test_ball_cameras_see_the_ball():
    for case in ES.ball_cases():
        hits = ES.reference(case).hits
        if case.name.endswith("behind"):
            assert hits == 0  # hi <= 0: the whole box lies behind the camera
            assert BF.steps(case.tsdf.shape, case.twist, case.offset, case.voxel_size) == 1
        else:
            assert hits >= (100 if "/ones/" in case.name else 10), (case, hits)


def test_the_box_has_three_extents_and_the_cameras_turn_past_a_quarter():
    """a transposed rotation or a swapped extent cannot cancel: X, Y and Z differ, and single-axis turns near and
    beyond 90 degrees exist about each axis"""
    assert len(set(ES.BALL_SHAPE)) == 3
    turns = {name: np.asarray(r) for name, (r, _) in ES.BALL_CAMERAS.items()}
    for axis in range(3):
        assert any(abs(r[axis]) >= 0.9 and np.count_nonzero(r) == 1 for r in turns.values())
    assert max(np.abs(r).max() for r in turns.values()) > np.pi / 2


def test_slab_rays_graze_the_faces_exactly():
    low, high = _case("slab/graze-low"), _case("slab/graze-high")
    for case, ax in ((low, 0.0), (high, 9.0)):
        a, b, _ = BF.ray(case.K, case.twist, case.offset, case.voxel_size, case.image_shape)
        assert np.all(b[0][:, 8] == 0.0) and np.all(a[0][:, 8] == ax)  # b_x == 0 and a_x on the face, exactly
    ref = ES.reference(low)
    assert ref.hit[:, 8].all() and np.all(ref.depth[:, 8] == np.float32(1.5))  # a_x == 0 is inside
    ref = ES.reference(high)
    assert not ref.hit[:, 8].any() and ref.hits >= 10  # a_x == n_x - 1 is outside
    assert ES.reference(_case("slab/mid")).hit.all() and not ES.reference(_case("slab/mid")).zero_normal.any()


def test_slab_samples_that_are_exactly_zero():
    case = _case("slab/exact-zero")
    ref = ES.reference(case)
    _, valid, value = BF.trace(*case.args())
    rows, cols = np.nonzero(ref.hit)
    own = value[ref.index[rows, cols], rows, cols]
    assert ref.hit.all() and np.count_nonzero(own == 0.0) >= 1  # a sample of exactly 0 is a hit (<= 0)
    assert ref.depth[4, 8] == np.float32(1.5)
    case = _case("slab/first-valid-zero")
    ref = ES.reference(case)
    _, valid, value = BF.trace(*case.args())
    first = valid.argmax(axis=0)
    rows, cols = np.indices(first.shape)
    assert valid.any(axis=0).all() and np.all(value[first, rows, cols] == 0.0)  # every ray's first valid sample is 0
    assert np.all(valid[first + 1, rows, cols] & (value[first + 1, rows, cols] < 0.0))  # and the next is negative
    assert ref.hits == 0  # prev > 0 is required: 0 then negative is no crossing


def test_the_inside_camera_starts_at_the_first_sample():
    case = _case("slab/inside")
    a, _, _ = BF.ray(case.K, case.twist, case.offset, case.voxel_size, case.image_shape)
    nz, ny, nx = case.tsdf.shape
    assert 0 < a[0][0, 0] < nx - 1 and 0 < a[1][0, 0] < ny - 1 and 0 < a[2][0, 0] < 4  # in the box, before z = 4
    inside, _, _ = BF.trace(*case.args())
    assert inside[1].all() and ES.reference(case).hit.all()  # lo < 0: the lane's first step is clamped to m = 1


def test_the_entry_hit_follows_a_sample_on_the_face():
    case = _case("slab/entry-hit")
    ref = ES.reference(case)
    inside, valid, value = BF.trace(*case.args())
    a, b, _ = BF.ray(case.K, case.twist, case.offset, case.voxel_size, case.image_shape)
    assert ref.hit.all() and np.all(ref.index == 5)
    assert inside[4].all() and not inside[3].any()  # sample 4 is every ray's first inside the box ...
    assert np.all(a[2] + (4.0 * 0.125) * b[2] == 0.0) and np.all((0.0 - a[2]) / b[2] / 0.125 == 4.0)  # ... on the face
    assert np.all(valid[4] & (value[4] > 0.0) & (value[5] < 0.0))


@pytest.mark.parametrize("case", FINITE, ids=repr)
def test_the_first_step_is_never_late(case):
    """the contract's first step, max(floor(lo / step) - 1, 1), is at or before every ray's first sample inside the
    box, and so is floor(lo / step) itself: the one-step pad in front is slack.  lo is an s from a division, the
    samples are a + s b, both within a few ulp, and hi / step < 2^50 keeps a few ulp of lo / step below one step.  A
    kernel without the front pad computes the same image on every scene; one whose first step is later does not
    (slab/entry-hit)"""
    a, b, _ = BF.ray(case.K, case.twist, case.offset, case.voxel_size, case.image_shape)
    inside, _, _ = BF.trace(*case.args())
    nz, ny, nx = case.tsdf.shape
    lo = np.full(a[0].shape, -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j, n in enumerate((nx, ny, nz)):
            s1, s2 = (0.0 - a[j]) / b[j], (float(n - 1) - a[j]) / b[j]
            lo = np.where(b[j] != 0.0, np.maximum(lo, np.minimum(s1, s2)), lo)
    enters = inside.any(axis=0)
    first = inside.argmax(axis=0)
    unpadded = np.maximum(np.floor(lo / (case.voxel_size / BF.STEP_DIVISOR)), 1.0)
    assert np.all(unpadded[enters] <= first[enters])


@pytest.mark.parametrize("name", ["slab/graze-low", "ball/holes/mixed"])
def test_hits_with_and_without_a_normal(name):
    ref = ES.reference(_case(name))
    assert int(ref.zero_normal.sum()) >= 10 and int((ref.hit & ~ref.zero_normal).sum()) >= 10


@pytest.mark.parametrize("case", ES.needle_cases(), ids=repr)
def test_needles_take_hundreds_of_steps(case):
    ref = ES.reference(case)
    assert ref.hits >= 40 and ref.index[ref.hit].max() >= 200


@pytest.mark.parametrize("case", FINITE, ids=repr)
def test_no_ray_needs_the_step_cap(case, record_property):
    needed = ES.steps_needed(case)
    record_property("steps_needed", needed)
    record_property("step_cap", case.step_cap)
    assert needed < case.step_cap


def test_rays_cross_holes_before_their_hit():
    for case in ES.ball_cases():
        crossings = ES.hole_crossings(case)
        if "/holes/" in case.name and not case.name.endswith("behind"):
            assert crossings >= 10, (case, crossings)
        else:
            assert crossings == 0, (case, crossings)


def test_colour_weights_have_holes_of_their_own():
    volume = ES.colour_volume()
    wc, w = volume[..., 3], ES.ball_weight("holes")
    assert np.isnan(wc[w > 0]).sum() == 1 and (wc[w > 0] < 0).sum() == 1 and (wc[w > 0] == 0).sum() > 50
    assert np.all(wc[4:6, 2:4, 3:5][~np.isnan(wc[4:6, 2:4, 3:5])] >= 0)
    with_colour = without = 0
    for case in ES.colour_cases():
        ref = ES.reference(case)
        image, valid = ES.colour_reference(case)
        assert not (valid & ~ref.hit).any()
        assert np.array_equal(np.isnan(image).any(axis=2), ~valid) and np.array_equal(np.isnan(image).all(axis=2), ~valid)
        # the restated colour image, which finds s_hit again from the rounded depth, agrees
        restated = P.raycast_colour(*case.args()[:2], case.colour, *case.args()[2:])[3]
        assert np.array_equal(restated.view(np.uint32), image.view(np.uint32))
        with_colour += int(valid.sum())
        without += int((ref.hit & ~valid).sum())
        if case.name in ("colour/ry", "colour/back", "colour/mixed"):
            assert int(valid.sum()) >= 10 and int((ref.hit & ~valid).sum()) >= 10, case
    assert with_colour >= 10 and without >= 10
    r, g, b = (volume[..., ch].astype(np.float64).ravel() for ch in range(3))
    for p, q in ((r, g), (r, b), (g, b)):  # distinct, and no channel a multiple of another
        assert np.linalg.matrix_rank(np.stack([p, q])) == 2


def test_crops_are_crops():
    full = ES.reference(_case("ball/ones/mixed"))
    for case in ES.crop_cases():
        h, w = case.image_shape
        ref = ES.reference(case)
        assert _bits_equal(ref.depth, full.depth[:h, :w]) and ref.hits == int(full.hit[:h, :w].sum())
    assert ES.reference(_case("crops/1x1")).hits == 0 and ES.reference(_case("crops/16x16")).hits >= 100


def test_the_non_finite_scene_reaches_the_image():
    """the restatement and the brute-force march agree there too (NaN payloads aside), and some depths are NaN"""
    nans = normal_nans = 0
    for case in ES.nonfinite_cases():
        ref = ES.reference(case)
        assert ref.hits == ref.restated_hits
        assert np.array_equal(np.isnan(ref.depth), np.isnan(ref.restated_depth))
        keep = ~np.isnan(ref.depth)
        assert _bits_equal(ref.depth[keep], ref.restated_depth[keep])
        nans += int(np.isnan(ref.depth).sum())
        normal_nans += int(np.isnan(ref.normals).any(axis=2).sum())
    # an infinite previous sample gives p / (p - c) = NaN; an infinite gradient gives a normal of n / inf
    assert nans >= 10 and normal_nans >= 10
