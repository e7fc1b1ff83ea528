"""The conditions tests/test_gpu_ragged_volumes.py relies on, checked on the scenes of tests/ragged_scene.py with the numpy
oracle alone (no GPU): which faces of the array carry band voxels (a BOUNDARY list beside the INTERIOR one, or none), the
band's size, how the extents sit against the box edge (4) and the prepare pass's 1024-voxel chunk, the regime of the
updates (several voxels: sparse states must give up; a fraction of a voxel: they must not), and that the oracle is quick
enough to be every GPU case's reference.  These are conditions on the inputs, not measurements: a scene that is changed
has to keep them.  Reference loop: nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:238-330, :360-362."""
import time

import numpy as np
import pytest

from oracle import lsf_oracle as O

import ragged_scene

CHUNK = 1024  # voxels per chunk of the prepare pass (kBandChunk)

KILLING = dict(compute_method=O.DIRECT, level_set_term_enabled=True, smoothing_term_method=O.KILLING,
               gradient_descent_rate=0.1, data_term_weight=1.0, smoothing_term_weight=0.2,
               isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2, maximum_warp_length_lower_threshold=0.0,
               max_iterations=4, min_iterations=4)

# name -> (voxels, band voxels, faces that carry band voxels as {(axis letter, side): count or None for "some"},
#          (lowest, highest) longest update of the four iterations in voxels, to the table's two digits)
FACTS = {
    "odd": (23310, 16496, {("x", 0): None, ("x", 1): None, ("z", 0): None, ("z", 1): None, ("y", 1): None}, (3.7, 5.1)),
    "fours": (20160, 15524, {(a, s): None for a in "xyz" for s in (0, 1)}, (2.3, 3.9)),
    "tiny": (315, 315, {("x", 0): 35, ("x", 1): 35, ("y", 0): 45, ("y", 1): 45, ("z", 0): 63, ("z", 1): 63}, (3.0, 4.1)),
    "far": (137250, 8763, {}, (0.18, 0.21)),
    # rows 0 and 32 (the two faces across y: the ellipse is 80 voxels tall in a 33-row array) hold 19 band voxels each,
    # columns 0 and 69 none
    "flat": (2310, 628, {("y", 0): 19, ("y", 1): 19}, (6.8, 10.7)),
}


@pytest.fixture(scope="module", params=sorted(ragged_scene.SCENES))
def case(request):
    name = request.param
    canonical, live = ragged_scene.scene(name)
    oracle = O.SlavchevaOracle(**KILLING)
    out = live.copy()
    started = time.perf_counter()
    oracle.optimize(out, canonical)
    return name, canonical, live, oracle, time.perf_counter() - started


def _band(canonical, live):
    return ~(O.is_truncated(live) & O.is_truncated(canonical))


def test_pair_follows_its_formula():
    """float32 fields in [-1, 1] of the asked shape; the canonical field is the unshifted, unscaled body; a voxel written
    out by hand; (x, y[, z]) order of semi / shift / scale / centre"""
    canonical, live = ragged_scene.pair((5, 7, 9), (3.0, 2.5, 4.0))
    assert canonical.shape == live.shape == (5, 7, 9) and canonical.dtype == live.dtype == np.float32
    assert float(np.abs(canonical).max()) <= 1.0 and float(np.abs(live).max()) <= 1.0
    same, _ = ragged_scene.pair((5, 7, 9), (3.0, 2.5, 4.0), shift=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))
    assert np.array_equal(same, canonical)
    z, y, x = 1, 5, 7
    cx, cy, cz = 4.3, 3.3, 2.3  # (extent - 1) / 2 + 0.3
    r = np.sqrt(((x - cx) / 3.0) ** 2 + ((y - cy) / 2.5) ** 2 + ((z - cz) / 4.0) ** 2)
    assert canonical[z, y, x] == np.float32(np.clip((r - 1.0) * 2.5 / 4.0, -1.0, 1.0))
    r = np.sqrt(((x - cx - 0.75) / (3.0 * 1.05)) ** 2 + ((y - cy + 0.5) / (2.5 * 0.95)) ** 2 + ((z - cz - 1.0) / 4.0) ** 2)
    assert live[z, y, x] == np.float32(np.clip((r - 1.0) * 2.5 / 4.0, -1.0, 1.0))
    c2, l2 = ragged_scene.pair((33, 70), (25.0, 40.0), centre=(10.0, 20.0))
    assert c2.shape == (33, 70) and c2[20, 10] == np.float32(-1.0) and c2[20, 35] == np.float32(0.0)  # x semi-axis 25


def test_extents_against_boxes_and_chunks():
    shapes = {name: shape for name, (shape, _) in ragged_scene.SCENES.items()}
    assert all(s % 4 for s in shapes["odd"]) and shapes["odd"][-1] % 2 == 1
    assert all(s % 4 == 0 and s % 8 for s in shapes["fours"]) and len(set(shapes["fours"])) == 3
    assert int(np.prod(shapes["tiny"])) < CHUNK
    assert len(shapes["flat"]) == 2
    for name in ("odd", "fours", "far", "flat"):  # a partial last chunk
        assert int(np.prod(shapes[name])) % CHUNK != 0
    nz, ny, nx = shapes["far"]
    assert 2 * CHUNK < ny * nx < 3 * CHUNK and (ny * nx) % CHUNK != 0  # a slice is 2.2 chunks
    assert len(set(shapes["far"])) == 3 and len(set(shapes["odd"])) == 3


def test_band_and_faces(case):
    name, canonical, live, _, _ = case
    voxels, band_voxels, faces, _ = FACTS[name]
    band = _band(canonical, live)
    assert band.size == voxels and int(band.sum()) == band_voxels
    letters = "zyx"[3 - band.ndim:]
    for axis, letter in enumerate(letters):
        for side in (0, 1):
            count = int(np.take(band, -side, axis=axis).sum())
            if (letter, side) in faces:
                want = faces[(letter, side)]
                assert count > 0 and (want is None or count == want), (name, letter, side, count)
            else:
                assert count == 0, (name, letter, side, count)
    # what the engine's lists must hold: INTERIOR = band voxels off every face, BOUNDARY = the rest
    inner = np.zeros_like(band)
    inner[(slice(1, -1),) * band.ndim] = True
    assert (int((band & ~inner).sum()) > 0) == bool(faces)
    assert int((band & inner).sum()) > 0


def test_update_regime(case):
    """`far` stays below one voxel (sparse states of reach 1 and 2 hold); every other scene moves two voxels or more in
    every iteration (a call on sparse states of reach 2 must give up), and no longest update ties with another voxel"""
    name, canonical, live, oracle, _ = case
    m = np.asarray(oracle.log["max_warps"])
    lo, hi = FACTS[name][3]
    assert len(m) == 4 and lo <= m.min() and m.max() <= hi, m
    if name == "far":
        assert m.max() < 1.0
    else:
        assert m.min() >= 2.0


def test_longest_update_does_not_tie():
    """the first iteration's longest update is the only voxel of its length (the arg-max is then the same whatever order
    a reduction visits the voxels in)"""
    for name in sorted(ragged_scene.SCENES):
        canonical, live = ragged_scene.scene(name)
        oracle = O.SlavchevaOracle(**dict(KILLING, max_iterations=1, min_iterations=1))
        oracle.optimize(live.copy(), canonical)
        lengths = O.vector_norm(oracle.warp_field)
        assert int((lengths == lengths.max()).sum()) == 1, name


def test_sobolev_updates_stay_small():
    """SobolevFusion (DIRECT terms, Tikhonov, the 7-tap kernel): below 0.16 voxels on every scene"""
    kernel = O.generate_1d_sobolev_kernel(7, 0.1)
    for name in sorted(ragged_scene.SCENES):
        canonical, live = ragged_scene.scene(name)
        oracle = O.SlavchevaOracle(compute_method=O.DIRECT, sobolev_smoothing_enabled=True, sobolev_kernel=kernel,
                                   maximum_warp_length_lower_threshold=0.0, max_iterations=4, min_iterations=4)
        oracle.optimize(live.copy(), canonical)
        assert 0.0 < max(oracle.log["max_warps"]) < 0.16, (name, oracle.log["max_warps"])


def test_threshold_probe_of_far():
    """the 12-iteration probe the threshold-terminated GPU case takes its lower threshold from: the maxima fall from the
    start, so iteration 2 is the first (from 2 on) below every earlier one and a threshold between ends the loop after three"""
    canonical, live = ragged_scene.scene("far")
    oracle = O.SlavchevaOracle(**dict(KILLING, max_iterations=12, min_iterations=12))
    oracle.optimize(live.copy(), canonical)
    m = np.float32(oracle.log["max_warps"])
    k = next(i for i in range(2, len(m)) if m[i] < m[:i].min())
    assert k == 2 and m[k] < (m[:k].min() + m[k]) / 2 < m[:k].min()


def test_oracle_is_quick(case):
    name, canonical, live, _, seconds = case
    if seconds >= 1.0:  # a busy machine: once more
        started = time.perf_counter()
        O.SlavchevaOracle(**KILLING).optimize(live.copy(), canonical)
        seconds = time.perf_counter() - started
    assert seconds < 1.0, (name, seconds)
