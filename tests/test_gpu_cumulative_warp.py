"""GPU checks of the cumulative warp of a KillingFusion call (csrc/lsf_cumulative_warp.hip, INTEGRATION.md section 3,
"Cumulative warp") against the numpy restatement (tests/cumulative_warp_restatement.py): PSI bit for bit (uint32 views)
on updates that leave the cell and the array, on lists and on the dense walk, on ragged and non-cubic volumes, behind a
stop test that fires inside a batch, and past the first trip of the kernel's capped grids; the call's other outputs against
the same call without the keyword; SequenceFusion3d end to end on tests/deforming_scene.py; reruns.
tests/test_cumulative_warp_host.py holds what is assumed about the inputs."""
import functools
import types

import numpy as np
import pytest
import torch

import cumulative_warp_restatement as CW
import deforming_scene as D
import mesh_restatement as M
import ragged_scene
from oracle import lsf_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _pair(key):
    """(canonical, live) of a named input, made once and read-only"""
    if key == "ortho64":
        pair = CW.ortho64()
    elif key == "sphere32":
        pair = O.sphere_pair(32, d=3)
    elif key == "smooth81":
        pair = CW.smooth_pair((81, 81, 81))
    else:
        pair = ragged_scene.scene(key)
    for a in pair:
        a.setflags(write=False)
    return pair


_RESTATED = {}


def _restated(key, cfg):
    """the restatement's run of `cfg` on a pair: computed once, shared, read-only"""
    frozen = (key,) + tuple(sorted(cfg.items()))
    if frozen not in _RESTATED:
        canonical, live = _pair(key)
        _RESTATED[frozen] = CW.run(canonical, live, cfg)
    return _RESTATED[frozen]


def _optimizer(lsf, dims, n, cfg, **kw):
    """the drop-in class for an oracle configuration (DIRECT terms)"""
    assert cfg["compute_method"] == O.DIRECT and cfg["data_term_method"] == O.BASIC
    cls = lsf.SlavchevaOptimizer3d if dims == 3 else lsf.SlavchevaOptimizer2d
    return cls(out_path=None, field_size=n, compute_method=lsf.ComputeMethod.DIRECT,
               level_set_term_enabled=cfg["level_set_term_enabled"],
               smoothing_term_method=lsf.SmoothingTermMethod.KILLING if cfg["smoothing_term_method"] == O.KILLING
               else lsf.SmoothingTermMethod.TIKHONOV,
               gradient_descent_rate=cfg["gradient_descent_rate"], data_term_weight=cfg["data_term_weight"],
               smoothing_term_weight=cfg["smoothing_term_weight"],
               isomorphic_enforcement_factor=cfg["isomorphic_enforcement_factor"],
               level_set_term_weight=cfg["level_set_term_weight"],
               maximum_warp_length_lower_threshold=cfg["maximum_warp_length_lower_threshold"],
               maximum_warp_length_upper_threshold=cfg["maximum_warp_length_upper_threshold"],
               max_iterations=cfg["max_iterations"], min_iterations=cfg["min_iterations"], **kw)


def _run_engine(key, cfg, options=None, check_interval=32, cumulative_warp=True):
    """one call of engine.SlavchevaEngine on device copies of a pair (non-cubes: the drop-in classes keep the reference's
    cube check): what it leaves behind, on the host"""
    from levelsetfusion_python_amd import _lib, device as dev, engine
    canonical, live = (torch.from_numpy(a.copy()).cuda() for a in _pair(key))
    eng = engine.SlavchevaEngine(
        True, cfg["level_set_term_enabled"], False, _lib.DATA_BASIC,
        _lib.SMOOTHING_KILLING if cfg["smoothing_term_method"] == O.KILLING else _lib.SMOOTHING_TIKHONOV,
        cfg["gradient_descent_rate"], cfg["data_term_weight"], cfg["smoothing_term_weight"],
        cfg["isomorphic_enforcement_factor"], cfg["level_set_term_weight"], cfg["maximum_warp_length_lower_threshold"],
        cfg["maximum_warp_length_upper_threshold"], cfg["max_iterations"], cfg["min_iterations"], None,
        check_interval=check_interval, options=options, cumulative_warp=cumulative_warp)
    lower = cfg["maximum_warp_length_lower_threshold"]
    outcome = eng.optimize(live, canonical, finalize=(live, lower, True))
    final, warp, _ = outcome.finalize(live, lower, True)
    assert final is live
    warp = warp() if callable(warp) else warp
    psi = eng.cumulative_warp_field()
    return types.SimpleNamespace(engine=eng, live=live.cpu().numpy(), warp=warp.cpu().numpy(),
                                 gradient=dev.interleave(eng.gradient_field()).cpu().numpy(),
                                 psi=None if psi is None else psi.cpu().numpy(), iteration_count=eng.iteration_count,
                                 max_warps=np.float32(eng.log["max_warps"]), indices=list(eng.log["max_warp_indices"]),
                                 energies=[list(eng.log[k]) for k in ("data_energies", "smoothing_energies",
                                                                      "level_set_energies")])


def _check(run, ref):
    """PSI and the call's fields bit for bit, the iteration count and every iteration's maximum"""
    assert run.iteration_count == ref.iteration_count
    assert _bits_equal(run.psi, ref.psi), "cumulative warp"
    assert _bits_equal(run.live, ref.live) and np.array_equal(run.warp, ref.warp)
    assert np.array_equal(run.max_warps, np.float32(ref.log["max_warps"]))


# ----------------------------------------------------------------------- updates that leave the cell and the array, 2-D
def test_orthographic_pair_of_config_1(lsf):
    """BASELINE config 1's 64 x 64 input, KillingFusion, 10 iterations: updates of 6.5 to 10 voxels, so the gather leaves
    the voxel's cell and the array; through the drop-in class, numpy in and a device tensor in"""
    cfg = CW.fixed(10)
    ref = _restated("ortho64", cfg)
    assert np.float32(ref.log["max_warps"]).min() > 2
    canonical, live0 = _pair("ortho64")
    opt = _optimizer(lsf, 2, 64, cfg, cumulative_warp=True)
    assert opt.cumulative_warp_field is None
    live = live0.copy()
    opt.optimize(live, canonical.copy())
    psi = opt.cumulative_warp_field
    assert isinstance(psi, np.ndarray) and psi.dtype == np.float32 and psi.shape == (64, 64, 2)
    assert _bits_equal(psi, ref.psi) and _bits_equal(live, ref.live) and np.array_equal(opt.warp_field, ref.warp)
    assert not opt.engine.last_call.library_run and opt.engine.iteration_count == 10
    assert np.count_nonzero(psi.any(axis=-1)) > 500 and not _bits_equal(psi, ref.summed)
    live_dev = torch.from_numpy(live0.copy()).cuda()
    opt.optimize(live_dev, torch.from_numpy(canonical.copy()).cuda())
    psi_dev = opt.cumulative_warp_field
    assert isinstance(psi_dev, torch.Tensor) and psi_dev.is_cuda and psi_dev.dtype == torch.float32
    assert opt.cumulative_warp_field is psi_dev  # built once
    assert _bits_equal(psi_dev.cpu().numpy(), ref.psi) and _bits_equal(live_dev.cpu().numpy(), ref.live)


# ------------------------------------------------------------------------------------------- the sphere pair, 30 iterations
@pytest.mark.parametrize("use_band_list", [True, False])
@pytest.mark.parametrize("check_interval", [1, 32])
def test_sphere_pair(lsf, check_interval, use_band_list):
    """lists and the dense walk against the same restatement: they are equal"""
    cfg = CW.fixed(30)
    ref = _restated("sphere32", cfg)
    canonical, live0 = _pair("sphere32")
    opt = _optimizer(lsf, 3, 32, cfg, cumulative_warp=True, check_interval=check_interval,
                     engine_options=dict(use_band_list=use_band_list))
    live = live0.copy()
    opt.optimize(live, canonical.copy())
    assert opt.engine.iteration_count == 30 and not opt.engine.last_call.library_run
    bands = opt.engine._fast.bands
    assert (len(bands) == 2 and all(b.count for b in bands)) if use_band_list else bands[0].indices is None
    psi = opt.cumulative_warp_field
    assert psi.shape == (32, 32, 32, 3) and _bits_equal(psi, ref.psi) and _bits_equal(live, ref.live)
    assert np.array_equal(opt.warp_field, ref.warp)
    assert np.array_equal(np.float32(opt.log.max_warps), np.float32(ref.log["max_warps"]))


# ------------------------------------------------------------------------------------------ ragged and non-cubic volumes
@pytest.mark.parametrize("walk", ["lists", "dense"])
@pytest.mark.parametrize("name", ["odd", "tiny", "far", "fours"])
def test_ragged_volumes(lsf, name, walk):
    """three different extents: a channel order other than x, y, z, or a transposed gather, reads another field; partial
    tiles, partial 256-entry units and 1024-voxel chunks are crossed"""
    cfg = CW.fixed(4)
    ref = _restated(name, cfg)
    run = _run_engine(name, cfg, None if walk == "lists" else dict(use_band_list=False))
    assert not run.engine.last_call.library_run
    bands = run.engine._fast.bands
    if walk == "lists":
        assert len(bands) == (1 if name == "far" else 2) and all(b.count for b in bands)
    else:
        assert len(bands) == 1 and bands[0].indices is None
    _check(run, ref)
    assert np.count_nonzero(ref.psi.any(axis=-1)) > (100 if name == "tiny" else 1000)
    assert not _bits_equal(ref.psi, ref.psi[..., ::-1]) and not _bits_equal(ref.psi, ref.summed)


def test_sparse_states_are_only_read_where_listed(lsf):
    """states initialised near the band only: the composition reads the listed voxels' states and nothing else"""
    cfg = CW.fixed(4)
    run = _run_engine("far", cfg, dict(sparse_reach=2, sparse_min_voxels=0))
    assert run.engine.last_call.sparse_states and not run.engine.sparse_disabled
    _check(run, _restated("far", cfg))
    # `odd` moves 3.7 to 5 voxels: the sparse attempt gives up, and the second attempt composes from zeros again
    run = _run_engine("odd", cfg, dict(sparse_reach=2, sparse_min_voxels=0))
    assert run.engine.sparse_disabled and not run.engine.last_call.sparse_states
    _check(run, _restated("odd", cfg))


# ----------------------------------------------------------------------------------------------- a stop test that fires
@pytest.mark.parametrize("check_interval", [4, 32])
def test_threshold_terminated(lsf, check_interval):
    """the lower threshold lies between the oracle's own maxima, so that it stops after n iterations, 1 < n < 4: the gated
    launches behind the stop, iterations and compositions alike, do nothing"""
    probe = np.float32(_restated("far", CW.fixed(12)).log["max_warps"])
    k = next(i for i in range(1, len(probe)) if probe[i] < probe[:i].min())
    threshold = float((probe[:k].min() + probe[k]) / 2)
    cfg = dict(CW.KILLING, min_iterations=1, max_iterations=30, maximum_warp_length_lower_threshold=threshold)
    ref = _restated("far", cfg)
    assert ref.iteration_count == k + 1 and 1 < ref.iteration_count < min(check_interval, 4)
    run = _run_engine("far", cfg, check_interval=check_interval)
    assert run.iteration_count == ref.iteration_count and len(run.max_warps) == ref.iteration_count
    _check(run, ref)
    assert not _bits_equal(ref.psi, _restated("far", CW.fixed(ref.iteration_count + 1)).psi)  # one more would show


def test_zero_iterations_leave_zeros(lsf):
    cfg = dict(CW.KILLING, min_iterations=0, max_iterations=5)
    run = _run_engine("tiny", cfg)
    assert run.iteration_count == 0 and _bits_equal(run.psi, np.zeros((5, 7, 9, 3), F32))


# --------------------------------------------------------------------------------------- the second trip of the capped grids
BLOCK, XCDS, BLOCKS_PER_XCD, LIST_BLOCKS_PER_XCD = 256, 8, 251, 256  # kBlock, kXcds, kBlocksPerXcd, band_list_blocks' default
TILE_X, TILE_Y = 64, 4                                                # kTileX, Grid::tile_y


def _dense_blocks_and_tiles(shape):
    """launch_blocks(make_tiling(g).total) of csrc/lsf_device.h: tiles of 64 x 4 voxels of a slice, at most 8 * 251 blocks"""
    nz, ny, nx = shape
    tiles = -(-nx // TILE_X) * -(-ny // TILE_Y) * nz
    return min(tiles, XCDS * BLOCKS_PER_XCD), tiles


def _list_blocks_and_units(count):
    """band_list_blocks(count) of csrc/lsf_device.h: units of 256 entries, every block the same number of them"""
    units = -(-count // BLOCK)
    if units <= XCDS:
        return max(units, 1), units
    per_xcd = -(-units // XCDS)
    rounds = -(-per_xcd // LIST_BLOCKS_PER_XCD)
    return XCDS * -(-per_xcd // rounds), units


def test_the_smooth_pair_crosses_both_caps():
    shape = (81, 81, 81)
    blocks, tiles = _dense_blocks_and_tiles(shape)
    assert blocks == 2008 and tiles == 3402 > blocks  # the dense walk: some blocks take a second tile
    assert _dense_blocks_and_tiles((64, 64, 64))[1] <= 2008
    blocks, units = _list_blocks_and_units(81 ** 3)
    assert 81 ** 3 == 531441 > XCDS * LIST_BLOCKS_PER_XCD * BLOCK and units == 2 * blocks - 4  # a list of every voxel: two units per block
    assert _list_blocks_and_units(80 ** 3)[1] <= _list_blocks_and_units(80 ** 3)[0]


@pytest.mark.parametrize("walk", ["lists", "dense"])
def test_every_voxel_in_the_band(lsf, walk):
    """a smooth (81, 81, 81) pair, every voxel in the band, 2 iterations: 3402 tiles on 2008 blocks, and lists of 493 039
    INTERIOR and 38 402 BOUNDARY voxels"""
    cfg = CW.fixed(2)
    ref = _restated("smooth81", cfg)
    run = _run_engine("smooth81", cfg, None if walk == "lists" else dict(use_band_list=False))
    if walk == "lists":
        assert sorted(b.count for b in run.engine._fast.bands) == [81 ** 3 - 79 ** 3, 79 ** 3]
    _check(run, ref)
    assert np.count_nonzero(ref.psi.any(axis=-1)) > 500000  # nearly every voxel moves: a tile left out would show


def test_one_launch_over_a_list_of_every_voxel(lsf):
    """lsf_cumulative_warp_compose on its own over ONE list of 531 441 entries, past band_list_blocks' 8 x 256 x 256: the
    second trip of its list walk, and the dense walk on the same buffers.  Random states and PSI; updates of +-1e30 gather
    outside the array (PSI' = u); a NaN or infinite update gives NaN at its own voxel and touches no other"""
    from levelsetfusion_python_amd import _lib, device as dev
    shape = (81, 81, 81)
    n = int(np.prod(shape))
    assert _list_blocks_and_units(n)[1] > _list_blocks_and_units(n)[0]
    rng = np.random.default_rng(53)
    update = rng.uniform(-3, 3, shape + (3,)).astype(F32)
    flat = update.reshape(-1)
    flat[5::1009] = 1e30
    flat[7::1013] = -1e30
    flat[11::4099] = 0.0
    wild = np.zeros(n * 3, bool)
    wild[13::50021] = True
    finite = update.copy()
    for value, at in zip((np.nan, np.inf, -np.inf), np.array_split(np.flatnonzero(wild), 3)):
        flat[at] = value
    wild = wild.reshape(shape + (3,)).any(axis=-1)
    finite[wild] = 0.0
    psi_in = rng.uniform(-4, 4, shape + (3,)).astype(F32)
    want = CW.compose(psi_in, finite)
    assert np.count_nonzero(wild) > 20 and np.isfinite(want).all()
    state = torch.from_numpy(np.concatenate([rng.uniform(-1, 1, shape + (1,)).astype(F32), update], axis=-1)).cuda()
    psi4 = torch.from_numpy(np.concatenate([np.zeros(shape + (1,), F32), psi_in], axis=-1)).cuda()
    grid = dev.make_grid(shape)
    every = dev.BandList(torch.arange(n, dtype=torch.int32, device="cuda"), n, _lib.BAND_ALL)
    for band in (every, None):
        out4 = torch.full(shape + (4,), 7.0, dtype=torch.float32, device="cuda")
        dev.cumulative_warp_compose(state, psi4, out4, grid, None, band)
        got = torch.empty(shape + (3,), dtype=torch.float32, device="cuda")
        dev.state_unpack(out4, grid, warp_interleaved_out=got)
        got = got.cpu().numpy()
        assert not out4[..., 0].any() and np.isnan(got[wild]).all()
        assert _bits_equal(got[~wild], want[~wild])
    with pytest.raises(_lib.LsfHipError, match="BAD_ARGUMENT"):
        dev.cumulative_warp_compose(state, psi4, psi4, grid, None, every)


# --------------------------------------------------------------------------------------- the keyword on against off
def test_the_keyword_changes_nothing_else(lsf):
    """the same call with and without the keyword: live, warp_field, gradient_field, iteration count, every iteration's
    maximum and its location bit for bit.  The energies are float64 sums that every launch accumulates by atomic adds in
    the order its blocks arrive, so two launches of the same kernel need not agree in the last bits: they are compared to
    the 1e-9 relative every comparison of these sums in this suite uses (tests/test_gpu_ragged_volumes.py)."""
    cfg = CW.fixed(30)
    canonical, live0 = _pair("sphere32")
    out = {}
    for on in (True, False):
        opt = _optimizer(lsf, 3, 32, cfg, cumulative_warp=on)
        live = live0.copy()
        opt.optimize(live, canonical.copy())
        out[on] = (opt, live, opt.warp_field, opt.gradient_field)
        assert opt.engine.last_call.library_run == (not on)
        assert (opt.cumulative_warp_field is None) == (not on)
    (a, live_a, warp_a, grad_a), (b, live_b, warp_b, grad_b) = out[True], out[False]
    assert _bits_equal(live_a, live_b) and _bits_equal(warp_a, warp_b) and _bits_equal(grad_a, grad_b)
    assert a.engine.iteration_count == b.engine.iteration_count == 30
    assert _bits_equal(a.log.max_warps, b.log.max_warps) and a.log.max_warp_locations == b.log.max_warp_locations
    for name in ("data_energies", "smoothing_energies", "level_set_energies"):
        mine, theirs = getattr(a.log, name), getattr(b.log, name)
        print("%s bit-equal with the keyword on and off: %s" % (name, mine == theirs))
        assert np.allclose(mine, theirs, rtol=1e-9, atol=1e-12), name
    ra, rb = a.get_convergence_report(), b.get_convergence_report()
    assert ra.iteration_count == rb.iteration_count and ra.iteration_limit_reached == rb.iteration_limit_reached
    assert ra.warp_delta_statistics.longest_warp_location == rb.warp_delta_statistics.longest_warp_location
    assert ra.warp_delta_statistics.length_max == rb.warp_delta_statistics.length_max
    assert ra.tsdf_difference_statistics.difference_max == rb.tsdf_difference_statistics.difference_max


def test_the_hook_and_the_focus_trace_keep_working(lsf):
    cfg = CW.fixed(5)
    ref = _restated("sphere32", cfg)
    canonical, live0 = _pair("sphere32")
    seen = []
    opt = _optimizer(lsf, 3, 32, cfg, cumulative_warp=True, focus_coordinates=(16, 9, 16))
    opt.iteration_hook = lambda level, it, warp, gradient, max_warp: seen.append((it, max_warp))
    live = live0.copy()
    opt.optimize(live, canonical.copy())
    assert [it for it, _ in seen] == list(range(5)) and len(opt.focus_neighborhood_log) == 27
    assert np.array_equal(np.float32([m for _, m in seen]), np.float32(ref.log["max_warps"]))
    assert _bits_equal(opt.cumulative_warp_field, ref.psi) and _bits_equal(live, ref.live)


# ------------------------------------------------------------------------------------------------------ end to end
CHAIN = CW.fixed(30, level_set_term_enabled=False)


@functools.lru_cache(maxsize=None)
def _chain():
    """the restated chain; the level-set term is off for the reason tests/test_cumulative_warp_host.py's chain() gives"""
    return CW.deforming_chain(CHAIN)


def _camera(K_, ratio=1.0):
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    return DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=K_), depth_unit_ratio=ratio)


def _sequence(lsf, optimizer=True, **kw):
    opt = _optimizer(lsf, 3, D.N, CHAIN, cumulative_warp=True) if optimizer else None
    return lsf.SequenceFusion3d(_camera(D.K), D.N, D.OFFSET, voxel_size=D.VOXEL, narrow_band_width_voxels=D.BAND,
                                rigid_iterations=0, nonrigid_optimizer=opt, **kw)


def test_a_growing_sphere_is_fused_through_the_cumulative_warp(lsf):
    """fused through PSI, frame 1 changes the model near its surface by less than half of what it changes it by when fused
    rigidly (the restated chain gives 0.070 against 0.212), and warp and model are the restated chain's, bit for bit"""
    t0, W0, psi, t1, W1, want, rigid_t1, _ = _chain()
    d0, d1 = D.frames()
    seq, rigid = _sequence(lsf), _sequence(lsf, optimizer=False)
    assert seq.warped
    first = seq.integrate(d0)
    rigid.integrate(d0)
    assert seq.warp is None and first["nonrigid"] is None and tuple(first["fusion"]) == lsf.fusion.RECORD_FIELDS
    assert _bits_equal(seq.canonical.tsdf.cpu().numpy(), t0) and _bits_equal(seq.canonical.weight.cpu().numpy(), W0)
    frame = seq.integrate(d1)
    rigid.integrate(d1)
    got_t, rigid_t = seq.canonical.tsdf.cpu().numpy(), rigid.canonical.tsdf.cpu().numpy()
    through, rigidly = D.model_change(t0, got_t), D.model_change(t0, rigid_t)
    print("mean |change| near the surface: %.6f through the cumulative warp, %.6f rigidly" % (through, rigidly))
    assert through < 0.5 * rigidly
    assert _bits_equal(rigid_t, rigid_t1)
    assert seq.warp.is_cuda and seq.warp.dtype == torch.float32 and tuple(seq.warp.shape) == (D.N,) * 3 + (3,)
    assert _bits_equal(seq.warp.cpu().numpy(), psi)
    assert _bits_equal(got_t, t1) and _bits_equal(seq.canonical.weight.cpu().numpy(), W1)
    assert tuple(frame["fusion"]) == lsf.fusion.WARPED_RECORD_FIELDS
    for key in ("fused", "first_seen", "max_abs_change", "carved", "weight_rejected", "coloured", "warp_rejected"):
        assert frame["fusion"][key] == want[key], key
    assert abs(frame["fusion"]["sum_abs_change"] - want["sum_abs_change"]) <= 1e-12 * want["sum_abs_change"]
    assert frame["fusion"]["fused"] > 1000 and frame["fusion"]["warp_rejected"] == 0
    call = frame["nonrigid"]
    assert call is seq.nonrigid_optimizer.engine.last_call and not call.library_run
    assert seq.nonrigid_optimizer.engine.iteration_count == 30
    assert np.array_equal(frame["twist"], np.zeros(6)) and len(seq.frame_records) == 2


def test_a_growing_sphere_with_carving_and_colour(lsf):
    d0, d1 = D.frames()
    image = D.colour_image()
    seq = _sequence(lsf, carve=True, colour=True)
    for d in (d0, d1):
        frame = seq.integrate(d, image)
        assert frame["fusion"]["carved"] > 1000 and frame["fusion"]["coloured"] > 1000
    assert tuple(frame["fusion"]) == lsf.fusion.WARPED_RECORD_FIELDS and frame["fusion"]["warp_rejected"] == 0
    # on an empty model carving changes weights alone, so the model after frame 0 and the warp are the uncarved run's
    assert _bits_equal(seq.warp.cpu().numpy(), _chain()[2])
    verts, faces, colours = seq.extract_mesh(colours=True)
    # carving gives the voxels the camera looks through a weight, so the carved model draws every cell the uncarved
    # restated chain's model draws (357 vertices, 572 faces by tests/mesh_restatement.py) and more
    t1, W1 = _chain()[3:5]
    want_verts, want_faces = M.extract(t1, W1, D.OFFSET, D.VOXEL)[:2]
    assert len(verts) >= len(want_verts) > 300 and len(faces) >= len(want_faces) > 500 and colours.dtype == np.uint8
    assert np.array_equal(colours, np.broadcast_to(np.array(D.COLOUR, np.uint8), (len(verts), 3)))


def test_without_the_keyword_the_sequence_is_as_before(lsf):
    opt = _optimizer(lsf, 3, D.N, CHAIN)
    with pytest.raises(ValueError, match="nonrigid_optimizer"):
        lsf.SequenceFusion3d(_camera(D.K), D.N, D.OFFSET, nonrigid_optimizer=opt, carve=True)
    seq = lsf.SequenceFusion3d(_camera(D.K), D.N, D.OFFSET, voxel_size=D.VOXEL, narrow_band_width_voxels=D.BAND,
                               rigid_iterations=0, nonrigid_optimizer=opt)
    assert not seq.warped
    for d in D.frames():
        frame = seq.integrate(d)
    assert seq.warp is None and tuple(frame["fusion"]) == lsf.fusion.RECORD_FIELDS  # volume mode
    assert frame["nonrigid"].library_run and opt.cumulative_warp_field is None


# --------------------------------------------------------------------------------------------------------- reruns
def test_reruns_are_bit_identical(lsf):
    cfg = CW.fixed(4)
    first, again = _run_engine("odd", cfg), _run_engine("odd", cfg)
    for x, y in ((first.psi, again.psi), (first.live, again.live), (first.warp, again.warp)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(first.max_warps, again.max_warps) and first.indices == again.indices
