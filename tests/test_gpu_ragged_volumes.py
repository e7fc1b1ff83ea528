"""The KillingFusion / SobolevFusion engine on ragged and non-cubic arrays (tests/ragged_scene.py: no extent a multiple of
the box edge, three different extents, a partial last 1024-voxel chunk, less than one chunk, slices of 2.2 chunks, 2-D
33 x 70), every way a call can be walked -- the library-enqueued call on lists, launch by launch, the dense tile walk, the
box walk and its refusal, sparsely initialised states and their fall-back, SobolevFusion on float4 lists, on boxes and on
planar fields, every term configuration, a threshold-terminated call, the drop-in classes on odd cubes, fields that are
not 16-byte aligned -- each against the numpy ORACLE of the same call, never against another GPU path alone: live, warp and
gradient field bit for bit, every iteration's maximum and its location, the energies to 1e-9 (float64 atomic sums), the
convergence report.  Every case asserts, from engine.last_call and engine._fast.bands, that the call took the path it is
named for.  Non-cubes are driven through engine.SlavchevaEngine (the drop-in classes keep the reference's cube check,
slavcheva_optimizer2d.py:157-161).  tests/test_ragged_scene_host.py holds what is assumed about the scenes.
Reference loop: nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:238-330, :354-388; report :393-404."""
import types

import numpy as np
import pytest
import torch

from oracle import lsf_oracle as O

import ragged_scene

pytestmark = pytest.mark.gpu

EXACT = 0.0

# the oracle's keywords; Killing + level set, DIRECT, four iterations, no stop test
BASE = dict(compute_method=O.DIRECT, level_set_term_enabled=True, sobolev_smoothing_enabled=False,
            data_term_method=O.BASIC, smoothing_term_method=O.KILLING, gradient_descent_rate=0.1, data_term_weight=1.0,
            smoothing_term_weight=0.2, isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2,
            maximum_warp_length_lower_threshold=0.0, maximum_warp_length_upper_threshold=10000, max_iterations=4,
            min_iterations=4, sobolev_kernel=None)
# SobolevFusion: DIRECT terms, Tikhonov, no level set, the zero-preserving filter (slavcheva_optimizer2d.py:238-330)
SOBOLEV = dict(BASE, level_set_term_enabled=False, smoothing_term_method=O.TIKHONOV, sobolev_smoothing_enabled=True)


@pytest.fixture(scope="module")
def lsf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import levelsetfusion_python_amd as pkg
    return pkg


def maxdiff(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


_KERNELS = {}


def _kernel(taps):
    if taps not in _KERNELS:
        _KERNELS[taps] = O.generate_1d_sobolev_kernel(taps, 0.1)
        _KERNELS[taps].setflags(write=False)
    return _KERNELS[taps]


_PAIRS = {}


def _pair(key):
    """a scene's name, or (shape, semi): (canonical, live), made once and read-only"""
    if key not in _PAIRS:
        canonical, live = ragged_scene.scene(key) if isinstance(key, str) else ragged_scene.pair(*key)
        canonical.setflags(write=False)
        live.setflags(write=False)
        _PAIRS[key] = (canonical, live)
    return _PAIRS[key]


_ORACLE = {}


def _oracle(key, cfg, report_lower=0.0):
    """the oracle's run of `cfg` on a pair, with its two statistics (computed once per case, shared, read-only)"""
    frozen = (key, report_lower) + tuple((k, v if k != "sobolev_kernel" or v is None else len(v))
                                         for k, v in sorted(cfg.items()))
    if frozen not in _ORACLE:
        canonical, live0 = _pair(key)
        o = O.SlavchevaOracle(**cfg)
        live = live0.copy()
        o.optimize(live, canonical)
        hi = cfg["maximum_warp_length_upper_threshold"]
        out = types.SimpleNamespace(
            live=live, warp=o.warp_field, gradient=o.gradient_field, log=o.log, iteration_count=o.iteration_count,
            warp_statistics=O.warp_delta_statistics(o.warp_field, canonical, live, report_lower, hi),
            tsdf_statistics=O.tsdf_difference_statistics(canonical, live))
        for a in (out.live, out.warp, out.gradient):
            a.setflags(write=False)
        _ORACLE[frozen] = out
    return _ORACLE[frozen]


def _make_engine(cfg, options=None, check_interval=32):
    from levelsetfusion_python_amd import _lib, engine
    kernel = cfg["sobolev_kernel"]
    return engine.SlavchevaEngine(
        cfg["compute_method"] == O.DIRECT, cfg["level_set_term_enabled"], cfg["sobolev_smoothing_enabled"],
        _lib.DATA_THRESHOLDED_FDM if cfg["data_term_method"] == O.THRESHOLDED_FDM else _lib.DATA_BASIC,
        _lib.SMOOTHING_KILLING if cfg["smoothing_term_method"] == O.KILLING else _lib.SMOOTHING_TIKHONOV,
        cfg["gradient_descent_rate"], cfg["data_term_weight"], cfg["smoothing_term_weight"],
        cfg["isomorphic_enforcement_factor"], cfg["level_set_term_weight"], cfg["maximum_warp_length_lower_threshold"],
        cfg["maximum_warp_length_upper_threshold"], cfg["max_iterations"], cfg["min_iterations"],
        None if kernel is None else np.asarray(kernel, dtype=np.float64), check_interval=check_interval, options=options)


def _run_engine(canonical, live, cfg, options=None, check_interval=32, report_lower=0.0):
    """one call of engine.SlavchevaEngine on device tensors, `live` warped in place: what it leaves behind, on the host"""
    from levelsetfusion_python_amd import convergence_report as R, device as dev
    eng = _make_engine(cfg, options, check_interval)
    outcome = eng.optimize(live, canonical, finalize=(live, report_lower, True))
    final, warp, raw = outcome.finalize(live, report_lower, True)
    assert final is live
    warp = warp() if callable(warp) else warp
    shape = tuple(live.shape)
    return types.SimpleNamespace(
        engine=eng, live=live.cpu().numpy(), warp=warp.cpu().numpy(),
        gradient=dev.interleave(eng.gradient_field()).cpu().numpy(),
        max_warps=list(eng.log["max_warps"]),
        locations=[tuple(int(i) for i in np.unravel_index(int(at), shape)) for at in eng.log["max_warp_indices"]],
        energies=[list(eng.log[k]) for k in ("data_energies", "smoothing_energies", "level_set_energies")],
        iteration_count=eng.iteration_count,
        warp_statistics=R.warp_delta_statistics_from_raw(raw[:8], shape, report_lower,
                                                         cfg["maximum_warp_length_upper_threshold"]),
        tsdf_statistics=R.tsdf_difference_statistics_from_raw(raw[8:], shape))


def _check_statistics(ws, ds, ref):
    """locations and counts exact; extrema as the float32 values they are; means and deviations to 1e-9 (float64 sums)"""
    want = ref.warp_statistics
    assert tuple(ws.longest_warp_location) == want["longest_warp_location"]
    assert ws.ratio_above_min_threshold == want["ratio_above_min_threshold"]  # two integer counts, one division
    assert ws.length_min == want["length_min"]
    assert np.float32(ws.length_max) == np.float32(want["length_max"])
    assert np.isclose(ws.length_mean, want["length_mean"], rtol=1e-9, atol=0.0)
    assert np.isclose(ws.length_standard_deviation, want["length_standard_deviation"], rtol=1e-9, atol=0.0)
    assert ws.is_largest_below_min_threshold == want["is_largest_below_min_threshold"]
    assert ws.is_largest_above_max_threshold == want["is_largest_above_max_threshold"]
    want = ref.tsdf_statistics
    assert tuple(ds.biggest_difference_location) == want["biggest_difference_location"]
    assert ds.difference_min == want["difference_min"]
    assert np.float32(ds.difference_max) == np.float32(want["difference_max"])
    assert np.isclose(ds.difference_mean, want["difference_mean"], rtol=1e-9, atol=0.0)
    assert np.isclose(ds.difference_standard_deviation, want["difference_standard_deviation"], rtol=1e-9, atol=0.0)


def _check(run, ref):
    assert run.iteration_count == ref.iteration_count
    assert maxdiff(run.live, ref.live) == EXACT, "live field"
    assert maxdiff(run.warp, ref.warp) == EXACT, "warp field"
    assert maxdiff(run.gradient, ref.gradient) == EXACT, "gradient field"
    assert np.array_equal(np.float32(run.max_warps), np.float32(ref.log["max_warps"]))
    assert run.locations == ref.log["max_warp_locations"]
    for mine, key in zip(run.energies, ("data_energies", "smoothing_energies", "level_set_energies")):
        assert np.allclose(mine, ref.log[key], rtol=1e-9, atol=1e-12), key
    _check_statistics(run.warp_statistics, run.tsdf_statistics, ref)


def _device(key):
    canonical, live = _pair(key)
    return torch.from_numpy(canonical.copy()).cuda(), torch.from_numpy(live.copy()).cuda()


def _case(key, cfg, options=None, **kw):
    canonical, live = _device(key)
    run = _run_engine(canonical, live, cfg, options, **kw)
    _check(run, _oracle(key, cfg, kw.get("report_lower", 0.0)))
    return run


def _numpy_lists(key):
    """(INTERIOR, BOUNDARY) voxel indices of the band union, ascending: tsdf_set_routines.py:19-52 and the faces"""
    canonical, live = _pair(key)
    band = ~(O.is_truncated(live) & O.is_truncated(canonical))
    inner = np.zeros_like(band)
    inner[(slice(1, -1),) * band.ndim] = True
    return np.flatnonzero(band & inner), np.flatnonzero(band & ~inner)


def _check_lists(bands, key):
    """the call's lists: the non-empty ones of (INTERIOR, BOUNDARY), each holding numpy's voxels"""
    from levelsetfusion_python_amd import _lib
    want = dict(zip((_lib.BAND_INTERIOR, _lib.BAND_BOUNDARY), _numpy_lists(key)))
    assert [b.subset for b in bands] == [s for s in (_lib.BAND_INTERIOR, _lib.BAND_BOUNDARY) if len(want[s])]
    for b in bands:
        assert b.count == len(want[b.subset])
        assert np.array_equal(b.indices[:b.count].cpu().numpy(), want[b.subset])


# ------------------------------------------------------------------------------------------ the default path
@pytest.mark.parametrize("name", ["odd", "fours", "tiny", "far", "flat"])
def test_library_run_on_lists(lsf, name):
    run = _case(name, BASE)
    call = run.engine.last_call
    assert call.library_run and not call.box_walk and not call.sparse_states and not call.sobolev_boxes
    bands = run.engine._fast.bands
    assert len(bands) == (1 if name == "far" else 2) and all(b.count for b in bands)
    _check_lists(bands, name)


@pytest.mark.parametrize("name", ["odd", "fours", "flat"])
def test_launch_by_launch(lsf, name):
    run = _case(name, BASE, dict(library_run=False))
    call = run.engine.last_call
    assert not call.library_run and not call.box_walk and not call.sparse_states
    bands = run.engine._fast.bands
    assert len(bands) == 2
    _check_lists(bands, name)


@pytest.mark.parametrize("name", ["odd", "tiny", "flat"])
def test_dense_tile_walk(lsf, name):
    """no list: the kernel walks tiles over every voxel, partial ones along x and y"""
    run = _case(name, BASE, dict(use_band_list=False))
    assert not run.engine.last_call.library_run
    bands = run.engine._fast.bands
    assert len(bands) == 1 and bands[0].indices is None and bands[0].count == 0


# ------------------------------------------------------------------------------------------ boxes
def test_box_walk_on_three_different_extents(lsf):
    run = _case("fours", BASE, dict(box_walk=True))
    call = run.engine.last_call
    assert call.library_run and call.box_walk
    boxes, boxed_canonical = run.engine._fast.boxes
    assert boxes is not None and boxes.shape[0] > 0 and boxed_canonical.numel() == 64 * boxes.shape[0]
    _check_lists(run.engine._fast.bands, "fours")


def test_box_walk_is_refused_off_multiples_of_four(lsf):
    run = _case("odd", BASE, dict(box_walk=True))
    call = run.engine.last_call
    assert call.library_run and not call.box_walk
    assert run.engine._fast.boxes == (None, None)
    _check_lists(run.engine._fast.bands, "odd")


def test_boxes_hold_the_interior_list_of_a_non_cube(lsf):
    """lsf_band_boxes_* with nx = 36, ny = 28, nz = 20: origins on multiples of four along every axis, ascending, the union
    of the boxes' voxels is numpy's INTERIOR list, the boxed canonical values are the canonical field's"""
    from levelsetfusion_python_amd import _lib, device as dev
    canonical, live = _device("fours")
    nz, ny, nx = canonical.shape
    assert (nz, ny, nx) == (20, 28, 36)
    grid = dev.make_grid((nz, ny, nx))
    assert dev.boxes_ok(grid)
    prepared = dev.StatePrepare(live, canonical, grid)
    bands, _ = prepared.collect()
    _check_lists(bands, "fours")
    boxes, count = dev.band_boxes(prepared)
    assert count > 0
    origin, mask = boxes[:count, 0] & 0xffffffff, boxes[:count, 1]
    assert bool((origin[1:] > origin[:-1]).all()), "ascending origins"
    x0, y0, z0 = origin % nx, (origin // nx) % ny, origin // (nx * ny)
    assert bool(((x0 % 4 == 0) & (y0 % 4 == 0) & (z0 % 4 == 0)).all()) and bool((mask != 0).all())
    assert int(x0.max()) == nx - 4 and int(y0.max()) == ny - 4 and int(z0.max()) == nz - 4  # the band reaches every face
    voxels = []
    for lane in range(64):
        has = ((mask >> lane) & 1).bool()
        lx, ly, lz = lane & 3, (lane >> 2) & 3, lane >> 4
        voxels.append((origin + (lz * ny + ly) * nx + lx)[has])
    voxels = torch.sort(torch.cat(voxels)).values
    assert np.array_equal(voxels.cpu().numpy(), _numpy_lists("fours")[0])
    boxed = dev.band_boxes_canonical(canonical, grid, boxes, count).view(-1, 4, 4, 4)
    for b in (0, count // 2, count - 1):
        bx, by, bz = int(x0[b]), int(y0[b]), int(z0[b])
        assert torch.equal(boxed[b], canonical[bz:bz + 4, by:by + 4, bx:bx + 4])
    # every band voxel, faces included
    boxes_all, count_all = dev.band_boxes(prepared, _lib.BAND_ALL)
    assert count_all >= count
    assert int(sum(bin(int(m) & 0xffffffffffffffff).count("1") for m in boxes_all[:count_all, 1].tolist())) \
        == sum(len(v) for v in _numpy_lists("fours"))


# ------------------------------------------------------------------------------------------ sparse states
@pytest.mark.parametrize("reach,library_run", [(1, True), (2, True), (2, False)])
def test_sparse_states(lsf, reach, library_run):
    """states initialised near the band only, on slices of 2.2 chunks with a partial last chunk: updates of 0.2 voxels stay
    inside either reach"""
    run = _case("far", BASE, dict(sparse_reach=reach, sparse_min_voxels=0, library_run=library_run))
    call = run.engine.last_call
    assert call.sparse_states and call.library_run == library_run and not run.engine.sparse_disabled
    assert len(run.engine._fast.bands) == 1
    _check_lists(run.engine._fast.bands, "far")


@pytest.mark.parametrize("reach", [1, 2])
def test_sparse_prepare_leaves_chunks_out_and_complete_fills_them(lsf, reach):
    from levelsetfusion_python_amd import device as dev
    canonical, live0 = _device("far")
    prepared = dev.StatePrepare(live0, canonical, sparse_reach=reach)
    bands, _ = prepared.collect()
    _check_lists(bands, "far")
    share = prepared.needed_fraction()
    print("sparse state initialisation of %s, reach %d: %.1f %% of the chunks" % (tuple(live0.shape), reach, 100.0 * share))
    assert 0.0 < share < 0.9
    # a chunk that holds band voxels is always needed: the band's chunks bound the share from below
    chunks = np.unique(np.concatenate(_numpy_lists("far")) // dev.StatePrepare.CHUNK)
    assert share >= len(chunks) / ((live0.numel() + dev.StatePrepare.CHUNK - 1) // dev.StatePrepare.CHUNK)
    whole = dev.state_pack(live0, None, prepared.grid, copies=1)[0]
    for st in prepared.states:
        prepared.complete(st, live0)
        assert torch.equal(st, whole)


@pytest.mark.parametrize("library_run", [True, False])
def test_updates_beyond_the_reach_fall_back(lsf, library_run):
    """`odd` moves 3.7 to 5 voxels per iteration: a call on states of reach 2 must notice, leave the caller's array alone,
    run again on full states and equal the oracle"""
    run = _case("odd", BASE, dict(sparse_reach=2, sparse_min_voxels=0, library_run=library_run))
    assert run.engine.sparse_disabled and not run.engine.last_call.sparse_states
    assert run.engine.last_call.library_run == library_run
    assert min(run.max_warps) >= 2.0


# ------------------------------------------------------------------------------------------ SobolevFusion
def _sobolev(taps):
    return dict(SOBOLEV, sobolev_kernel=_kernel(taps))


@pytest.mark.parametrize("taps", [3, 5, 7, 9])
def test_sobolev_float4_lists_on_odd_extents(lsf, taps):
    run = _case("odd", _sobolev(taps))
    call = run.engine.last_call
    assert not call.sobolev_boxes and not call.library_run
    assert run.engine._fast is not None and len(run.engine._fast.bands) == 2  # the float4 states and their lists
    _check_lists(run.engine._fast.bands, "odd")


@pytest.mark.parametrize("taps", [3, 5, 7, 9])
@pytest.mark.parametrize("how", ["library", "launches", "lists"])
def test_sobolev_on_three_different_extents(lsf, taps, how):
    """whole boxes: the library-enqueued call, the same launches made one by one, and the float4 lists without boxes"""
    options = {"library": None, "launches": dict(library_run=False), "lists": dict(sobolev_boxes=False)}[how]
    run = _case("fours", _sobolev(taps), options)
    call = run.engine.last_call
    assert call.sobolev_boxes == (how != "lists") and call.library_run == (how == "library")
    assert run.engine._fast is not None
    _check_lists(run.engine._fast.bands, "fours")


def test_sobolev_planar_with_eleven_taps(lsf):
    run = _case("odd", _sobolev(11))
    call = run.engine.last_call
    assert not call.sobolev_boxes and not call.library_run
    assert run.engine._fast is None  # no float4 states: planar fields


def test_sobolev_2d(lsf):
    run = _case("flat", _sobolev(7))
    call = run.engine.last_call
    assert not call.sobolev_boxes and not call.library_run
    assert run.engine._fast is not None and len(run.engine._fast.bands) == 2
    _check_lists(run.engine._fast.bands, "flat")


# ------------------------------------------------------------------------------------------ other configurations
@pytest.mark.parametrize("config", ["tikhonov", "thresholded_fdm", "no_level_set", "vectorized"])
def test_other_configurations(lsf, config):
    cfg = dict(BASE, **{"tikhonov": dict(smoothing_term_method=O.TIKHONOV),
                        "thresholded_fdm": dict(data_term_method=O.THRESHOLDED_FDM),
                        "no_level_set": dict(level_set_term_enabled=False),
                        "vectorized": dict(compute_method=O.VECTORIZED)}[config])
    run = _case("odd", cfg)
    assert run.engine.last_call.library_run and len(run.engine._fast.bands) == 2


# ------------------------------------------------------------------------------------------ a stop test that fires
@pytest.mark.parametrize("reach,library_run", [(0, True), (0, False), (2, True)])
def test_threshold_terminated(lsf, reach, library_run):
    """the lower threshold lies between the maxima of iterations 1 and 2 of a 12-iteration oracle probe: the call ends after
    three iterations, inside its first batch of four gated launches"""
    probe = np.float32(_oracle("far", dict(BASE, max_iterations=12, min_iterations=12)).log["max_warps"])
    k = next(i for i in range(2, len(probe)) if probe[i] < probe[:i].min())
    threshold = float((probe[:k].min() + probe[k]) / 2)
    cfg = dict(BASE, min_iterations=1, max_iterations=30, maximum_warp_length_lower_threshold=threshold)
    ref = _oracle("far", cfg, threshold)
    assert ref.iteration_count == k + 1 < 30
    run = _case("far", cfg, dict(sparse_reach=reach, sparse_min_voxels=0, library_run=library_run), check_interval=4,
                report_lower=threshold)
    assert run.iteration_count == k + 1 and len(run.max_warps) == k + 1
    call = run.engine.last_call
    assert call.library_run == library_run and call.sparse_states == bool(reach) and not run.engine.sparse_disabled


# ------------------------------------------------------------------------------------------ the drop-in classes
def _check_drop_in(opt, live, key, cfg):
    ref = _oracle(key, cfg, cfg["maximum_warp_length_lower_threshold"])
    assert maxdiff(live, ref.live) == EXACT
    assert maxdiff(opt.warp_field, ref.warp) == EXACT
    assert maxdiff(opt.gradient_field, ref.gradient) == EXACT
    assert np.array_equal(np.float32(opt.log.max_warps), np.float32(ref.log["max_warps"]))
    assert opt.log.max_warp_locations == [at[::-1] for at in ref.log["max_warp_locations"]]
    for mine, k in ((opt.log.data_energies, "data_energies"), (opt.log.smoothing_energies, "smoothing_energies"),
                    (opt.log.level_set_energies, "level_set_energies")):
        assert np.allclose(mine, ref.log[k], rtol=1e-9, atol=1e-12), k
    report = opt.get_convergence_report()
    assert report.iteration_count == ref.iteration_count == 4 and report.iteration_limit_reached
    _check_statistics(report.warp_delta_statistics, report.tsdf_difference_statistics, ref)
    call = opt.engine.last_call
    assert call.library_run and not call.box_walk and not call.sparse_states
    _check_lists(opt.engine._fast.bands, key)


GPU_KILLING = dict(level_set_term_enabled=True, gradient_descent_rate=0.1, data_term_weight=1.0, smoothing_term_weight=0.2,
                   isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2, maximum_warp_length_lower_threshold=0.0,
                   max_iterations=4, min_iterations=4)


@pytest.mark.parametrize("n", [27, 30])
def test_drop_in_3d_on_cubes_off_multiples_of_four(lsf, n):
    key = ((n, n, n), (0.3 * n, 0.36 * n, 0.27 * n))
    canonical, live0 = _pair(key)
    opt = lsf.SlavchevaOptimizer3d(field_size=n, compute_method=lsf.ComputeMethod.DIRECT,
                                   smoothing_term_method=lsf.SmoothingTermMethod.KILLING, **GPU_KILLING)
    live = live0.copy()
    assert opt.optimize(live, canonical.copy()) is live
    _check_drop_in(opt, live, key, BASE)


def test_drop_in_2d_on_an_odd_square(lsf, tmp_path):
    n = 45
    key = ((n, n), (0.3 * n, 0.36 * n))
    canonical, live0 = _pair(key)
    opt = lsf.SlavchevaOptimizer2d(out_path=str(tmp_path), field_size=n, compute_method=lsf.ComputeMethod.DIRECT,
                                   smoothing_term_method=lsf.SmoothingTermMethod.KILLING, **GPU_KILLING)
    live = live0.copy()
    assert opt.optimize(live, canonical.copy()) is live
    _check_drop_in(opt, live, key, BASE)


# ------------------------------------------------------------------------------------------ fields off 16-byte alignment
@pytest.mark.parametrize("how", ["library", "launches", "boxes", "sparse"])
def test_fields_one_float_into_a_buffer(lsf, how):
    """rows of a multiple of four voxels, but live and canonical start 4 bytes behind a 16-byte boundary: lsf_state_prepare
    must take its dword kernel (its 16-byte loads need aligned fields), and whatever reads the fields behind it must cope"""
    canonical_np, live_np = _pair("fours")
    n = canonical_np.size

    def offset(a):
        buffer = torch.empty(n + 8, dtype=torch.float32, device="cuda")
        view = buffer[1:1 + n].view(a.shape)
        view.copy_(torch.from_numpy(a.copy()))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return buffer, view
    (keep_c, canonical), (keep_l, live) = offset(canonical_np), offset(live_np)
    options = {"library": None, "launches": dict(library_run=False), "boxes": dict(box_walk=True),
               "sparse": dict(sparse_reach=2, sparse_min_voxels=0)}[how]
    run = _run_engine(canonical, live, BASE, options)  # (the finalize pass writes the offset view too)
    _check(run, _oracle("fours", BASE))
    eng = run.engine
    call = eng.last_call
    assert call.library_run == (how != "launches") and call.box_walk == (how == "boxes")
    assert eng.sparse_disabled == (how == "sparse")  # (updates of 2.4 to 3.8 voxels: the sparse attempt gives up)
    _check_lists(eng._fast.bands, "fours")
    del keep_c, keep_l
