"""Record rows (lsf_state_run::record_rows, engine_options record_rows): in a fixed-count library call every iteration
launch ends with one stored row per wave instead of its workgroup reduction and atomics, and ONE launch behind the last
iteration (records_from_rows_kernel) makes the records.  Each case runs the same call twice -- rows and atomics -- on the
same inputs and demands the same fields, maxima, arg-max locations and statistics bit for bit, the energies to 1e-9 of
each other and of the numpy oracle, and bit-identical energies from two consecutive row calls.  The shapes are the ways
the row ending can go wrong: more waves than units, two launches per iteration, 2-D, a BOUNDARY list alone, an empty
band, the box kernel, the sparse fall-back (the guard reads the records the reducer made), and a gated call, which must
keep the atomics.  Also: the used words and statistics the combine kernel now gathers, against the records themselves.
Reference loop: nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:354-388; report :393-404."""
import types

import numpy as np
import pytest
import torch

from oracle import lsf_oracle as O

import ragged_scene

pytestmark = pytest.mark.gpu

# the oracle's keywords: Killing + level set, DIRECT, no stop test
BASE = dict(compute_method=O.DIRECT, level_set_term_enabled=True, sobolev_smoothing_enabled=False,
            data_term_method=O.BASIC, smoothing_term_method=O.KILLING, gradient_descent_rate=0.1, data_term_weight=1.0,
            smoothing_term_weight=0.2, isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2,
            maximum_warp_length_lower_threshold=0.0, maximum_warp_length_upper_threshold=10000, sobolev_kernel=None)
ENERGIES = ("data_energies", "smoothing_energies", "level_set_energies")
DEPTH_HALF_WIDTH, DEPTH_SHIFT = 1.0, 4.0  # _depth_like_pair: voxels


@pytest.fixture(scope="module")
def lsf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import levelsetfusion_python_amd as pkg
    return pkg


def _cfg(iterations, **extra):
    return dict(BASE, max_iterations=iterations, min_iterations=iterations, **extra)


def _engine(cfg, options):
    from levelsetfusion_python_amd import _lib, engine
    return engine.SlavchevaEngine(
        True, cfg["level_set_term_enabled"], False, _lib.DATA_BASIC, _lib.SMOOTHING_KILLING, cfg["gradient_descent_rate"],
        cfg["data_term_weight"], cfg["smoothing_term_weight"], cfg["isomorphic_enforcement_factor"],
        cfg["level_set_term_weight"], cfg["maximum_warp_length_lower_threshold"], cfg["maximum_warp_length_upper_threshold"],
        cfg["max_iterations"], cfg["min_iterations"], None, options=options)


def _run(canonical, live0, cfg, rows, eng=None, **options):
    """one library-enqueued call of engine.SlavchevaEngine with the row ending on or off: what it leaves behind"""
    from levelsetfusion_python_amd import device as dev
    if eng is None:
        eng = _engine(cfg, dict(dict(sparse_reach=0, sparse_min_voxels=0), record_rows=rows, **options))
    live = live0.clone()
    outcome = eng.optimize(live, canonical, finalize=(live, 0.0, True))
    final, warp, raw = outcome.finalize(live, 0.0, True)
    assert final is live and eng.last_call.library_run
    warp = warp() if callable(warp) else warp
    return types.SimpleNamespace(
        engine=eng, live=live, warp=warp, gradient=dev.interleave(eng.gradient_field()), raw=np.array(raw),
        max_warps=np.float32(eng.log["max_warps"]), indices=list(eng.log["max_warp_indices"]),
        energies=[np.float64(eng.log[k]) for k in ENERGIES], bands=eng._fast.bands)


def _oracle_energies(canonical, live0, cfg):
    o = O.SlavchevaOracle(**cfg)
    live = live0.cpu().numpy().copy()
    o.optimize(live, canonical.cpu().numpy())
    return [np.float64(o.log[k]) for k in ENERGIES]


def _rows_equal_atomics(canonical, live0, cfg, oracle=True, **options):
    """rows == atomics (fields, maxima, locations, statistics: bits; energies: 1e-9), == oracle (energies), rows == rows"""
    a = _run(canonical, live0, cfg, True, **options)
    b = _run(canonical, live0, cfg, False, **options)
    assert a.engine.last_call.record_rows and not b.engine.last_call.record_rows, "the call took the other ending"
    assert torch.equal(a.live, b.live), "caller's live field"
    assert torch.equal(a.warp, b.warp), "warp field (the final state at every listed voxel)"
    assert torch.equal(a.gradient, b.gradient), "gradient field"
    assert np.array_equal(a.max_warps.view(np.uint32), b.max_warps.view(np.uint32)), "maxima, bit for bit"
    assert a.indices == b.indices, "arg-max locations"
    assert np.array_equal(a.raw.view(np.uint64), b.raw.view(np.uint64)), "the 16 convergence statistics"
    for x, y, key in zip(a.energies, b.energies, ENERGIES):
        print(key, "rows vs atomics: max relative difference %.3e" % float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))))
        assert np.allclose(x, y, rtol=1e-9, atol=0.0), key
    if oracle:
        for x, y, key in zip(a.energies, _oracle_energies(canonical, live0, cfg), ENERGIES):
            print(key, "rows vs oracle: max relative difference %.3e" % float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))))
            assert np.allclose(x, y, rtol=1e-9, atol=0.0), key
    # a fixed association: the same call again (the same optimizer, then a fresh one) logs the same bits
    again = _run(canonical, live0, cfg, True, eng=a.engine)
    fresh = _run(canonical, live0, cfg, True, **options)
    for x, y, z in zip(a.energies, again.energies, fresh.energies):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(x.view(np.uint64), z.view(np.uint64))
    assert np.array_equal(a.max_warps, again.max_warps) and a.indices == again.indices
    return a, b


def _sphere_pair_r03(n):
    from levelsetfusion_python_amd.synthetic import sphere_pair
    return sphere_pair(n, 3, "cuda")  # r = 0.3 n


def test_fewer_units_than_waves_32(lsf):
    """32^3 sphere pair (r = 0.3 n), six iterations: the lists are no more 64-entry units than their launches have waves (the
    ten-voxel band reaches the faces: a BOUNDARY list of a few units rides along) -- waves store zero rows, and workgroups
    of the XCDs whose share of the units is short have no unit at all"""
    canonical, live0 = _sphere_pair_r03(32)
    a, _ = _rows_equal_atomics(canonical, live0, _cfg(6))
    assert a.bands[0].count > 0 and not a.engine.last_call.box_walk
    assert sum((band.count + 63) // 64 for band in a.bands) <= 32 ** 3 // 64 + 2  # (512 units for up to 4096 waves)
    assert a.max_warps.min() > 0.0


def test_two_launches_per_iteration_band_cut_by_a_face(lsf):
    """40 x 36 x 44 with the ellipsoid cut by the x faces, five iterations: an INTERIOR and a BOUNDARY list, two launches and
    two row blocks per iteration, the arg-max (and its tie rule) taken across them"""
    canonical, live0 = (torch.from_numpy(f).cuda() for f in ragged_scene.pair((40, 36, 44), semi=(24.0, 12.0, 10.0)))
    a, _ = _rows_equal_atomics(canonical, live0, _cfg(5))
    assert len(a.bands) == 2 and all(band.count for band in a.bands)


def test_2d_interior_band(lsf):
    canonical, live0 = (torch.from_numpy(f).cuda() for f in ragged_scene.pair((48, 48), semi=(12.0, 10.0)))
    a, _ = _rows_equal_atomics(canonical, live0, _cfg(5))
    assert len(a.bands) == 1 and a.bands[0].count > 0


def test_2d_boundary_list_alone(lsf):
    """the band is a stretch of the row y = 0 and of the column x = 47: every band voxel lies on a face, no INTERIOR list"""
    canonical = torch.ones((48, 48), device="cuda")
    live0 = torch.ones((48, 48), device="cuda")
    live0[0, 5:40] = torch.linspace(-0.8, 0.7, 35, device="cuda")
    live0[10:30, 47] = torch.linspace(0.6, -0.5, 20, device="cuda")
    a, _ = _rows_equal_atomics(canonical, live0, _cfg(5))
    from levelsetfusion_python_amd import _lib
    assert len(a.bands) == 1 and a.bands[0].count == 55 and a.bands[0].subset == _lib.BAND_BOUNDARY
    assert a.max_warps.max() > 0.0


def test_empty_band(lsf):
    """both fields truncated everywhere: one launch over an empty BOUNDARY list still yields the record "length 0, first
    voxel" of an all-zero update"""
    canonical = torch.ones((32, 32, 32), device="cuda")
    live0 = -torch.ones((32, 32, 32), device="cuda")
    a, _ = _rows_equal_atomics(canonical, live0, _cfg(3))
    assert a.max_warps.tolist() == [0.0, 0.0, 0.0] and a.indices == [0, 0, 0]
    assert all(float(np.abs(e).max()) == 0.0 for e in a.energies)


def test_box_kernel_row_ending_32(lsf):
    canonical, live0 = _sphere_pair_r03(32)
    a, b = _rows_equal_atomics(canonical, live0, _cfg(6), box_walk=True)
    assert a.engine.last_call.box_walk and b.engine.last_call.box_walk
    # ... and the box walk's rows are the list walk's results
    c = _run(canonical, live0, _cfg(6), True, box_walk=False)
    assert torch.equal(a.live, c.live) and np.array_equal(a.max_warps, c.max_warps) and a.indices == c.indices


def test_sparse_fall_back_sees_the_records_in_time(lsf):
    """tests/test_gpu_sparse_state.py's fall-back scene at its size (128^3 sphere pair, rate 20, four iterations): the first
    update is beyond the reach of two voxels.  The finalize guard reads records the reducer launch made: the attempt on
    sparse states must leave the caller's array untouched and report the excess; the repeat equals the atomics' result"""
    from levelsetfusion_python_amd.engine_run import _SparseStateExceeded
    canonical, live0 = _sphere_pair_r03(128)
    cfg = _cfg(4, **{"gradient_descent_rate": 20.0})
    options = dict(sparse_reach=2, sparse_min_voxels=0)
    eng = _engine(cfg, dict(options, record_rows=True))
    live = live0.clone()
    with pytest.raises(_SparseStateExceeded):
        eng._optimize(live, canonical, (live, 0.0, True))
    assert eng.last_call.record_rows and eng.last_call.sparse_states
    assert torch.equal(live, live0), "the guard must have kept the finalize pass from the caller's array"
    a = _run(canonical, live0, cfg, True, **options)
    b = _run(canonical, live0, cfg, False, **options)
    assert a.engine.sparse_disabled and b.engine.sparse_disabled and a.max_warps.max() > 2.0
    assert a.engine.last_call.record_rows and not a.engine.last_call.sparse_states
    assert torch.equal(a.live, b.live) and torch.equal(a.warp, b.warp)
    assert np.array_equal(a.max_warps, b.max_warps) and a.indices == b.indices
    assert np.array_equal(a.raw.view(np.uint64), b.raw.view(np.uint64))
    for x, y in zip(a.energies, b.energies):
        assert np.allclose(x, y, rtol=1e-9, atol=0.0)


def _depth_like_pair(n, half_width=DEPTH_HALF_WIDTH, shift=DEPTH_SHIFT):
    """a depth-like pair: the TSDF of a tilted, gently bumped surface z = s(x, y), truncated `half_width` voxels around it, and
    of the same surface `shift` voxels nearer -- steep enough (the defaults' update is rate x difference x slope) that the
    default loop's 0.1-voxel threshold holds for dozens of iterations"""
    ax = torch.arange(n, dtype=torch.float64, device="cuda")
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    surface = 0.55 * n + 0.05 * (xx - n / 2) - 0.03 * (yy - n / 2) + 1.5 * torch.sin(xx / 5.0) * torch.cos(yy / 7.0)
    def tsdf(s):
        return torch.clamp((zz - s) / half_width, -1.0, 1.0).to(torch.float32).contiguous()
    return tsdf(surface), tsdf(surface - shift)


def test_default_constructor_keeps_the_atomics(lsf):
    """the default loop (min 1, max 100, lower threshold 0.1) on a 32^3 depth-like pair runs past the first batch of
    check_interval gated launches: the next launch's gate and the host read the records between launches, so the call keeps
    the atomics whatever record_rows says -- and equals the call made launch by launch"""
    canonical, live0 = _depth_like_pair(32)
    runs = []
    for library_run in (True, False):
        opt = lsf.SlavchevaOptimizer3d(field_size=32, engine_options=dict(library_run=library_run))
        assert opt.engine.record_rows is True
        live = live0.clone()
        opt.optimize(live, canonical)
        assert opt.engine.last_call.library_run == library_run and opt.engine.last_call.record_rows is False
        runs.append((opt, live))
    (oa, la), (ob, lb) = runs
    n = len(oa.log.max_warps)
    assert n > oa.engine.check_interval, "the scene must run past the first batch (%d iterations)" % n
    assert torch.equal(la, lb) and torch.equal(torch.as_tensor(oa.warp_field), torch.as_tensor(ob.warp_field))
    assert np.array_equal(np.float32(oa.log.max_warps), np.float32(ob.log.max_warps))
    assert oa.log.max_warp_locations == ob.log.max_warp_locations
    for key in ENERGIES:
        assert np.allclose(getattr(oa.log, key), getattr(ob.log, key), rtol=1e-9, atol=0.0)
    assert oa.get_convergence_report() == ob.get_convergence_report()


def test_rows_buffer_is_sized_by_the_library_and_checked(lsf):
    """lsf_state_run_rows_elements grows with iterations and launches per iteration, is 0 for arguments that make no call,
    and lsf_state_run_finish refuses a smaller buffer before it launches anything"""
    import ctypes
    from levelsetfusion_python_amd import _lib, device as dev
    grid = dev.full_range(dev.make_grid((32, 32, 32)))
    f = _lib.lib.lsf_state_run_rows_elements
    one, two = f(ctypes.byref(grid), 1, 1), f(ctypes.byref(grid), 1, 2)
    assert one > 0 and one % 4 == 0 and two > one and f(ctypes.byref(grid), 7, 2) == 7 * two
    assert f(ctypes.byref(grid), 0, 1) == 0 and f(ctypes.byref(grid), 1, 3) == 0 and f(ctypes.byref(grid), 1, 0) == 0
    canonical, live0 = _sphere_pair_r03(32)
    eng = _engine(_cfg(3), dict(sparse_reach=0, sparse_min_voxels=0))
    real = _lib.lib.lsf_state_run_finish_rows
    seen = []

    def short(*args):
        args = list(args)
        # what the engine sized the buffer to (the 32^3 band reaches the faces: two launches per iteration)
        assert args[17] == f(ctypes.byref(grid), 3, 2)
        args[17] -= 4  # one row short of what the library asks for
        seen.append(real(*args))
        return seen[-1]
    live = live0.clone()
    try:
        _lib.lib.lsf_state_run_finish_rows = short
        with pytest.raises(_lib.LsfHipError):
            eng.optimize(live, canonical, finalize=(live, 0.0, True))
    finally:
        _lib.lib.lsf_state_run_finish_rows = real
    torch.cuda.synchronize()
    assert seen == [-1] and torch.equal(live, live0)


def _prologue_restatement(canonical, live, reach):
    """numpy: what lsf_state_run_begin leaves behind -- the two exclusive prefix arrays of the per-chunk INTERIOR / BOUNDARY
    band counts, the four totals, and lsf_state_pack_needed's verdicts (1024-voxel chunks; its (dz, dy) loop and candidates)"""
    shape, n = canonical.shape, canonical.size
    chunks = (n + 1023) // 1024
    truncated = (np.abs(live) == 1.0) & (np.abs(canonical) == 1.0)
    inner = np.zeros(shape, dtype=bool)
    inner[(slice(1, -1),) * canonical.ndim] = True
    pad = chunks * 1024 - n

    def per_chunk(mask):
        return np.concatenate([mask.ravel(), np.zeros(pad, dtype=bool)]).reshape(chunks, 1024).sum(axis=1)
    counts = [per_chunk(~truncated & inner), per_chunk(~truncated & ~inner)]
    prefix = [np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int32) for c in counts]
    opposite = np.flatnonzero((truncated & (live == -canonical)).ravel())
    totals = [int(counts[0].sum()), int(counts[1].sum()), int(opposite.size), int(opposite[0]) if opposite.size else -1]
    nonempty = (counts[0] + counts[1]) > 0
    row, plane = shape[-1], shape[-1] * shape[-2]
    needed = np.zeros(chunks, dtype=np.int32)
    for c in range(chunks):
        for dz in (range(-reach, reach + 1) if canonical.ndim == 3 else (0,)):
            for dy in range(-reach, reach + 1):
                lo = c * 1024 + dz * plane + dy * row - reach
                hi = c * 1024 + 1023 + dz * plane + dy * row + reach
                first, last = max(lo // 1024, 0), min(hi // 1024, chunks - 1)  # (floor division, also of negatives)
                if first <= last and nonempty[first:last + 1].any():
                    needed[c] = 1
    return chunks, prefix, totals, needed


@pytest.mark.parametrize("scene", ["sphere32", "sphere64", "odd"])
def test_prologue_in_fewer_launches_leaves_the_same_words(lsf, scene):
    """lsf_state_run_begin with the fifth total written by the scan (no memset launch) and the chunk verdicts formed inside
    the pack kernel (no launch of their own), against a numpy restatement: the scratch prefix arrays, the five totals (the
    fifth, the number of boxes, 0), the `needed` verdicts, and the chunks written -- both states (live, 0) exactly in the
    needed chunks, untouched elsewhere.  32^3, 64^3, and 21 x 30 x 37: 23 chunks, the last one partial, no extent a multiple
    of 4 (the narrow counting kernel)"""
    import ctypes
    from levelsetfusion_python_amd import _lib, device as dev
    if scene == "odd":
        canonical, live = (torch.from_numpy(f).cuda() for f in ragged_scene.scene("odd"))
    else:
        canonical, live = _sphere_pair_r03(int(scene[6:]))
    reach = 2
    grid = dev.full_range(dev.make_grid(tuple(live.shape)))
    n = live.numel()
    chunks, prefix, totals, needed = _prologue_restatement(canonical.cpu().numpy(), live.cpu().numpy(), reach)
    states = [torch.full(tuple(live.shape) + (4,), float("nan"), device="cuda") for _ in range(2)]
    scratch = torch.full((int(_lib.lib.lsf_state_prepare_scratch_elements(ctypes.byref(grid))),), -7, dtype=torch.int32,
                         device="cuda")
    totals_device = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    totals_host = torch.full((5,), -7, dtype=torch.int64).pin_memory()
    run = _lib.StateRun()
    run.live, run.canonical = live.data_ptr(), canonical.data_ptr()
    run.state[0], run.state[1] = states[0].data_ptr(), states[1].data_ptr()
    run.prepare_scratch, run.totals_device, run.totals_host = scratch.data_ptr(), totals_device.data_ptr(), totals_host.data_ptr()
    run.grid, run.sparse_reach = grid, reach
    _lib.check(_lib.lib.lsf_state_run_begin(ctypes.byref(run), dev.stream_ptr()), "lsf_state_run_begin")
    assert totals_host.tolist() == totals + [0]
    torch.cuda.synchronize()
    words = scratch.cpu().numpy()
    assert np.array_equal(words[:chunks], prefix[0]) and np.array_equal(words[chunks + 1:2 * chunks + 1], prefix[1])
    at = 2 * (chunks + 1) + 64 * chunks + 2 * chunks + chunks  # lsf_slavcheva.hip::prepare_needed
    assert np.array_equal(words[at:at + chunks], needed) and 0 < needed.sum()
    want = torch.zeros((n, 4), device="cuda")
    want[:, 0] = live.reshape(-1)
    written = torch.from_numpy(np.repeat(needed.astype(bool), 1024)[:n]).cuda()
    for state in states:
        flat = state.reshape(n, 4)
        assert torch.equal(flat[written], want[written]), "the needed chunks hold (live, 0)"
        assert bool(torch.isnan(flat[~written]).all()), "every other chunk is left alone"


@pytest.mark.parametrize("rows", [True, False])
def test_used_words_and_statistics_come_from_the_combine_kernel(lsf, rows):
    """the finalize pass's one-block combine kernel gathers the records' used words and the 16 statistics for the call's one
    copy to the host (no records_used_words_kernel launch at the end of a call): words_host against the records themselves
    and against the statistics buffer, with rows and with atomics"""
    from levelsetfusion_python_amd import _lib, device as dev
    canonical, live0 = _sphere_pair_r03(32)
    run = _run(canonical, live0, _cfg(6), rows)
    records = run.engine._fast.records
    n_words = 6 * _lib.RECORD_SLOTS * dev.USED_SLOT_WORDS + 16
    words = dev.pinned_scratch("run records", n_words, torch.int64).numpy()[:n_words].copy()  # (the call's landing place)
    slots = records.view(torch.int64).reshape(6 * _lib.RECORD_SLOTS, -1)[:, :dev.USED_SLOT_WORDS].cpu().numpy()
    assert np.array_equal(words[:-16].reshape(slots.shape), slots)
    assert np.array_equal(words[-16:], run.raw.view(np.int64))
    if rows:  # the reducer: everything in slot 0, zeros in the other seven
        per_record = slots.reshape(6, _lib.RECORD_SLOTS, dev.USED_SLOT_WORDS)
        assert (per_record[:, 0, 0] != 0).all() and not per_record[:, 1:].any()
