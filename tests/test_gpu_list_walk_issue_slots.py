"""The INTERIOR list walk after its issue-slot diet (csrc/lsf_slavcheva_state.hip, lsf_device.h): the energy select on the
float32 value, the slice test behind the wave-uniform Grid::e_all, no row test in walks that are not cut along y, and
the row ending whose four DPP reductions run side by side and are stored by lane 63.  None of that may
move a bit of a state, a maximum, a location or a statistic, nor an energy beyond 1e-9:

- both voxel decodes (shifts at 32^3, two multiply-high divisions at 24 x 40 x 48) against the numpy ORACLE, 8 iterations;
- the list walk against the dense tile walk of the same engine on all-in-band random fields, at sizes where the waves of a
  launch get 0 or 1 (16^3, 48^3), 1 or 2 (64 x 64 x 80) and 3 or more (96^3) wave-units;
- two consecutive row calls: the same energy bits;
- an energy slice range: it cuts the energies, exactly to the voxels of its slices, and nothing else.
Reference loop: nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:238-330, :354-388."""
import types

import numpy as np
import pytest
import torch

from oracle import lsf_oracle as O

import ragged_scene

pytestmark = pytest.mark.gpu

# the oracle's keywords: Killing + level set, DIRECT energies, no stop test
BASE = dict(compute_method=O.DIRECT, level_set_term_enabled=True, sobolev_smoothing_enabled=False,
            data_term_method=O.BASIC, smoothing_term_method=O.KILLING, gradient_descent_rate=0.1, data_term_weight=1.0,
            smoothing_term_weight=0.2, isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2,
            maximum_warp_length_lower_threshold=0.0, maximum_warp_length_upper_threshold=10000, sobolev_kernel=None)
ENERGIES = ("data_energies", "smoothing_energies", "level_set_energies")
FULL_STATES = dict(sparse_reach=0, sparse_min_voxels=0)


@pytest.fixture(scope="module")
def lsf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import levelsetfusion_python_amd as pkg
    return pkg


def _cfg(iterations):
    return dict(BASE, max_iterations=iterations, min_iterations=iterations)


def _run(canonical, live0, cfg, **options):
    """one call of engine.SlavchevaEngine on device tensors: what it leaves behind"""
    from levelsetfusion_python_amd import _lib, device as dev, engine
    eng = engine.SlavchevaEngine(
        True, cfg["level_set_term_enabled"], False, _lib.DATA_BASIC, _lib.SMOOTHING_KILLING, cfg["gradient_descent_rate"],
        cfg["data_term_weight"], cfg["smoothing_term_weight"], cfg["isomorphic_enforcement_factor"],
        cfg["level_set_term_weight"], cfg["maximum_warp_length_lower_threshold"], cfg["maximum_warp_length_upper_threshold"],
        cfg["max_iterations"], cfg["min_iterations"], None, options=options)
    live = live0.clone()
    outcome = eng.optimize(live, canonical, finalize=(live, 0.0, True))
    final, warp, raw = outcome.finalize(live, 0.0, True)
    assert final is live
    warp = warp() if callable(warp) else warp
    return types.SimpleNamespace(
        engine=eng, live=live, warp=warp, gradient=dev.interleave(eng.gradient_field()), raw=np.array(raw),
        max_warps=np.float32(eng.log["max_warps"]), indices=[int(i) for i in eng.log["max_warp_indices"]],
        energies=[np.float64(eng.log[k]) for k in ENERGIES], bands=eng._fast.bands)


def _interior(bands):
    from levelsetfusion_python_amd import _lib
    found = [b for b in bands if b.subset == _lib.BAND_INTERIOR]
    assert len(found) == 1 and found[0].count > 0, "the scene must have an INTERIOR list"
    return found[0]


def _close(mine, want, key):
    worst = float(np.max(np.abs(mine - want) / np.maximum(np.abs(want), 1e-300)))
    print("%s: max relative difference %.3e" % (key, worst))
    assert np.allclose(mine, want, rtol=1e-9, atol=0.0), key


# ------------------------------------------------------------------------------------------ both decodes, against the oracle
@pytest.mark.parametrize("shape,semi", [((32, 32, 32), (9.0, 8.0, 7.0)), ((24, 40, 48), (14.0, 11.0, 6.0))],
                         ids=["32_shifts", "24x40x48_divisions"])
def test_decode_paths_against_the_oracle(lsf, shape, semi):
    """rows and slices of a power of two (x, y, z by shifts and masks) and of 48 and 40 voxels (two divisions by multiply-
    high): the fixed-count library call with the row ending, 8 iterations, against the oracle -- live, warp and gradient
    fields, maxima and their locations bit for bit, the energies to 1e-9"""
    canonical_np, live_np = ragged_scene.pair(shape, semi=semi)
    power_of_two = all(n & (n - 1) == 0 for n in shape[1:])
    assert power_of_two == (shape == (32, 32, 32))
    cfg = _cfg(8)
    oracle = O.SlavchevaOracle(**cfg)
    live_ref = live_np.copy()
    oracle.optimize(live_ref, canonical_np)
    run = _run(torch.from_numpy(canonical_np).cuda(), torch.from_numpy(live_np).cuda(), cfg, **FULL_STATES)
    call = run.engine.last_call
    assert call.library_run and call.record_rows and not call.box_walk and not call.sparse_states
    _interior(run.bands)
    assert np.array_equal(run.live.cpu().numpy(), live_ref), "live field"
    assert np.array_equal(run.warp.cpu().numpy(), oracle.warp_field), "warp field"
    assert np.array_equal(run.gradient.cpu().numpy(), oracle.gradient_field), "gradient field"
    assert np.array_equal(run.max_warps.view(np.uint32), np.float32(oracle.log["max_warps"]).view(np.uint32))
    assert [tuple(int(i) for i in np.unravel_index(at, shape)) for at in run.indices] == oracle.log["max_warp_locations"]
    assert run.max_warps.min() > 0.0
    for mine, key in zip(run.energies, ENERGIES):
        _close(mine, np.float64(oracle.log[key]), key)


# ------------------------------------------------------------------------------------------ unit counts per wave
def _all_in_band_pair(shape):
    """every voxel in the band (|values| < 1), smooth enough that the updates stay well below a voxel"""
    generator = torch.Generator(device="cpu").manual_seed(1000 + sum(shape))
    canonical = 0.3 * (torch.rand(shape, generator=generator) - 0.5)
    live = canonical + 0.06 * (torch.rand(shape, generator=generator) - 0.5)
    return canonical.cuda().contiguous(), live.cuda().contiguous()


@pytest.mark.parametrize("shape", [(16, 16, 16), (48, 48, 48), (80, 64, 64), (96, 96, 96)],
                         ids=["16", "48", "64x64x80", "96"])
def test_list_walk_equals_dense_walk(lsf, shape):
    """all-in-band random fields, 5 iterations: the INTERIOR list is every voxel off the faces -- 43, 1521, 4685 and 12978
    wave-units for launches of 48, 1536, 4096 and 4096 waves, i.e. waves with 0 or 1, 0 or 1, 1 or 2 and 3 or more trips of
    the walk's loop; none of the lists is a multiple of 64 entries (the last unit is partial).  Against the dense tile walk of
    the same engine, which shares neither the loop nor the row ending: states and maxima identical, energies to 1e-9"""
    canonical, live0 = _all_in_band_pair(shape)
    cfg = _cfg(5)
    listed = _run(canonical, live0, cfg, **FULL_STATES)
    dense = _run(canonical, live0, cfg, use_band_list=False)
    assert listed.engine.last_call.library_run and listed.engine.last_call.record_rows
    assert not dense.engine.last_call.library_run and dense.bands[0].indices is None
    interior = _interior(listed.bands)
    nz, ny, nx = shape
    assert interior.count == (nz - 2) * (ny - 2) * (nx - 2) and interior.count % 64 != 0
    assert len(listed.bands) == 2  # ... and the faces ride along in a BOUNDARY list
    assert torch.equal(listed.live, dense.live), "live field"
    assert torch.equal(listed.warp, dense.warp), "warp field"
    assert torch.equal(listed.gradient, dense.gradient), "gradient field"
    assert np.array_equal(listed.max_warps.view(np.uint32), dense.max_warps.view(np.uint32)), "maxima, bit for bit"
    assert listed.indices == dense.indices, "arg-max locations"
    assert listed.max_warps.min() > 0.0
    assert np.array_equal(listed.raw.view(np.uint64)[[0, 1, 2, 5, 8, 9, 10, 13]],
                          dense.raw.view(np.uint64)[[0, 1, 2, 5, 8, 9, 10, 13]]), "counts, extrema and locations"
    for mine, want, key in zip(listed.energies, dense.energies, ENERGIES):
        _close(mine, want, key)


# ------------------------------------------------------------------------------------------ a fixed association
def test_two_row_calls_log_the_same_energy_bits(lsf):
    """two consecutive fixed-count library calls at 32^3 with record_rows=True: every wave's sums are reduced in a fixed order
    and combined in a fixed order, so the logged energies are the same bits"""
    from levelsetfusion_python_amd.synthetic import sphere_pair
    canonical, live0 = sphere_pair(32, 3, "cuda")
    first = _run(canonical, live0, _cfg(6), record_rows=True, **FULL_STATES)
    second = _run(canonical, live0, _cfg(6), record_rows=True, **FULL_STATES)
    assert first.engine.last_call.record_rows and second.engine.last_call.record_rows
    for a, b, key in zip(first.energies, second.energies, ENERGIES):
        assert a.max() > 0.0, key  # (the warp starts at zero: the first iteration's smoothing energy is 0)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), key
    assert np.array_equal(first.max_warps.view(np.uint32), second.max_warps.view(np.uint32))
    assert first.indices == second.indices and torch.equal(first.live, second.live)


# ------------------------------------------------------------------------------------------ the energy slice range
def test_energy_slice_range_cuts_the_energies(lsf):
    """lsf_grid::energy_z_begin / _end (what a z-slab sets so that its recomputed halo slices are not counted twice) on ONE
    launch of the INTERIOR kernel at 32^3 -- no process group needed to reach the kernel's test.  The ending is the
    records' (atomics), as with record_rows=False.  A range of slices must count exactly the voxels of those slices (the
    launch over the list cut to them), an explicit whole range must count what no range counts (Grid::e_all either way),
    and the range must touch nothing but the energies"""
    from levelsetfusion_python_amd import device as dev
    canonical_np, live_np = ragged_scene.pair((32, 32, 32), semi=(9.0, 8.0, 7.0))
    canonical, live = torch.from_numpy(canonical_np).cuda(), torch.from_numpy(live_np).cuda()
    params = lsf.SlavchevaOptimizer3d(field_size=32, compute_method=lsf.ComputeMethod.DIRECT, level_set_term_enabled=True,
                                      smoothing_term_method=lsf.SmoothingTermMethod.KILLING).engine.params
    grid = dev.make_grid((32, 32, 32))
    band = _interior(dev.band_lists(live, canonical, grid))
    z = band.indices[:band.count] // (32 * 32)
    lo, hi = 12, 19
    inside = band.indices[:band.count][(z >= lo) & (z < hi)].contiguous()
    assert 0 < inside.numel() < band.count and int(z.min()) < lo and int(z.max()) >= hi

    # the launches under test are second iterations: the warp of the first one gives them a smoothing energy
    start = dev.state_pack(live, None, grid)
    dev.slavcheva_state_iteration(start[0], canonical, start[1], grid, params, None, dev.new_records(1, "cuda"), 0, band)

    def launch(g, b):
        records = dev.new_records(1, "cuda")
        out = start[0].clone()
        dev.slavcheva_state_iteration(start[1], canonical, out, g, params, None, records, 0, b)
        host = dev.decode_records(dev.records_to_host(records))
        energies = np.float64([host[k][0] for k in ("data_energy", "smoothing_energy", "level_set_energy")])
        return out, np.float32(host["max_value"][0]), int(host["argmax"][0]), energies

    def ranged(first, last):
        g = dev.Grid.from_buffer_copy(grid)
        g.energy_z_begin, g.energy_z_end = first, last
        return g
    whole = launch(grid, band)
    cut = launch(ranged(lo, hi), band)
    explicit = launch(ranged(0, 32), band)
    only = launch(grid, dev.BandList(inside, inside.numel(), band.subset))
    assert whole[3].min() > 0.0
    for key, mine, want in zip(ENERGIES, cut[3], only[3]):
        _close(mine, want, key + ", slices [12, 19)")
    assert np.all(cut[3] < 0.9 * whole[3]), "the range must cut the energies"
    for key, mine, want in zip(ENERGIES, explicit[3], whole[3]):
        _close(mine, want, key + ", slices [0, 32)")
    for other in (cut, explicit):
        assert torch.equal(other[0], whole[0]), "the new state does not depend on the range"
        assert other[1].view(np.uint32) == whole[1].view(np.uint32) and other[2] == whole[2]
