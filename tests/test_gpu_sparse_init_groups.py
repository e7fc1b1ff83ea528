"""The sparse state initialisation per GROUP of 32 consecutive voxels (lsf_state_pack_needed): the
verdicts come from the band ballots the counting pass keeps, a bit per group in the int32 kept per 1024-voxel chunk.
(Sixteen-voxel groups need 64 bits per chunk; tests/test_cabi_and_host.py pins the scratch size, so the groups are 32.)
Against a numpy restatement of the verdict -- a band bit in [32 q + dz * slice + dy * row - reach, 32 q + 31 + dz * slice +
dy * row + reach] for some |dy|, |dz| <= reach, the run cut to the array -- on NaN-poisoned states: exactly the needed groups
are written, they hold (live, 0, 0, 0), every voxel within Chebyshev distance `reach` of a band voxel is among them, and
invert = 1 writes exactly the rest.  Shapes: rows that are no multiple of 32 in a volume that is no multiple of 1024 voxels
(the narrow counting kernel), a 2-D field, 64^3 (the 16-byte counting kernel); bands that touch the first and the last
voxel of the array.  End to end: a 48^3 call on such states against fully initialised ones, bit for bit, list walk and box
walk, and with updates that outrun the reach.
Arrays below 2^21 voxels keep whole 1024-voxel chunks by default (tests/test_gpu_record_rows.py holds the prologue to that at
its sizes), so every test here but the last runs with LSF_SPARSE_MIN_VOXELS = 0, groups at every size; the last one
holds the default: chunks below the limit, and the same group code at 128^3, the first size above it.
Reference loop: nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:238-330, :360-362."""
import numpy as np
import pytest
import torch

import ragged_scene

pytestmark = pytest.mark.gpu

GROUP, CHUNK = 32, 1024
KILLING = dict(level_set_term_enabled=True, gradient_descent_rate=0.1, data_term_weight=1.0, smoothing_term_weight=0.2,
               isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2, maximum_warp_length_lower_threshold=0.0)


@pytest.fixture(scope="module")
def lsf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import levelsetfusion_python_amd as pkg
    return pkg


@pytest.fixture
def groups_everywhere(monkeypatch):
    monkeypatch.setenv("LSF_SPARSE_MIN_VOXELS", "0")


def _scene(name):
    """(canonical, live) numpy float32; `-ends`: the band touches the first and the last voxel of the array"""
    base = name.split("-")[0]
    if base == "ragged3d":  # rows of 70 voxels, 78 540 voxels = 76.7 chunks
        canonical, live = ragged_scene.pair((33, 34, 70), semi=(22.0, 10.0, 9.5))
    elif base == "field2d":  # rows of 130 voxels, 9 100 voxels = 8.9 chunks
        canonical, live = ragged_scene.pair((70, 130), semi=(40.0, 20.0))
    else:
        from levelsetfusion_python_amd.synthetic import sphere_pair
        canonical, live = (f.numpy() for f in sphere_pair(64, 3, "cpu"))
    canonical, live = np.ascontiguousarray(canonical, np.float32), np.array(live, np.float32)
    if name.endswith("-ends"):
        live.reshape(-1)[0] = 0.25
        live.reshape(-1)[-1] = -0.5
    return canonical, live


def _band(canonical, live):
    return ~((np.abs(live) == 1.0) & (np.abs(canonical) == 1.0))


def group_verdicts(band, reach):
    """the restatement: bool per group of 32 linear voxels, 32 groups per 1024-voxel chunk"""
    shape, n = band.shape, band.size
    chunks = (n + CHUNK - 1) // CHUNK
    row, plane = shape[-1], shape[-1] * shape[-2]
    bits = np.concatenate([band.ravel(), np.zeros(chunks * CHUNK - n, dtype=bool)])
    before = np.concatenate([[0], np.cumsum(bits)])
    first = GROUP * np.arange(chunks * (CHUNK // GROUP), dtype=np.int64)
    needed = np.zeros(first.size, dtype=bool)
    for dz in (range(-reach, reach + 1) if band.ndim == 3 else (0,)):
        for dy in range(-reach, reach + 1):
            lo = np.maximum(first + dz * plane + dy * row - reach, 0)
            hi = np.minimum(first + GROUP - 1 + dz * plane + dy * row + reach, chunks * CHUNK - 1)
            inside = lo <= hi
            needed[inside] |= before[hi[inside] + 1] > before[lo[inside]]
    return needed


def within_reach(band, reach):
    """voxels within Chebyshev distance `reach` of a band voxel (no wrap-around)"""
    out = band.copy()
    for axis in range(band.ndim):
        src = out.copy()
        for d in range(1, reach + 1):
            lo = [slice(None)] * band.ndim
            hi = [slice(None)] * band.ndim
            lo[axis], hi[axis] = slice(d, None), slice(None, -d)
            out[tuple(lo)] |= src[tuple(hi)]
            out[tuple(hi)] |= src[tuple(lo)]
    return out


_CACHE = {}


def _case(name, reach):
    """scene, restatement and what the device left behind: computed once per (scene, reach), read by the tests"""
    key = (name, reach)
    if key not in _CACHE:
        from levelsetfusion_python_amd import device as dev
        canonical, live = _scene(name)
        band = _band(canonical, live)
        d_live, d_canonical = torch.from_numpy(live).cuda(), torch.from_numpy(canonical).cuda()
        states = [torch.full(live.shape + (4,), float("nan"), device="cuda") for _ in range(2)]
        prepared = dev.StatePrepare(d_live, d_canonical, sparse_reach=reach, states=states)
        torch.cuda.synchronize()
        _CACHE[key] = dict(live=live, band=band, d_live=d_live, prepared=prepared, needed=group_verdicts(band, reach),
                           after_pack=[s.cpu().numpy().reshape(-1, 4) for s in states])
    return _CACHE[key]


SCENES = ["ragged3d", "field2d", "cube64", "ragged3d-ends", "field2d-ends"]


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("scene", SCENES)
def test_written_groups_equal_the_restatement(lsf, groups_everywhere, scene, reach):
    case = _case(scene, reach)
    live, needed, n = case["live"], case["needed"], case["live"].size
    assert 0 < needed.sum() < needed.size, "the case is meant to leave groups out"
    # the kept masks: bit g of chunk c = group 32 c + g
    masks = case["prepared"].needed_masks().cpu().numpy().view(np.uint32)
    kept = ((masks[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).ravel()
    assert np.array_equal(kept, needed)
    want_written = np.repeat(needed, GROUP)[:n]
    for flat in case["after_pack"]:
        nan = np.isnan(flat)
        assert np.array_equal(nan.all(axis=1), nan.any(axis=1))
        written = ~nan[:, 0]
        groups = np.concatenate([written, np.zeros(needed.size * GROUP - n, dtype=bool)]).reshape(-1, GROUP)
        whole = np.concatenate([np.ones(n, dtype=bool), np.zeros(needed.size * GROUP - n, dtype=bool)]).reshape(-1, GROUP)
        assert np.array_equal(groups.any(axis=1), needed & whole.any(axis=1)), "group for group"
        assert np.array_equal(written, want_written)
        assert np.array_equal(flat[written, 0], live.ravel()[written]) and not flat[written, 1:].any()
        assert written[within_reach(case["band"], reach).ravel()].all(), "a voxel an iteration can read was left out"
    if scene.endswith("-ends"):
        assert case["band"].ravel()[0] and case["band"].ravel()[-1] and needed[0] and needed[(n - 1) // GROUP]


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("scene", SCENES)
def test_invert_writes_every_other_voxel_once(lsf, groups_everywhere, scene, reach):
    from levelsetfusion_python_amd import device as dev
    case = _case(scene, reach)
    prepared, d_live, n = case["prepared"], case["d_live"], case["live"].size
    first = ~np.isnan(case["after_pack"][0][:, 0])
    # on a poisoned buffer the second call writes exactly what the first left out ...
    other = torch.full(tuple(d_live.shape) + (4,), float("nan"), device="cuda")
    prepared.complete(other, d_live)
    second = ~np.isnan(other.cpu().numpy().reshape(-1, 4)[:, 0])
    assert np.array_equal(second, ~first) and 0 < second.sum() < n
    # ... and on the state of the first it leaves a whole state: state_pack's, word for word
    whole = dev.state_pack(d_live, None, prepared.grid, copies=1)[0]
    state = torch.from_numpy(case["after_pack"][1].copy()).cuda().reshape(whole.shape)
    prepared.complete(state, d_live)
    assert int(torch.isnan(state).sum()) == 0 and torch.equal(state, whole)


def _run3d(lsf, canonical, live0, reach, box_walk, **kw):
    opt = lsf.SlavchevaOptimizer3d(field_size=canonical.shape[-1], compute_method=lsf.ComputeMethod.DIRECT,
                                   smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                   engine_options=dict(sparse_reach=reach, sparse_min_voxels=0, box_walk=box_walk), **kw)
    live = live0.clone()
    opt.optimize(live, canonical)
    return opt, live


def _bits_equal(a, b):
    (oa, la), (ob, lb) = a, b
    assert torch.equal(la, lb), "live field"
    assert torch.equal(torch.as_tensor(oa.warp_field), torch.as_tensor(ob.warp_field)), "warp field"
    assert np.array_equal(np.float32(oa.log.max_warps), np.float32(ob.log.max_warps))
    assert oa.log.max_warp_locations == ob.log.max_warp_locations
    assert list(oa.log.data_energies) == list(ob.log.data_energies)
    assert list(oa.log.smoothing_energies) == list(ob.log.smoothing_energies)
    assert list(oa.log.level_set_energies) == list(ob.log.level_set_energies)
    assert oa.get_convergence_report() == ob.get_convergence_report()


@pytest.fixture(scope="module")
def pair48(lsf):
    from levelsetfusion_python_amd.synthetic import sphere_pair
    return sphere_pair(48, 3, "cuda")


@pytest.mark.parametrize("box_walk", [False, True])
def test_a_call_on_group_states_equals_one_on_full_states(lsf, groups_everywhere, pair48, box_walk):
    """engine_options sparse_min_voxels = 0 (the default reach) against sparse_reach = 0.  The box walk's idle lanes read
    voxels nobody initialised: allowed, and nothing of it may reach a result"""
    canonical, live0 = pair48
    kw = dict(KILLING, max_iterations=8, min_iterations=8)
    opt = lsf.SlavchevaOptimizer3d(field_size=48, compute_method=lsf.ComputeMethod.DIRECT,
                                   smoothing_term_method=lsf.SmoothingTermMethod.KILLING,
                                   engine_options=dict(sparse_min_voxels=0, box_walk=box_walk), **kw)
    live = live0.clone()
    opt.optimize(live, canonical)
    call = opt.engine.last_call
    assert call.sparse_states and call.box_walk == box_walk and not opt.engine.sparse_disabled
    _bits_equal((opt, live), _run3d(lsf, canonical, live0, 0, box_walk, **kw))
    from levelsetfusion_python_amd import device as dev
    share = dev.StatePrepare(live0, canonical, sparse_reach=opt.engine.sparse_reach).written_fraction()
    assert 0.0 < share < 1.0, "the case is meant to leave part of the states uninitialised"


@pytest.mark.parametrize("box_walk", [False, True])
def test_updates_beyond_the_reach_fall_back(lsf, groups_everywhere, pair48, box_walk):
    """rate 20: the first iteration already moves more than two voxels; the guard notices, the call runs again on full
    states and the result is the full-state result"""
    canonical, live0 = pair48
    kw = dict(KILLING, max_iterations=4, min_iterations=4)
    kw["gradient_descent_rate"] = 20.0
    full = _run3d(lsf, canonical, live0, 0, box_walk, **kw)
    assert max(full[0].log.max_warps) > 2.0
    sparse = _run3d(lsf, canonical, live0, 2, box_walk, **kw)
    assert sparse[0].engine.sparse_disabled and not sparse[0].engine.last_call.sparse_states
    _bits_equal(sparse, full)


def test_the_default_limit_chunks_below_groups_from_2_21_voxels(lsf, monkeypatch):
    """no override: 64^3 keeps whole chunks and 0 / 1 words, 128^3 = 2^21 voxels gets the group verdicts of the restatement"""
    from levelsetfusion_python_amd import device as dev
    from levelsetfusion_python_amd.synthetic import sphere_pair
    monkeypatch.delenv("LSF_SPARSE_MIN_VOXELS", raising=False)
    assert dev.StatePrepare.group_min_voxels() == 1 << 21
    for n in (64, 128):
        canonical, live = sphere_pair(n, 3, "cuda")
        states = [torch.full(tuple(live.shape) + (4,), float("nan"), device="cuda") for _ in range(2)]
        prepared = dev.StatePrepare(live, canonical, sparse_reach=2, states=states)
        words = prepared._needed_words().cpu().numpy()
        written = ~torch.isnan(states[0].reshape(-1, 4)[:, 0]).cpu().numpy()
        assert np.array_equal(written, ~torch.isnan(states[1].reshape(-1, 4)[:, 0]).cpu().numpy())
        if n == 64:
            assert set(np.unique(words)) == {0, 1}
            assert np.array_equal(written, np.repeat(words.astype(bool), CHUNK))
        else:
            needed = group_verdicts(_band(canonical.cpu().numpy(), live.cpu().numpy()), 2)
            kept = ((words.view(np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).ravel()
            assert np.array_equal(kept, needed) and np.array_equal(written, np.repeat(needed, GROUP))
            assert 0 < needed.sum() < np.repeat(words != 0, 32).sum(), "finer than the chunks"
        for st in states:
            prepared.complete(st, live)
        whole = dev.state_pack(live, None, prepared.grid, copies=1)[0]
        assert torch.equal(states[0], whole) and torch.equal(states[1], whole)
