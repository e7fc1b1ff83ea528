"""GPU check of what one SlavchevaEngine call asks of the library on every route: in each configuration below the names
of the lsf_* symbols called during the span

    engine.optimize(live, canonical, finalize=(live, 0.0, True)); outcome.finalize(live, 0.0, True);
    engine.gradient_field(); engine.cumulative_warp_field()  (where the engine composes one)

equal, in order, a table of literals, and engine.last_call -- the route included -- and the keys of engine.log are the
tabled ones.  The table was recorded with tests/test_gpu_sequence_calls.py's recorder on the commit before the engine got
one route, one iteration object per kind of launch-by-launch call, one setup for the library calls and a typed gradient
source, so it pins the number and the order of the launches of every route.  Results are not restated here:
tests/test_gpu_ragged_volumes.py holds each of these routes against the oracle on the same scenes (tests/ragged_scene.py).
Three fixed iterations unless a configuration says otherwise."""
import numpy as np
import pytest
import torch

import test_gpu_ragged_volumes as R
import test_gpu_sequence_calls as Q

pytestmark = pytest.mark.gpu

THREE = dict(max_iterations=3, min_iterations=3)
LOG_KEYS = {"max_warps", "max_warp_indices", "data_energies", "smoothing_energies", "level_set_energies"}
NO_LIBRARY = dict(library_run=False)
SPARSE = dict(sparse_reach=2, sparse_min_voxels=0)


def _sobolev(taps, **kw):
    return dict(R.SOBOLEV, sobolev_kernel=R._kernel(taps), **dict(THREE, **kw))


def _killing(**kw):
    return dict(R.BASE, **dict(THREE, **kw))


# name -> (scene, the oracle's keywords, engine options, further settings: check_interval, calls (spans on one engine),
# hook (an iteration_hook that reads gradient_field()), focus (focus_voxels), cumulative_warp)
CONFIGURATIONS = {
    "library: fours": ("fours", _killing(), None, {}),
    "library: fours, box walk": ("fours", _killing(), dict(box_walk=True), {}),
    # updates of 2.4 to 3.8 voxels outrun the reach: the span holds the sparse attempt and the one on full states
    "library: fours, sparse": ("fours", _killing(), SPARSE, {}),
    # every maximum of `odd` (3.7 to 5 voxels) stays above the lower threshold: three batches of two gated launches
    "library: odd, threshold": ("odd", _killing(min_iterations=1, max_iterations=6,
                                                 maximum_warp_length_lower_threshold=0.5), None, dict(check_interval=2)),
    # the second call zeroes the first call's listed voxels and does not refill the gradient buffers
    "library: fours, sobolev 7, two calls": ("fours", _sobolev(7), None, dict(calls=2)),
    "launches: odd": ("odd", _killing(), NO_LIBRARY, {}),
    "launches: odd, sparse": ("odd", _killing(), dict(NO_LIBRARY, **SPARSE), {}),
    # `far` moves 0.2 voxels per iteration: the sparse states stand, and gradient_field() completes its input state
    "launches: far, sparse": ("far", _killing(), dict(NO_LIBRARY, **SPARSE), {}),
    "launches: odd, no list": ("odd", _killing(), dict(NO_LIBRARY, use_band_list=False), {}),
    "launches: odd, hook": ("odd", _killing(), NO_LIBRARY, dict(hook=True)),
    "launches: flat, focus": ("flat", _killing(), NO_LIBRARY, dict(focus=[(16, 35), (17, 35)])),
    "launches: flat, sobolev 7": ("flat", _sobolev(7), NO_LIBRARY, {}),
    "launches: odd, sobolev 7, no boxes": ("odd", _sobolev(7), dict(NO_LIBRARY, sobolev_boxes=False), {}),
    "launches: odd, sobolev 11": ("odd", _sobolev(11), NO_LIBRARY, {}),
    "launches: odd, sobolev 7, no list": ("odd", _sobolev(7), dict(NO_LIBRARY, use_band_list=False), {}),
    "launches: odd, cumulative warp": ("odd", _killing(), NO_LIBRARY, dict(cumulative_warp=True)),
    # tests/test_gpu_ragged_volumes.py::test_updates_beyond_the_reach_fall_back's pair and settings (four iterations)
    "fall-back: library": ("odd", dict(R.BASE), SPARSE, {}),
    "fall-back: launches": ("odd", dict(R.BASE), dict(NO_LIBRARY, **SPARSE), {}),
}

_PREPARE = ["lsf_state_prepare_scratch_elements", "lsf_state_prepare", "lsf_state_pack"] + ["lsf_band_list_fill_prepared"] * 2
_PREPARE_SPARSE = [c + "_needed" if c == "lsf_state_pack" else c for c in _PREPARE]
_ITERATION = ["lsf_slavcheva_state_iteration"] * 2  # the INTERIOR and the BOUNDARY list
_FINALIZE = ["lsf_state_finalize_scratch_elements", "lsf_state_finalize_listed", "lsf_records_decode"]
_GRADIENT = ["lsf_state_unpack", "lsf_slavcheva_gradient", "lsf_slavcheva_update_rewarp"]  # gradient_field(), dense
_LISTED_GRADIENT = ["lsf_state_unpack"] + ["lsf_slavcheva_gradient"] * 2 + ["lsf_slavcheva_update_rewarp"] * 2
_RUN = ["lsf_state_prepare_scratch_elements", "lsf_state_run_begin", "lsf_state_run_rows_elements",
        "lsf_state_finalize_scratch_elements", "lsf_state_run_finish_rows"]
_RUN_BOXES = ["lsf_state_prepare_scratch_elements", "lsf_band_boxes_scratch_elements", "lsf_state_run_begin"]
_SOBOLEV_FINISH = ["lsf_state_finalize_scratch_elements", "lsf_sobolev_run_finish"]
_WARP = ["lsf_state_finalize_listed"]  # the library call's warp, built when finalize()'s callable is called
_HOOK = ["lsf_state_unpack"] * 2 + _GRADIENT[1:] + ["lsf_interleave"] * 2
_PROBE = ["lsf_state_unpack", "lsf_slavcheva_gradient"]
_PLANAR = ["lsf_slavcheva_gradient"] + ["lsf_convolve_axis"] * 3 + ["lsf_slavcheva_update_rewarp"]
_PLANAR_CALL = _PLANAR * 3 + ["lsf_records_decode", "lsf_state_finalize_scratch_elements", "lsf_planar_finalize"]
_LISTED4 = ["lsf_convolve_axis_listed4"] * 2 + ["lsf_sobolev_state_update"] * 2
_FALL_BACK = _RUN * 2 + _WARP + _LISTED_GRADIENT  # the sparse attempt (its finalize pass held back by the guard), again

# name -> the symbols called during the span(s), in order
CALLS = {
    "library: fours": _RUN + _WARP + _LISTED_GRADIENT,
    "library: fours, box walk": _RUN_BOXES + _RUN[2:] + _WARP + _LISTED_GRADIENT,
    "library: fours, sparse": _FALL_BACK,
    "library: odd, threshold": _RUN[:2] + _RUN[3:] + _WARP + _LISTED_GRADIENT,  # a gated loop takes no record rows
    "library: fours, sobolev 7, two calls": (_RUN_BOXES + _SOBOLEV_FINISH + _WARP
                                             + _RUN_BOXES + ["lsf_zero_listed4"] * 2 + _SOBOLEV_FINISH + _WARP),
    "launches: odd": _PREPARE + _ITERATION * 3 + _FINALIZE + _GRADIENT,
    "launches: odd, sparse": (_PREPARE_SPARSE + _ITERATION * 3 + _FINALIZE
                              + _PREPARE + _ITERATION * 3 + _FINALIZE + _GRADIENT),
    "launches: far, sparse": (_PREPARE_SPARSE[:-1] + _ITERATION[:1] * 3 + _FINALIZE
                              + ["lsf_state_pack_needed"] + _GRADIENT),  # one list; the rest of the input state
    "launches: odd, no list": (["lsf_state_pack"] + _ITERATION[:1] * 3
                               + ["lsf_state_finalize_scratch_elements", "lsf_state_finalize", "lsf_records_decode"]
                               + _GRADIENT),
    "launches: odd, hook": (_PREPARE + (_ITERATION + ["lsf_records_decode"] + _HOOK) * 2 + _ITERATION + _FINALIZE + _HOOK
                            + _GRADIENT),
    "launches: flat, focus": (_PREPARE + (_ITERATION + ["lsf_records_decode"] + _PROBE) * 2 + _ITERATION + _FINALIZE
                              + _PROBE + _GRADIENT),
    "launches: flat, sobolev 7": _PREPARE + (["lsf_sobolev_state_gradient"] * 2 + _LISTED4) * 3 + _FINALIZE,
    "launches: odd, sobolev 7, no boxes": (_PREPARE + ["lsf_merge_sorted_runs"]
                                           + (["lsf_sobolev_state_gradient_x"] + _LISTED4) * 3 + _FINALIZE),
    "launches: odd, sobolev 11": _PLANAR_CALL,
    "launches: odd, sobolev 7, no list": _PLANAR_CALL,
    "launches: odd, cumulative warp": (_PREPARE + (_ITERATION + ["lsf_cumulative_warp_compose"] * 2) * 3 + _FINALIZE
                                       + _GRADIENT + ["lsf_state_unpack"]),
    "fall-back: library": _FALL_BACK,
    "fall-back: launches": (_PREPARE_SPARSE + _ITERATION * 4 + _FINALIZE + _PREPARE + _ITERATION * 4 + _FINALIZE
                            + _GRADIENT),
}


def _report(route, **taken):
    report = dict(sparse_states=False, box_walk=False, sobolev_boxes=False, library_run=route != "launches",
                  blocked_levels=0, record_rows=False, route=route)
    return dict(report, **taken)


# name -> vars(engine.last_call) after the span(s); unnamed: launch by launch, nothing taken
LAST_CALL = {
    "library: fours": _report("library_run", record_rows=True),
    "library: fours, box walk": _report("library_run", record_rows=True, box_walk=True),
    "library: fours, sparse": _report("library_run", record_rows=True),
    "library: odd, threshold": _report("library_run"),
    "library: fours, sobolev 7, two calls": _report("library_sobolev_run", sobolev_boxes=True),
    "launches: far, sparse": _report("launches", sparse_states=True),
    "fall-back: library": _report("library_run", record_rows=True),
}

# name -> (iteration_count, sparse_disabled) after the span(s); unnamed: (3, False)
ENDS = {
    "library: fours, sparse": (3, True),
    "library: odd, threshold": (6, False),
    "launches: odd, sparse": (3, True),
    "fall-back: library": (4, True),
    "fall-back: launches": (4, True),
}


class _Spans:
    """Q.recorded_frames records what `integrate` calls from its second set of arguments on: the first does nothing,
    the second runs the spans"""

    def integrate(self, run):
        run()


def span(engine, canonical, live0, calls=1):
    """the recorded part: `calls` times optimize on a fresh copy of the live field, finalize, the two fields"""
    for _ in range(calls):
        live = live0.clone()
        outcome = engine.optimize(live, canonical, finalize=(live, 0.0, True))
        final, warp, raw = outcome.finalize(live, 0.0, True)
        assert final is live and raw is not None
        warp = warp() if callable(warp) else warp
        gradient = engine.gradient_field()
        psi = engine.cumulative_warp_field()
        assert (psi is not None) == engine.cumulative_warp
    return live, warp, gradient, psi, raw


def make(name):
    """(engine, canonical, live) of a configuration, on the device"""
    from levelsetfusion_python_amd import _lib, engine
    key, cfg, options, more = CONFIGURATIONS[name]
    kernel = cfg["sobolev_kernel"]
    eng = engine.SlavchevaEngine(
        cfg["compute_method"] == R.O.DIRECT, cfg["level_set_term_enabled"], cfg["sobolev_smoothing_enabled"],
        _lib.DATA_BASIC, _lib.SMOOTHING_KILLING if cfg["smoothing_term_method"] == R.O.KILLING else _lib.SMOOTHING_TIKHONOV,
        cfg["gradient_descent_rate"], cfg["data_term_weight"], cfg["smoothing_term_weight"],
        cfg["isomorphic_enforcement_factor"], cfg["level_set_term_weight"], cfg["maximum_warp_length_lower_threshold"],
        cfg["maximum_warp_length_upper_threshold"], cfg["max_iterations"], cfg["min_iterations"],
        None if kernel is None else np.asarray(kernel, dtype=np.float64), check_interval=more.get("check_interval", 32),
        options=options, cumulative_warp=more.get("cumulative_warp", False))
    if more.get("hook"):
        eng.iteration_hook = lambda level, i, warp, gradient, max_warp: eng.gradient_field()
    if more.get("focus"):
        eng.focus_voxels = more["focus"]
    canonical, live = R._device(key)
    return eng, canonical, live


def recorded(patch, name):
    """(the symbols called during the configuration's spans, the engine, what the last span returned)"""
    eng, canonical, live = make(name)
    got = []
    calls = Q.recorded_frames(patch, _Spans(), [(lambda: None,), (lambda: got.append(
        span(eng, canonical, live, CONFIGURATIONS[name][3].get("calls", 1))),)])
    return calls, eng, got[0]


@pytest.mark.parametrize("name", sorted(CONFIGURATIONS))
def test_a_call_asks_the_library_as_tabled(monkeypatch, name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    calls, eng, _ = recorded(monkeypatch, name)
    print(name, calls, vars(eng.last_call), eng.iteration_count, eng.sparse_disabled)
    assert calls == CALLS[name]
    assert vars(eng.last_call) == LAST_CALL.get(name, _report("launches"))
    assert set(eng.log.keys()) == LOG_KEYS
    assert (eng.iteration_count, eng.sparse_disabled) == ENDS.get(name, (3, False))
    assert all(len(eng.log[k]) == eng.iteration_count for k in LOG_KEYS)
