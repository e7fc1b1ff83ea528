"""Host check, no card: the route of a SlavchevaEngine call (engine_slavcheva.ROUTES), the sub-decisions of the
launch-by-launch route (_LaunchPlan) and the "sparse states?" rule equal tables of literals.  The tables were filled from the
expressions _optimize, _optimize_run and _optimize_slab_run held before the route was decided in one place, and hold for both.
The shapes are tests/ragged_scene.py's -- `fours` (whole boxes), `odd`, `tiny`, 2-D `flat` -- and, for slabs, arrays whose
slices are a multiple of the prepare pass's 1024-voxel chunk (32 x 32) or not (`fours`)."""
import types

import numpy as np
import pytest
import torch

import ragged_scene

SHAPES = dict({name: shape for name, (shape, _) in ragged_scene.SCENES.items()}, chunked=(20, 32, 32),
              tall=(140, 32, 32))


class StubComm:
    """an active slab communicator as _grid, _route and _slab_run_ok read it: z-slabs of halo `halo` around the owned
    slices of an nz-slice local array, with or without the library's transport"""

    active = True

    def __init__(self, nz, halo, native=True):
        self.layout = types.SimpleNamespace(axis=0, nz_local=nz, z_begin=halo, z_end=nz - halo, z_global_offset=0,
                                            halo=halo)
        self._native = object() if native else None

    def native(self):
        return self._native


def make(options, taps, cumulative_warp, iterations, comm):
    from levelsetfusion_python_amd import _lib, engine
    kernel = None if taps is None else np.full(taps, 1.0 / taps)
    return engine.SlavchevaEngine(True, taps is None, taps is not None, _lib.DATA_BASIC,
                                  _lib.SMOOTHING_KILLING if taps is None else _lib.SMOOTHING_TIKHONOV, 0.1, 1.0, 0.2, 0.1,
                                  0.2, 0.0, 10000.0, iterations[1], iterations[0], kernel, comm=comm, options=options,
                                  cumulative_warp=cumulative_warp)


def _comm(spec, shape):
    return None if spec is None else StubComm(SHAPES[shape][0], *spec)


F, T = False, True
FIXED, GATED = (3, 3), (1, 6)
NO_LIBRARY = (("library_run", False),)
DENSE = (("use_band_list", False),)
ALWAYS_SPARSE = (("sparse_min_voxels", 0),)
STATISTICS, NO_STATISTICS, NO_FINALIZE = "statistics", "no statistics", None
# (engine options, shape, Sobolev taps, finalize, hook set, cumulative_warp, (min, max) iterations, comm: None or (halo[,
# native])) -> (route, _LaunchPlan or None: planar_sobolev, sob_state, fused_prepare, slab_groups, sparse, warp_fill,
# sobolev_boxes)
ROUTES = {
    # the library call on a whole volume: 3-D, less than a chunk, 2-D, a gated loop
    ((), "fours", None, STATISTICS, F, F, FIXED, None): ("library_run", None),
    ((), "odd", None, NO_STATISTICS, F, F, FIXED, None): ("library_run", None),
    ((), "tiny", None, STATISTICS, F, F, FIXED, None): ("library_run", None),
    ((), "flat", None, STATISTICS, F, F, FIXED, None): ("library_run", None),
    ((), "odd", None, STATISTICS, F, F, GATED, None): ("library_run", None),
    # ... and what takes a call off it
    (NO_LIBRARY, "fours", None, STATISTICS, F, F, FIXED, None): ("launches", (F, F, T, F, F, "before", F)),
    ((), "fours", None, NO_FINALIZE, F, F, FIXED, None): ("launches", (F, F, T, F, F, None, F)),
    ((), "fours", None, STATISTICS, T, F, FIXED, None): ("launches", (F, F, T, F, F, "before", F)),
    ((), "fours", None, STATISTICS, F, F, (0, 3), None): ("launches", (F, F, T, F, F, "before", F)),
    ((), "fours", None, STATISTICS, F, T, FIXED, None): ("launches", (F, F, T, F, F, "before", F)),
    (DENSE, "odd", None, STATISTICS, F, F, FIXED, None): ("launches", (F, F, F, F, F, None, F)),
    # sparse states launch by launch: from sparse_min_voxels on, and not under a hook
    (NO_LIBRARY + ALWAYS_SPARSE, "odd", None, STATISTICS, F, F, FIXED, None): ("launches", (F, F, T, F, T, "before", F)),
    (NO_LIBRARY + ALWAYS_SPARSE, "odd", None, STATISTICS, T, F, FIXED, None): ("launches", (F, F, T, F, F, "before", F)),
    (NO_LIBRARY + ALWAYS_SPARSE + (("sparse_reach", 0),), "odd", None, STATISTICS, F, F, FIXED, None):
        ("launches", (F, F, T, F, F, "before", F)),
    # SobolevFusion: the library call wants whole boxes in 3-D and a listed tap count
    ((), "fours", 7, STATISTICS, F, F, FIXED, None): ("library_sobolev_run", None),
    ((), "fours", 7, STATISTICS, F, F, GATED, None): ("library_sobolev_run", None),
    (NO_LIBRARY, "fours", 7, STATISTICS, F, F, FIXED, None): ("launches", (F, T, T, F, F, "before", T)),
    ((("sobolev_boxes", False),), "fours", 7, STATISTICS, F, F, FIXED, None): ("launches", (F, T, T, F, F, "before", F)),
    ((), "fours", 7, STATISTICS, T, F, FIXED, None): ("launches", (F, T, T, F, F, "before", T)),
    ((), "odd", 7, STATISTICS, F, F, FIXED, None): ("launches", (F, T, T, F, F, "before", F)),
    ((), "flat", 7, STATISTICS, F, F, FIXED, None): ("launches", (F, T, T, F, F, "before", F)),
    ((), "fours", 11, STATISTICS, F, F, FIXED, None): ("launches", (T, F, F, F, F, None, F)),
    ((), "odd", 11, STATISTICS, F, F, FIXED, None): ("launches", (T, F, F, F, F, None, F)),
    (DENSE, "odd", 7, STATISTICS, F, F, FIXED, None): ("launches", (T, F, F, F, F, None, F)),
    # a z-slab rank: the library call wants chunked slices, a fixed count, no statistics, a halo of at most 32 slices and
    # the native transport
    ((), "chunked", None, NO_STATISTICS, F, F, FIXED, (2,)): ("library_slab_run", None),
    (ALWAYS_SPARSE, "chunked", None, NO_STATISTICS, F, F, FIXED, (2,)): ("library_slab_run", None),
    ((), "chunked", None, STATISTICS, F, F, FIXED, (2,)): ("launches", (F, F, T, T, F, None, F)),
    ((), "chunked", None, NO_STATISTICS, F, F, GATED, (2,)): ("launches", (F, F, T, F, F, None, F)),
    ((), "tall", None, NO_STATISTICS, F, F, FIXED, (33,)): ("launches", (F, F, T, T, F, None, F)),
    ((), "chunked", None, NO_STATISTICS, F, F, FIXED, (2, False)): ("launches", (F, F, T, T, F, None, F)),
    ((), "fours", None, NO_STATISTICS, F, F, FIXED, (2,)): ("launches", (F, F, T, T, F, None, F)),
    (NO_LIBRARY + ALWAYS_SPARSE, "chunked", None, NO_STATISTICS, F, F, FIXED, (2,)): ("launches", (F, F, T, T, T, None, F)),
    (NO_LIBRARY + ALWAYS_SPARSE, "chunked", None, NO_STATISTICS, F, F, FIXED, (1,)): ("launches", (F, F, T, F, F, None, F)),
    (NO_LIBRARY + ALWAYS_SPARSE, "chunked", None, NO_STATISTICS, F, F, GATED, (2,)): ("launches", (F, F, T, F, F, None, F)),
    ((), "chunked", 7, NO_STATISTICS, F, F, FIXED, (3,)): ("launches", (T, F, F, F, F, None, F)),
}


def _arguments(key):
    options, shape, taps, finalize, hook, cumulative, iterations, comm = key
    eng = make(dict(options), taps, cumulative, iterations, _comm(comm, shape))
    if hook:
        eng.iteration_hook = lambda *a: None
    live = torch.zeros(SHAPES[shape])
    return eng, eng._grid(live), None if finalize is None else (live, 0.0, finalize == STATISTICS), hook


@pytest.mark.parametrize("key", list(ROUTES), ids=[repr(k) for k in ROUTES])
def test_route_and_launch_plan(key):
    from levelsetfusion_python_amd import engine_slavcheva
    eng, grid, finalize, watched = _arguments(key)
    route, plan = ROUTES[key]
    assert route in engine_slavcheva.ROUTES and eng._route(grid, finalize, watched) == route
    if plan is not None:
        got = eng._launch_plan(grid, finalize, watched)
        assert isinstance(got, engine_slavcheva._LaunchPlan) and tuple(got) == plan


def test_focus_voxels_watch_a_call_as_a_hook_does():
    eng, grid, finalize, _ = _arguments(((), "flat", None, STATISTICS, F, F, FIXED, None))
    assert eng._route(grid, finalize, True) == "launches"
    assert eng.last_call.route is None  # (nothing has been called yet)


# who asks, engine options, shape, (min, max) iterations, comm, exchange every iteration (a wider re-run),
# sparse_disabled, watched -> sparse states?  The library calls never ask for a watched call or a gated slab
LAUNCHES, RUN, SLAB_RUN = "launch by launch", "library call", "library slab call"
BELOW = (("sparse_min_voxels", 20 * 28 * 36 + 1),)
AT = (("sparse_min_voxels", 20 * 28 * 36),)
SPARSE = {
    (RUN, (), "fours", FIXED, None, F, F, F): F,          # the default 2^21 voxels
    (RUN, BELOW, "fours", FIXED, None, F, F, F): F,
    (RUN, AT, "fours", FIXED, None, F, F, F): T,
    (RUN, AT, "fours", GATED, None, F, F, F): T,
    (RUN, AT, "fours", FIXED, None, F, T, F): F,
    (RUN, AT + (("sparse_reach", 0),), "fours", FIXED, None, F, F, F): F,
    (RUN, ALWAYS_SPARSE, "flat", FIXED, None, F, F, F): T,
    (LAUNCHES, (), "fours", FIXED, None, F, F, F): F,
    (LAUNCHES, AT, "fours", FIXED, None, F, F, F): T,
    (LAUNCHES, AT, "fours", GATED, None, F, F, F): T,
    (LAUNCHES, AT, "fours", FIXED, None, F, F, T): F,
    (LAUNCHES, AT, "fours", FIXED, None, F, T, F): F,
    (LAUNCHES, ALWAYS_SPARSE, "chunked", FIXED, (2,), F, F, F): T,
    (LAUNCHES, ALWAYS_SPARSE, "chunked", FIXED, (2,), F, F, T): F,
    (LAUNCHES, ALWAYS_SPARSE, "chunked", FIXED, (1,), F, F, F): F,   # a halo below max(sparse_reach, 2)
    (LAUNCHES, ALWAYS_SPARSE + (("sparse_reach", 3),), "chunked", FIXED, (2,), F, F, F): F,
    (LAUNCHES, ALWAYS_SPARSE + (("sparse_reach", 3),), "chunked", FIXED, (3,), F, F, F): T,
    (LAUNCHES, ALWAYS_SPARSE, "chunked", GATED, (2,), F, F, F): F,   # no exchange groups
    (LAUNCHES, ALWAYS_SPARSE, "chunked", FIXED, (2,), T, F, F): F,
    (SLAB_RUN, (), "chunked", FIXED, (2,), F, F, F): F,
    (SLAB_RUN, ALWAYS_SPARSE, "chunked", FIXED, (2,), F, F, F): T,
    (SLAB_RUN, ALWAYS_SPARSE, "chunked", FIXED, (1,), F, F, F): F,
    (SLAB_RUN, ALWAYS_SPARSE, "chunked", FIXED, (2,), T, F, F): F,
    (SLAB_RUN, ALWAYS_SPARSE, "chunked", FIXED, (2,), F, T, F): F,
    (SLAB_RUN, ALWAYS_SPARSE + (("sparse_reach", 0),), "chunked", FIXED, (2,), F, F, F): F,
}


def sparse_engine(key):
    _, options, shape, iterations, comm, every, disabled, watched = key
    eng = make(dict(options), None, False, iterations, _comm(comm, shape))
    eng._exchange_every_iteration, eng.sparse_disabled = every, disabled
    return eng, eng._grid(torch.zeros(SHAPES[shape])), watched


@pytest.mark.parametrize("key", list(SPARSE), ids=[repr(k) for k in SPARSE])
def test_sparse_states_rule(key):
    eng, grid, watched = sparse_engine(key)
    assert eng._sparse_states(grid, watched) is SPARSE[key]
