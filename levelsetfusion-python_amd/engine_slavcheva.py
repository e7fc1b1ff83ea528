"""SlavchevaEngine: the per-iteration-update optimizer with in-place re-warping of the live field
(nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:332-408), D = 2 or 3, on whole volumes or slabs.  The drop-in classes
SlavchevaOptimizer2d / 3d are thin shells around it.  This module: construction and the engine's declared state, the
route of a call (_route) and the sub-decisions of the launch-by-launch one (_launch_plan), that call as stages over one
iteration object (one foreign call per launch, batches of `check_interval` iterations between host reads) with the
fused iteration object, hooks and gradient_field; the library-enqueued calls and their shared setup live in engine_run.py,
slabs in engine_slab.py, the SobolevFusion iteration objects in engine_sobolev.py, what a call leaves behind -- outcome,
log, gradient sources -- in engine_outcome.py."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, device as dev, engine_options
from .engine_common import _Counted, _Fast, _Lazy
from .engine_focus import FocusMixin
from .engine_outcome import _StateIteration, recompute_gradient
from .engine_run import RunMixin, _SparseStateExceeded
from .engine_slab import SlabMixin, _HaloTooNarrow
from .engine_sobolev import _PlanarIteration, _SobolevStatePlan

# the ways a call is enqueued (last_call.route): the library call on a whole volume, the library SobolevFusion call, the
# library slab call, launch by launch
ROUTES = ("library_run", "library_sobolev_run", "library_slab_run", "launches")

# the sub-decisions of a launch-by-launch call: planar fields / float4 SobolevFusion / (neither: the fused state); states and
# lists from one prepare pass; a slab in exchange groups whose halo carries sparse states; sparsely initialised states; the
# zero fill of the warp output "before" or "behind" the counting pass (None: no such fill); SobolevFusion box by box
_LaunchPlan = collections.namedtuple("_LaunchPlan", "planar_sobolev sob_state fused_prepare slab_groups sparse warp_fill "
                                                    "sobolev_boxes")


class _FusedIteration(_StateIteration):
    """fused path: ONE kernel per iteration (and per band list) on the float4 state (live, u, v, w), on a whole volume or
    -- through SlabMixin's launch plan -- a slab, and with cumulative_warp the composition launches behind it"""

    def __init__(self, engine, launcher, limit, psi=None, complete=None):
        self.engine, self.f, self.limit, self.psi, self._complete = engine, launcher, limit, psi, complete

    def enqueue(self, i):
        e, f = self.engine, self.f
        if e._slab():
            return e._enqueue_slab_state_iteration(i, self.states, self.limit)
        s_in, s_out = f.p_state[i % 2], f.p_state[(i + 1) % 2]
        gate_ref = None if i < e.min_iterations else f.gate_ref(i - 1)
        run = _lib.lib.lsf_slavcheva_state_iteration
        for band in f.bands:  # interior + boundary band voxels (or one list / the dense walk)
            status = run(s_in, f.p_canon, s_out, f.grid_ref, f.params_ref, gate_ref, f.record_ptrs[i],
                         band.pointer, band.count, band.subset, f.stream)
            if status:
                _lib.check(status, "lsf_slavcheva_state_iteration")
        # cumulative_warp: PSI_{i+1} = u_i + PSI_i(id + u_i) at the voxels of every band list, from the state iteration i
        # has just written, under iteration i's gate (lsf_cumulative_warp_compose)
        run = _lib.lib.lsf_cumulative_warp_compose
        for band in f.bands if self.psi is not None else ():
            if band.indices is not None and band.count == 0:
                continue  # an empty list: nothing to compose
            status = run(f.p_state[(i + 1) % 2], f.p_psi[i % 2], f.p_psi[(i + 1) % 2], f.grid_ref, gate_ref, band.pointer,
                         band.count, f.stream)
            if status:
                _lib.check(status, "lsf_cumulative_warp_compose")

    def _recompute(self, state_in, complete=None):
        params, canonical, grid = self.engine.params, self.canonical, self.grid
        return _Lazy(lambda: recompute_gradient(params, state_in, canonical, grid, complete=complete))

    def after(self, i):
        """iteration i has run: the warp it left and its gradient, planar; the hook may read gradient_field() itself"""
        warp_planar = self.inputs(i + 1)[1]
        source = self.engine._gradient_state = self._recompute(self.states[i % 2])
        return warp_planar, source.get()

    def gradient_source(self, n_exec):
        return self._recompute(self.states[(n_exec - 1) % 2], self._complete)

    def cumulative_source(self, n_exec):
        """gated launches behind the stop composed nothing: n_exec compositions have run"""
        psi, grid = self.psi[n_exec % 2], self.grid

        def interleaved():
            out = torch.empty(tuple(psi.shape[:-1]) + (grid.dims,), dtype=torch.float32, device=psi.device)
            dev.state_unpack(psi, grid, warp_interleaved_out=out)
            return out
        return _Lazy(interleaved)


class SlavchevaEngine(RunMixin, SlabMixin, FocusMixin):
    """per-iteration-update optimizer with in-place re-warping of the live field
    (nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:332-408), D = 2 or 3, optionally on a z-slab."""

    def __init__(self, direct, level_set_term_enabled, sobolev_smoothing_enabled, data_term_method,
                 smoothing_term_method, gradient_descent_rate, data_term_weight, smoothing_term_weight,
                 isomorphic_enforcement_factor, level_set_term_weight, lower_threshold, upper_threshold,
                 max_iterations, min_iterations, sobolev_kernel, compute_energies=True, check_interval=32,
                 comm=None, options=None, cumulative_warp=False):
        self.direct = bool(direct)
        self.sobolev = bool(sobolev_smoothing_enabled)
        self.sobolev_kernel = sobolev_kernel
        if self.sobolev and sobolev_kernel is None:
            raise ValueError("sobolev_smoothing_enabled requires a sobolev_kernel")
        # the call also composes its iterations' updates into the cumulative displacement PSI with
        # live_0(v + PSI(v)) ~ canonical(v) ("Cumulative warp"): a keyword, not an engine
        # option, since it changes what a call leaves behind
        self.cumulative_warp = bool(cumulative_warp)
        if self.cumulative_warp and self.sobolev:
            raise ValueError("cumulative_warp does not combine with sobolev_smoothing_enabled: the planar and float4 "
                             "Sobolev launch plans do not compose the warp")
        if self.cumulative_warp and comm is not None and comm.active:
            raise ValueError("cumulative_warp does not combine with an active comm: slab runs would need a halo of the "
                             "cumulative warp")
        lam = float(isomorphic_enforcement_factor)
        # VECTORIZED ignores the Killing / level-set / thresholded options (slavcheva_optimizer2d.py:163-190)
        smoothing = smoothing_term_method if self.direct else _lib.SMOOTHING_TIKHONOV
        data = data_term_method if self.direct else _lib.DATA_BASIC
        level_set = bool(level_set_term_enabled) and self.direct
        energy = _lib.ENERGY_NONE if not compute_energies else \
            (_lib.ENERGY_DIRECT if self.direct else _lib.ENERGY_VECTORIZED)
        self.params = _lib.SlavchevaParams(lam, float(gradient_descent_rate), float(data_term_weight),
                                           float(smoothing_term_weight), float(level_set_term_weight), lam,
                                           float(np.float32(-2.0 * (1.0 + lam))), int(smoothing), int(data),
                                           int(level_set), int(energy), int(self.direct), 0)
        self.weights = (float(data_term_weight), float(smoothing_term_weight), float(level_set_term_weight))
        self.lo, self.hi = float(lower_threshold), float(upper_threshold)
        self.max_iterations, self.min_iterations = int(max_iterations), int(min_iterations)
        self.check_interval = max(1, int(check_interval))
        self.comm = comm
        engine_options.apply(self, engine_options.SLAVCHEVA_DEFAULTS, options)  # use_band_list, library_run, ...
        # a call on sparsely initialised states met an update they cannot carry: this optimizer's data move that far,
        # every later call runs on fully initialised states
        self.sparse_disabled = False
        # opt-in per-iteration call-back f(level = 0, iteration, warp, gradient, max_warp) (device tensors, API layout),
        # where the reference writes its per-iteration visualisations (slavcheva_optimizer2d.py:387-388).  None: no cost.
        self.iteration_hook = None
        self._declare_call_state()

    def _declare_call_state(self):
        """everything the engine keeps between or during calls, apart from its settings: what the last call left, the
        caches, the slab transport's device resources.  A wider re-run starts from these values (_widened_engine)."""
        self.last_call = engine_options.new_call_report()
        self.iteration_count = 0
        self.log = None
        # engine_common._Fast of the last call (None on planar fields); the engine_common._Lazy behind gradient_field() and
        # behind cumulative_warp_field(); SobolevFusion: what the call listed (a .count: bench.py prices the path over it)
        self._fast = self._gradient_state = self._cumulative_state = self._sobolev_band = None
        # caches: the library SobolevFusion call's gradient buffers (key, g4, lists, listed voxels); z-slabs: (key, the z
        # cuts as chunk numbers on the device)
        self._g4_cache, self._cut_chunk_cache = None, (None, None)
        # slabs: the faces travel every iteration (a wider re-run); (the caller's tensor an early finalize pass wrote, its
        # contents before); torch transport: the event of an exchange in flight; the transport's device resources
        self._exchange_every_iteration = False
        self._slab_restore = self._pending_halos = None
        self._comm_stream = self._events = self._plan_stream = self._no_face = None
        self._focus_flat = None        # the traced voxels of a call with focus_voxels

    def _grid(self, live):
        if self.comm is not None and self.comm.active:
            L = self.comm.layout
            if L.axis == 1:
                # slabs cut along y: the launches name their voxels by band lists (every z), the grid carries the global
                # row of local row 0 (gather positions, reported indices) and the owned rows (energies)
                if live.dim() != 3 or live.shape[1] != L.n_local:
                    raise ValueError("y-slab runs need a 3-D local field with %d rows, got %r"
                                     % (L.n_local, tuple(live.shape)))
                g = dev.make_grid(live.shape)
                g.y_global_offset, g.ny_global = L.global_offset, L.n_global
                g.energy_y_begin, g.energy_y_end = L.begin, L.end
                return g
            if live.dim() != 3 or live.shape[0] != L.nz_local:
                raise ValueError("slab runs need a 3-D local field with %d slices, got %r"
                                 % (L.nz_local, tuple(live.shape)))
            return dev.make_grid(live.shape, L.z_begin, L.z_end, L.z_global_offset)
        return dev.make_grid(live.shape)

    def _slab(self):
        return self.comm is not None and self.comm.active

    def _gate_for(self, records, i):
        # iteration i runs iff i < min_iterations or (i < max_iterations and lo < max_warp[i-1] < hi)
        # (slavcheva_optimizer2d.py:360-362)
        return None if i < self.min_iterations else dev.make_gate(records, i - 1, _lib.GATE_SLAVCHEVA, self.lo,
                                                                  self.hi)

    def _sparse_states(self, grid, watched=False):
        """does this call run on states that are initialised near the band only?
        whole volumes: the states are initialised near the band only (a quarter of the voxels of a 256^3 sphere
        pair), valid while every update stays below SPARSE_REACH voxels -- checked on the device in front of an
        early finalize pass and on the host behind every batch
        Slabs: in exchange groups only (a fixed iteration count; an update of one voxel or more already sends the
        call to _optimize_widened, which exchanges every iteration and runs on full states), with a halo of at
        least SPARSE_REACH slices: then every chunk a rank reads in its halo is one the owner initialises too (the
        band voxel that makes it needed lies inside the owner's halo), so even whole faces carry valid data"""
        if self._slab() and not self._slab_groups():
            return False
        return (self.sparse_reach > 0 and dev.n_voxels(grid) >= self.sparse_min_voxels and not watched
                and not self.sparse_disabled)

    def _slab_groups(self):
        return (self._slab() and self.min_iterations >= max(self.max_iterations, self.min_iterations)
                and not self._exchange_every_iteration and self.comm.layout.halo >= max(self.sparse_reach, 2))

    def _route(self, grid, finalize, watched):
        """how this call is enqueued, one of ROUTES: decided from the arguments and the engine's settings alone"""
        slab = self._slab()
        # cumulative_warp: the general path, where a composition launch follows every iteration's launches
        run_ok = (self.library_run and finalize is not None and not self.sobolev and self.use_band_list
                  and not watched and self.min_iterations > 0 and dev.buffer_addressing_ok(grid)
                  and not self.cumulative_warp)
        if (self.library_run and finalize is not None and self.sobolev and self.sobolev_boxes and self.use_band_list
                and not watched and self.min_iterations > 0 and not slab and grid.dims == 3
                and dev.boxes_ok(grid) and dev.n_voxels(grid) < (1 << 27) and dev.buffer_addressing_ok(grid)
                and len(self.sobolev_kernel) in dev.LISTED_TAP_COUNTS):
            # SobolevFusion on a whole 3-D volume of whole boxes: the call enqueued by the library as well
            return "library_sobolev_run"
        if run_ok and not slab:
            # a whole volume, no Sobolev filter, nobody watching the iterations: the whole call is enqueued by the library
            # (two host calls; slavcheva_optimizer2d.py:354-388's loop without a Python iteration) -- a fixed iteration count
            # at once, the reference's default threshold-terminated loop in batches of check_interval gated launches
            return "library_run"
        if run_ok and slab and not finalize[2] and self.min_iterations >= self.max_iterations and self._slab_run_ok(grid):
            # a z-slab rank on the library's RCCL transport, a fixed iteration count: likewise (lsf_slab_run_begin / _finish)
            return "library_slab_run"
        return "launches"

    def _launch_plan(self, grid, finalize, watched):
        """the sub-decisions of a launch-by-launch call (_LaunchPlan), from the same arguments as _route"""
        slab = self._slab()
        # SobolevFusion on band lists of a whole volume runs on the float4 layouts too (one vector-memory instruction per
        # neighbour / tap instead of one per component: lsf_sobolev_state.hip); z-slabs, filters of other lengths and
        # list-less runs keep the planar kernels
        sob_state = (self.sobolev and self.use_band_list and not slab and dev.buffer_addressing_ok(grid)
                     and len(self.sobolev_kernel) in dev.LISTED_TAP_COUNTS)
        planar_sobolev = self.sobolev and not sob_state
        # one pass: both states + the INTERIOR / BOUNDARY band lists of the WHOLE local array
        fused_prepare = not planar_sobolev and self.use_band_list and dev.buffer_addressing_ok(grid)
        # the listed finalize pass wants a zero-filled warp output (192 MB at 256^3, 26 us): filled in the call's
        # prologue, where the card waits for the host, instead of behind the last iteration.  Up to 256^3 IN FRONT of
        # the counting pass: the states written behind it are then the last thing to pass through the 256 MB Infinity
        # Cache before the first two iterations read them (filled behind the states it evicted them: 1.846-1.858
        # against 1.817-1.825 ms per step, three alternating runs on one box); a larger volume's fill (1.6 GB at
        # 512^3) would only keep the list sizes from the host (8.67 against 8.53 ms)
        fill_first = dev.n_voxels(grid) <= (1 << 24)
        fill = fused_prepare and finalize is not None and not slab
        warp_fill = ("before" if fill_first else "behind") if fill else None
        # whole 3-D volumes of whole boxes: everything behind the x pass box by box in one launch
        boxes = (sob_state and fused_prepare and not slab and self.sobolev_boxes and _SobolevStatePlan.fuses_x(grid)
                 and dev.boxes_ok(grid) and dev.n_voxels(grid) < (1 << 27)
                 and len(self.sobolev_kernel) in dev.LISTED_TAP_COUNTS)
        return _LaunchPlan(planar_sobolev, sob_state, fused_prepare, fused_prepare and self._slab_groups(),
                           fused_prepare and self._sparse_states(grid, watched), warp_fill, boxes)

    def optimize(self, live, canonical, finalize=None):
        """live, canonical: float32 device tensors (z-slab runs: the local slab incl. halos).  Returns a
        SlavchevaOutcome holding the final fields on the device; the caller's tensors are not modified.

        z-slab runs never abort on large warps (the reference only stops at 10 000 voxels,
        slavcheva_optimizer2d.py:360-362): an iteration is exact on a slab while its re-warp gather, floor(|w_z|) + 1
        slices, stays inside what the halo schedule keeps valid -- one slice inside an exchange group, the halo width
        with an exchange per iteration.  Every rank sees the same (reduced) maxima, so when a batch breaks that bound
        all ranks together discard the call's work and run it again from its inputs on a WIDER internal slab: halo
        ceil(max) + 1 (live and canonical slices fetched from the neighbours), the faces exchanged every iteration
        ("fall back to a wider exchange if the max exceeds 1").  The result is bit for bit the
        whole-volume one (tests/test_gpu_slab_many_ranks.py)."""
        if not self._slab():
            try:
                return self._optimize(live, canonical, finalize)
            except _SparseStateExceeded:
                # an update of SPARSE_REACH voxels or more may have gathered from a part of the states that was never
                # initialised.  The finalize pass has left the caller's tensors alone (its skip flag): the call runs again
                # on fully initialised states, and so does every later call of this optimizer (its data move that far)
                self.sparse_disabled = True
                torch.cuda.synchronize()
                return self._optimize(live, canonical, finalize)
        self._slab_restore = None
        try:
            outcome = self._optimize(live, canonical, finalize)
            self._slab_restore = None
            return outcome
        except _HaloTooNarrow as exc:
            torch.cuda.synchronize()  # nothing of the abandoned attempt (an exchange left in flight) may linger
            if self._slab_restore is not None:  # the abandoned attempt's finalize pass has written the caller's tensor
                self._slab_restore[0].copy_(self._slab_restore[1])
                self._slab_restore = None
            return self._optimize_widened(live, canonical, exc.max_update)

    def _optimize(self, live, canonical, finalize=None):
        """one attempt of optimize() (see there): route, set up, loop over batches, leave behind
        finalize = (live_out, lower_threshold, statistics): the arguments the caller is going to pass to
        outcome.finalize() -- with a fixed iteration count and a whole volume (no stop test can fire) the finalize pass is then enqueued
        right behind the last iteration and the records and statistics are read with ONE host synchronisation."""
        if live.shape != canonical.shape:
            raise ValueError("live and canonical fields must have the same shape")
        # what the previous call left for gradient_field() and its launcher still holds that call's ping-pong states: let
        # go of them BEFORE this call allocates its own, so that the allocator hands the same blocks out again (otherwise
        # the footprint doubles and the first three calls of an optimizer each pay device allocations: 120 / 131 / 70 ms
        # against 9 ms at 512^3, tools/step_times.py)
        self._gradient_state = None
        self._cumulative_state = None
        self._fast = None
        self.last_call = engine_options.new_call_report()
        grid = self._grid(live)
        # somebody looks at every iteration (the hook, the focus-neighbourhood trace): launched and synchronised one by one
        watched = self.iteration_hook is not None or self.focus_voxels is not None
        if self.focus_voxels is not None:
            self._focus_begin(live, canonical)
        route = self.last_call.route = self._route(grid, finalize, watched)
        if route in ("library_run", "library_sobolev_run"):
            return self._optimize_run(live, canonical, grid, finalize, sobolev=route == "library_sobolev_run")
        if route == "library_slab_run":
            return self._optimize_slab_run(live, canonical, grid, finalize)
        if self._slab():
            need = 1 if not self.sobolev else max(1, len(self.sobolev_kernel) // 2)
            if self.comm.layout.halo < need:
                raise ValueError("slab halo of %d slices is too narrow: this configuration needs >= %d"
                                 % (self.comm.layout.halo, need))
        plan = self._launch_plan(grid, finalize, watched)
        # with min_iterations == 0 the reference never enters its loop (max_warp starts at +inf, :354,:360-362)
        limit = 0 if self.min_iterations == 0 else max(self.max_iterations, self.min_iterations)
        iteration = self._set_up(live, canonical, grid, finalize, plan, limit)
        n_exec, dec = self._run_batches(iteration, plan, finalize, limit, watched)
        return self._leave_behind(iteration, n_exec, dec, limit)

    def _slab_cut_chunks(self, live, grid):
        """z-slabs whose slices are a multiple of 1024 voxels: the positions of the z cuts as chunk numbers, on the device
        (the prepare pass's per-chunk prefix counts hold the cuts' positions in the lists); else None"""
        if not (self._slab() and self.comm.layout.axis == 0 and (grid.ny * grid.nx) % dev.StatePrepare.CHUNK == 0):
            return None
        zs = self._slab_cut_slices(grid)
        key = (tuple(zs), grid.ny * grid.nx, live.device)
        if self._cut_chunk_cache[0] != key:
            per_slice = grid.ny * grid.nx // dev.StatePrepare.CHUNK
            self._cut_chunk_cache = (key, torch.tensor([z * per_slice for z in zs], dtype=torch.int64,
                                                       device=live.device))
        return self._cut_chunk_cache[1]

    def _set_up(self, live, canonical, grid, finalize, plan, limit):
        """states, lists, records and launch arguments of a launch-by-launch call: its iteration object"""
        slab, dims = self._slab(), grid.dims
        prepared = warp_zeroed = None
        if plan.fused_prepare:
            # one pass: both states + the INTERIOR / BOUNDARY band lists of the WHOLE local array.  Launched first: the
            # host sets up records and launch arguments while it runs, and only then waits for the list sizes -- and, in
            # a z-slab run, for the positions of the z cuts in the lists (slices of a multiple of 1024 voxels: the
            # prepare pass's per-chunk prefix counts hold them)
            cut_chunks = self._slab_cut_chunks(live, grid)
            if plan.warp_fill == "before":
                warp_zeroed = torch.zeros(tuple(live.shape) + (dims,), dtype=torch.float32, device=live.device)
            self.last_call.sparse_states = plan.sparse
            prepared = dev.StatePrepare(live, canonical, dev.full_range(grid), cut_chunks,
                                        sparse_reach=self.sparse_reach if plan.sparse else 0)
            if plan.warp_fill == "behind":
                warp_zeroed = torch.zeros(tuple(live.shape) + (dims,), dtype=torch.float32, device=live.device)
        live_at_entry = None
        if slab and finalize is not None and finalize[0] is not None and not plan.planar_sobolev \
                and self.min_iterations >= max(self.max_iterations, self.min_iterations):
            # the finalize pass of a fixed-count slab call is enqueued behind the last iteration, before the records of
            # every rank have said whether the call stands: what it overwrites is kept (a copy while the card waits for
            # the host anyway) -- instead of a launch, a synchronisation and a read-back behind the records
            live_at_entry = finalize[0].clone()
        records = dev.new_records(max(self.max_iterations, self.min_iterations, 1), live.device)
        if plan.planar_sobolev:
            iteration = _PlanarIteration(self, live, canonical, grid, records, limit)
            self._sobolev_band = iteration.band
            return iteration
        # Both ping-pong states start as (live, 0): the fused kernel only visits the voxels of the band list and
        # the rest must already hold their final values (lsf_slavcheva_state_iteration); slab halos start valid.
        listed = None
        states = prepared.states if plan.fused_prepare else dev.state_pack(live, None, grid, copies=2)
        n = dev.n_voxels(grid)
        f = _Fast(grid, records, gate=(_lib.GATE_SLAVCHEVA, self.lo, self.hi))
        f.p_state = [f.pointer(t, 4 * n, "state") for t in states]
        f.p_canon = f.pointer(canonical, n, "canonical")
        f.params_ref = ctypes.byref(self.params)
        f.stream = dev.stream_ptr()  # the launch stream of this call (one ctypes object, not one per launch)
        if plan.fused_prepare:
            bands, unlisted = prepared.collect()
            # z-slab runs: the lists cover the whole local array (owned slices + halos), like the dense finalize
            # pass does; the unlisted counts would too, so statistics (never asked for there) take the dense pass
            listed = (live, bands, None if slab else unlisted)
        else:
            bands = dev.band_lists(live, canonical, dev.full_range(grid)) if self.use_band_list \
                else [dev.BandList.none()]
        f.bands = bands
        self._fast = f
        if plan.sob_state:
            g4 = [torch.zeros(tuple(live.shape) + (4,), dtype=torch.float32, device=live.device)
                  for _ in range(2 if _SobolevStatePlan.fuses_x(grid) else 3)]
            n_max = max(self.max_iterations, self.min_iterations)
            every = self.iteration_hook is not None or self.min_iterations < n_max
            boxes = dev.band_boxes(prepared, _lib.BAND_ALL) if plan.sobolev_boxes else None
            self.last_call.sobolev_boxes = boxes is not None
            iteration = _SobolevStatePlan(f, states, canonical, grid, self.params, bands, g4, self.sobolev_kernel,
                                          self.min_iterations, n_max, gradient_every_iteration=every, boxes=boxes)
            self._sobolev_band = _Counted(sum(b.count for b in bands))  # what bench.py prices this path over
        else:
            psi = None
            if self.cumulative_warp:
                # two zero-filled PSI buffers in the state's layout, ping-pong with the states; allocated per attempt, so
                # a call that runs again on fully initialised states composes from zeros again
                psi = [torch.zeros(tuple(live.shape) + (4,), dtype=torch.float32, device=live.device) for _ in range(2)]
                f.p_psi = [f.pointer(t, 4 * n, "cumulative warp") for t in psi]
            iteration = _FusedIteration(self, f, limit, psi, (prepared, live) if plan.sparse else None)
        iteration.hold(states, canonical, grid, records, listed=listed, sparse=prepared if plan.sparse else None,
                       warp_zeroed=warp_zeroed, live_at_entry=live_at_entry)
        if slab:
            self._plan_slab(f, live, grid, bands, limit, prepared if plan.fused_prepare and prepared.cuts is not None
                            else None)
        return iteration

    def _run_batches(self, iteration, plan, finalize, limit, watched):
        """enqueue the iterations batch by batch, read and judge every batch: (executed iterations, decoded records)"""
        slab, records = self._slab(), iteration.records
        done, n_exec, dec = 0, 0, None
        while done < limit:
            # a run whose stop test cannot fire (min_iterations == max_iterations) has nothing to look at in between: all of
            # it is enqueued at once, whatever check_interval says
            batch = 1 if watched else (limit - done if self.min_iterations >= limit
                                       else min(self.check_interval, limit - done))
            for i in range(done, done + batch):
                iteration.enqueue(i)
            # z-slab: a gated run's device-side gate reads the records, so they are all-reduced (global max: idempotent;
            # once per record the energy sums of this batch); a fixed count only needs them on the host: every rank's
            # partial slots are gathered when they are read
            ungated = self.min_iterations >= limit
            if slab and not ungated:
                self.comm.reduce_records(records, done, done + batch)
            done += batch
            if finalize is not None and done == limit and self.min_iterations >= limit:
                iteration.finalize_early(finalize, records, limit, self.sparse_reach)
                self._slab_restore = iteration.restore
            dec = dev.decode_records(self.comm.gather_records(records, 0, done) if slab and ungated
                                     else dev.records_to_host(records[:done]))
            n_exec = int(dec["executed"].sum())
            # z-slab: every EXECUTED iteration must have stayed inside what the halo schedule keeps valid -- also those
            # of a batch in which the gate then closed (a large update followed by convergence inside one
            # check_interval).  Every rank sees the same reduced / gathered records, so the raise is collective.
            if plan.sparse and not slab and n_exec > 0 and not dec["max_value"][:n_exec].max() < self.sparse_reach:
                raise _SparseStateExceeded()  # (a slab's exchange groups stop at one voxel: _HaloTooNarrow below)
            reach = self.comm.layout.halo if slab else 0
            if slab and not self.sobolev and self._fast.exchange_interval > 1:
                reach = 1  # inside an exchange group every iteration may consume one slice of validity only
            if slab and n_exec > 0 and not (dec["max_value"][:n_exec].max() < reach):
                raise _HaloTooNarrow(float(dec["max_value"][:n_exec].max()), reach)
            if n_exec < done:
                break
            m = dec["max_value"][n_exec - 1]
            if self.focus_voxels is not None:
                self._probe_focus(done - 1, iteration)
            if self.iteration_hook is not None:
                self._call_hook(done - 1, float(m), iteration)
            if n_exec >= self.min_iterations and not (np.float32(self.lo) < m < np.float32(self.hi)):
                break
        return n_exec, dec

    def _leave_behind(self, iteration, n_exec, dec, limit):
        """the call stands: count, log, the sources of the two fields, the outcome"""
        self.iteration_count = n_exec
        if self.cumulative_warp:
            self._cumulative_state = iteration.cumulative_source(n_exec)
        wd, ws, wl = self.weights
        if dec is None:
            dec = dev.decode_records(dev.records_to_host(iteration.records[:1]))
        self.log = dict(max_warps=dec["max_value"][:n_exec].tolist(),
                        max_warp_indices=dec["argmax"][:n_exec].tolist(),
                        data_energies=(wd * dec["data_energy"][:n_exec]).tolist(),
                        smoothing_energies=(ws * dec["smoothing_energy"][:n_exec]).tolist(),
                        level_set_energies=(wl * dec["level_set_energy"][:n_exec]).tolist())
        outcome = iteration.outcome(n_exec, limit)
        # what is needed to (re)produce gradient_field of the last executed iteration on demand
        if n_exec == 0:
            like = iteration.canonical
            zeros = torch.zeros((iteration.grid.dims,) + tuple(like.shape), dtype=torch.float32, device=like.device)
            self._gradient_state = _Lazy(lambda: zeros)
        else:
            self._gradient_state = iteration.gradient_source(n_exec)
        return outcome

    def _call_hook(self, i, max_warp, iteration):
        """iteration i has run: hand its warp and gradient to the hook in the API layout (owned slices of a slab)"""
        warp_planar, g = iteration.after(i)
        own = (slice(None), self.comm.layout.owned_local()) if self._slab() else (slice(None),)
        self.iteration_hook(0, i, dev.interleave(warp_planar[own].contiguous()), dev.interleave(g[own].contiguous()),
                            max_warp)

    def cumulative_warp_field(self):
        """PSI of the last call in the API layout [..., D] (x, y[, z] channels), a float32 device tensor built when first
        read; None before the first call and without cumulative_warp"""
        source = self._cumulative_state
        return None if source is None else source.get()

    def gradient_field(self):
        """planar gradient of the last executed iteration (zeroed where the live field snapped, DIRECT only); made when
        first read (engine_outcome.recompute_gradient, the SobolevFusion plans' final buffer, a wider re-run's field)"""
        source = self._gradient_state
        return None if source is None else source.get()
