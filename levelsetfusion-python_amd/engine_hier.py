"""HierarchicalEngine: coarse-to-fine gradient descent on a cumulative warp field, D = 2 or 3, whole volumes and
z-slabs (nonrigid_opt/hierarchical/hierarchical_optimizer2d.py:123-246).  The drop-in classes
HierarchicalOptimizer2d / 3d are thin shells around it."""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, device as dev, engine_options
from .engine_common import _CAPTURE_LOCK, _RETIRED_GRAPHS, _combine_statistics, _conv_axis_order, _retire_graphs
from .engine_hier_pyramid import build_pyramids


class LevelResult:
    def __init__(self, iteration_count, max_updates, argmax, data_energies, voxel_count=0, tikhonov_energies=()):
        self.voxel_count = voxel_count
        self.tikhonov_energies = list(tikhonov_energies)  # sum |np.gradient(previous gradient)|^2 per iteration
        self.iteration_count = iteration_count
        self.max_updates = max_updates
        self.argmax = argmax
        self.data_energies = data_energies
        self.iteration_limit_reached = False


class HierarchicalEngine:
    """coarse-to-fine gradient descent on a cumulative warp field
    (nonrigid_opt/hierarchical/hierarchical_optimizer2d.py:123-246), D = 2 or 3."""

    def __init__(self, tikhonov_term_enabled, gradient_kernel_enabled, maximum_chunk_size, rate,
                 maximum_iteration_count, maximum_warp_update_threshold, data_term_amplifier, tikhonov_strength,
                 kernel, compute_energy=False, check_interval=32, collect_reports=False, comm=None,
                 collect_iteration_data=False, linear_resampling=False, options=None):
        # use_graphs, graph_max_voxels, fused_filter, fused_filter_min_voxels, defer_maximum, blocked_levels
        engine_options.apply(self, engine_options.HIERARCHICAL_DEFAULTS, options)
        self.graph_max_voxels = int(self.graph_max_voxels)
        self.last_call = engine_options.new_call_report()
        # False: levels without a captured graph run eagerly (same results) -- set while optimizers work side by side in
        # several host threads: HIP refuses ordinary calls of OTHER threads while a capture is in progress
        self.allow_graph_capture = True
        self._graphs = {}
        self.linear_resampling = linear_resampling  # ResamplingStrategy.LINEAR (3-D): math_utils/resampling.py
        self.collect_reports = collect_reports
        self.collect_iteration_data = collect_iteration_data  # telemetry: per-iteration warp / gradient snapshots
        self.iteration_data = []
        # opt-in per-iteration call-back, f(level, iteration, warp, gradient, max_update) with device tensors in the API
        # layout [..., D]: where the reference calls its visualiser inside the loop (hierarchical_optimizer2d.py:242-245).
        # None (default): nothing is synchronised or copied per iteration; set: every iteration is read back at once.
        self.iteration_hook = None
        self.comm = comm  # SlabComm of the FINEST level (z-slab runs), or None
        self.maximum_chunk_size = maximum_chunk_size
        self.rate = rate
        self.data_term_amplifier = data_term_amplifier
        # enable-flag folding of hierarchical_optimizer2d.py:96-107
        if tikhonov_term_enabled:
            self.tikhonov_strength = tikhonov_strength
            self.tikhonov_term_enabled = tikhonov_strength != 0.0
        else:
            self.tikhonov_strength = 0.0
            self.tikhonov_term_enabled = False
        if gradient_kernel_enabled:
            self.gradient_kernel = kernel
            self.gradient_kernel_enabled = kernel is not None
        else:
            self.gradient_kernel = None
            self.gradient_kernel_enabled = False
        self.maximum_warp_update_threshold = maximum_warp_update_threshold
        self.maximum_iteration_count = int(maximum_iteration_count)
        self.compute_energy = compute_energy
        self.check_interval = max(1, int(check_interval))
        self.level_results = []
        self.last_gradient = None  # planar gradient of the finest level after the last iteration
        # z-slab runs: levels whose gather operand had to be replicated on every rank because the cumulative warp outgrew
        # the halo (_optimize_level_slab); once a level needed it the finer ones start that way -- warps are not rescaled
        # between levels (hierarchical_optimizer2d.py:155-156), so they only grow
        self.replicated_levels = 0

    def optimize(self, canonical, live):
        """canonical, live: float32 device tensors [z,]y,x (z-slab runs: the local slab incl. halos).
        Returns the warp field, PLANAR [c][z][y][x] (z-slab runs: local extent, only owned slices are meaningful)."""
        if canonical.shape != live.shape:
            raise ValueError("canonical and live fields must have the same shape")
        dims = live.dim()
        self.last_call = engine_options.new_call_report()
        canon_levels, packed_levels, comms = build_pyramids(canonical, live, self.maximum_chunk_size,
                                                            self.linear_resampling, self.comm)
        self.level_results, self.iteration_data, self.replicated_levels = [], [], 0
        waiting = []  # outcomes of levels whose results are made later (level_results stays in level order)
        warp = torch.zeros((dims,) + tuple(canon_levels[0].shape), dtype=torch.float32, device=live.device)
        for level, (canon_l, packed_l, comm_l) in enumerate(zip(canon_levels, packed_levels, comms)):
            waiting.append(self.optimize_level(canon_l, packed_l, warp, comm_l))
            if not waiting[-1].deferred:
                self._finish_levels(waiting)
            if level != len(canon_levels) - 1:
                if self.linear_resampling:
                    if comm_l is not None:
                        # the lerp of a slab's first / last fine slices reads the neighbour's adjacent coarse slice;
                        # iterations never touch the warp's halo slices (the warp is only read voxel by voxel)
                        comm_l.exchange_halos([warp], width=1)
                    fine = torch.stack([dev.upsample2x_linear(warp[c].contiguous()) for c in range(dims)])
                else:
                    fine = dev.prolong_repeat(warp)
                if comm_l is not None:  # keep [owned + halo] of the finer level's layout
                    lo = comm_l.layout.halo_lo
                    fine = fine[:, lo:lo + comms[level + 1].layout.nz_local].contiguous()
                warp = fine
        self._finish_levels(waiting)
        return warp

    # ------------------------------------------------------------------------------------------------
    # One level.  Gradient buffers: F[0], F[1] alternate as "previous gradient" / "this iteration's final gradient"
    # (iteration i reads F[i % 2], leaves its result in F[(i + 1) % 2]); with a gradient kernel the raw gradient and the
    # intermediate filter passes ping-pong between two scratch buffers and the LAST pass writes F[(i + 1) % 2].  The
    # buffer roles therefore repeat with period 2, which is what lets a batch of iterations be captured ONCE as a HIP
    # graph and replayed (launch-bound levels: 2-D fields, coarse 3-D levels).
    def _filter_plan(self, grid, full_grid, warp, S, comm):
        """the launches behind lsf_hier_iteration that filter the raw gradient in S[0] into this iteration's F, decided
        once per level: steps (run, src, dst) -- run(src, dst, gate) enqueues one, dst None = F -- and whether the last
        one also moves the warp by the gradient it writes"""
        taps, rate, fused, steps = self.gradient_kernel, self.rate, self.fused_filter, []
        if comm is not None:  # z-slab: the z pass reads taps / 2 slices of the (x,y)-filtered field on either side
            steps.append((lambda src, dst, gate: comm.exchange_halos([src], width=len(taps) // 2), S[0], S[0]))
        if fused and dev.n_voxels(grid) >= self.fused_filter_min_voxels and dev.convolve_xyz_ok(grid, taps):
            # x, y, z in one launch, which also moves the warp by its filtered gradient, component by component
            steps.append((lambda src, dst, gate: dev.convolve_xyz(src, dst, grid, taps, gate, warp, rate), S[0], None))
            return steps, True
        axes, src = _conv_axis_order(grid.dims), S[0]
        if len(axes) == 3 and fused and dev.convolve_xy_ok(full_grid, taps):
            # smaller 3-D levels: the x and the y pass in one launch (these levels are launch-bound)
            steps.append((lambda src, dst, gate: dev.convolve_xy(src, dst, full_grid, taps, gate), S[0], S[1]))
            axes, src = axes[2:], S[1]
        # the last pass moves the warp by the gradient it writes, instead of lsf_hier_update reading the gradient again
        moves_warp = dev.convolve_axis_update_ok(grid, taps)
        for axis in axes:
            last = axis == axes[-1]
            dst = None if last else (S[0] if src is S[1] else S[1])
            g = grid if axis == 2 else full_grid
            if last and moves_warp:
                run = lambda src, dst, gate, g=g, a=axis: dev.convolve_axis_update(src, dst, warp, rate, g, a, taps, gate)
            else:
                run = lambda src, dst, gate, g=g, a=axis: dev.convolve_axis(src, dst, None, g, a, taps, gate)
            steps.append((run, src, dst))
            src = dst
        return steps, moves_warp

    def _make_level(self, canonical, packed, warp, grid, full_grid, n_records, packed_global=None, comm=None):
        """packed_global: the packed live field of the WHOLE level (every rank's owned slices, SlabComm.all_gather_owned)
        for the gather instead of the local slab + halo; comm: the level's SlabComm (z-slab runs)"""
        dims, tik, ker = canonical.dim(), self.tikhonov_term_enabled, self.gradient_kernel_enabled
        params = _lib.HierParams(float(self.data_term_amplifier), float(self.tikhonov_strength), float(self.rate),
                                 int(tik), int(not ker), int(self.compute_energy))
        if packed_global is not None:
            params.packed_nz, params.packed_z_global_offset = int(packed_global.shape[0]), 0
        F = [torch.zeros_like(warp) for _ in range(2)] if (tik or ker) else []
        S = [torch.zeros_like(warp) for _ in range(2)] if ker else []
        report_g = torch.zeros_like(warp) if (self.collect_reports and not F) else None
        records = dev.new_records(n_records, canonical.device)
        f = dev.IterationLauncher(grid, records, _lib.GATE_HIERARCHICAL, float(self.maximum_warp_update_threshold))
        n = dev.n_voxels(grid)
        steps, moves_warp = self._filter_plan(grid, full_grid, warp, S, comm) if ker else ([], False)
        # Deferred maximum (3-D levels whose filter moves the warp itself, Tikhonov on): when the stop test cannot fire
        # (threshold <= 0) the maximum update length is only a log value, and the NEXT iteration's kernel reads the
        # gradient it belongs to anyway (as g_prev, for the Laplacian): that kernel writes it into the previous record
        # (lsf_hier_params::previous_max, an LSF_GATE_OPEN gate naming the record), and only the last iteration of a
        # batch keeps the separate maximum pass (44 us of 520 per 256^3 iteration).  Slab levels reduce every iteration's
        # maximum over the ranks, the hook and the telemetry look at every iteration: they keep the pass.
        defer_max = bool(dims == 3 and tik and moves_warp and float(self.maximum_warp_update_threshold) <= 0.0
                         and self.defer_maximum and comm is None and self.iteration_hook is None
                         and not self.collect_iteration_data)
        prevmax, open_gates = _lib.HierParams.from_buffer_copy(params), []
        if defer_max:
            prevmax.previous_max = 1
            open_gates = [_lib.Gate(records.data_ptr() + i * _lib.RECORD_BYTES, _lib.GATE_OPEN, 0.0, 0.0)
                          for i in range(n_records)]
        return _Level(
            canonical=canonical, packed=packed, packed_global=packed_global, warp=warp, grid=grid, comm=comm, params=params,
            params_ref=ctypes.byref(params), F=F, S=S, report_g=report_g, records=records, launcher=f, steps=steps,
            moves_warp=moves_warp,
            p_packed=f.pointer(packed, 4 * n, "packed live") if packed_global is None else
            f.pointer(packed_global, packed_global.numel(), "packed live (whole level)"),
            p_canon=f.pointer(canonical, n, "canonical"), p_warp=f.pointer(warp, n * dims, "warp"),
            p_F=[f.pointer(t, n * dims, "gradient buffer") for t in F],
            p_S=[f.pointer(t, n * dims, "scratch buffer") for t in S],
            p_report=f.pointer(report_g, n * dims, "gradient", allow_none=True), defer_max=defer_max, prevmax=prevmax,
            prevmax_ref=ctypes.byref(prevmax), open_gates=open_gates, open_gate_refs=[ctypes.byref(g) for g in open_gates])

    def _graph_key(self, canonical):
        K = min(self.check_interval, self.maximum_iteration_count)
        return (tuple(canonical.shape), canonical.device, K - K % 2)

    def invalidate_graphs(self):
        """a setting changed: captured graphs hold the old rate / threshold / taps / iteration counts"""
        _retire_graphs(self._graphs)

    def __del__(self):
        try:
            _retire_graphs(self._graphs)
        except Exception:  # noqa: BLE001 -- interpreter shutdown: nothing left to protect
            pass

    def _enqueue(self, lv, rec_idx, prev_idx, parity, defer_max=False, prev_deferred=False):
        """one iteration: record slot rec_idx, gated on record prev_idx (None: always runs), buffer parity 0/1.
        defer_max: leave this iteration's maximum to the next one (see _make_level); prev_deferred: the previous did"""
        f = lv.launcher
        gated = prev_idx is not None and prev_idx >= 0
        # the gradient kernel: after the previous gradient (Tikhonov term) it writes the raw gradient for the filter,
        # this iteration's gradient (it then moves the warp itself) or, with neither term, the reports' gradient
        prev = lv.p_F[parity] if self.tikhonov_term_enabled else None
        first = lv.p_S[0] if lv.steps else (lv.p_F[1 - parity] if lv.F else lv.p_report)
        params_ref, gate_ref = lv.params_ref, f.gate_ref(prev_idx)
        if prev_deferred and gated:
            params_ref, gate_ref = lv.prevmax_ref, lv.open_gate_refs[prev_idx]
        _lib.check(_lib.lib.lsf_hier_iteration(lv.p_packed, lv.p_canon, lv.p_warp, prev, first, f.grid_ref, params_ref,
                                               gate_ref, f.record_ptrs[rec_idx], dev.stream_ptr()), "lsf_hier_iteration")
        if not lv.steps:
            return
        gate, out = (f.gates[prev_idx] if gated else None), lv.F[1 - parity]
        for run, src, dst in lv.steps:
            run(src, out if dst is None else dst, gate)
        if not (lv.moves_warp and defer_max):
            dev.hier_update(out, None if lv.moves_warp else lv.warp, lv.grid, self.rate, gate, lv.records, rec_idx)

    def _read_batch(self, records, log):
        """the one host synchronisation of a batch of iterations: their records, decoded, the executed ones added to `log`;
        returns (executed iterations, whether the level ends here: a gate closed or the last maximum is below the threshold)"""
        dec = dev.decode_records(dev.records_to_host(records))
        k_exec = int(dec["executed"].sum())
        log.append({k: v[:k_exec].copy() for k, v in dec.items()})
        return k_exec, bool(k_exec < records.shape[0]
                            or dec["max_value"][k_exec - 1] < np.float32(self.maximum_warp_update_threshold))

    @staticmethod
    def _merged(log):
        if not log:  # maximum_iteration_count == 0: the reference's loop body never runs
            return dev.decode_records(np.zeros((1, dev.RECORD_WORDS), np.int64))
        return {k: np.concatenate([part[k] for part in log]) for k in log[0]}

    def _finish_levels(self, outcomes):
        """results (and reports) of levels in level order; the records that are still on the card -- the fixed-count
        levels of _optimize_level_blocked -- are read in ONE transfer with ONE synchronisation"""
        unread = [o for o in outcomes if o.decoded is None]
        if unread:
            used = torch.cat([dev.slot_view(o.records)[:, :, :dev.USED_SLOT_WORDS].reshape(-1) for o in unread])
            host = dev.pinned_scratch("level records", used.numel(), torch.int64)[:used.numel()]
            host.copy_(used, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            flat, at = host.numpy(), 0
            for o in unread:
                n = o.records.shape[0]
                words = n * _lib.RECORD_SLOTS * dev.USED_SLOT_WORDS
                o.decoded = dev.decode_records(flat[at:at + words].reshape(n, _lib.RECORD_SLOTS, -1).copy())
                o.n_exec = int(o.decoded["executed"].sum())
                at += words
        for o in outcomes:
            self._finish_level(o)
        del outcomes[:]

    def _finish_level(self, o):
        thr = float(self.maximum_warp_update_threshold)
        L = o.comm.layout if o.comm is not None else None
        n_exec, dec = o.n_exec, o.decoded
        n_vox = dev.n_voxels(o.grid) if L is None else L.nz_global * o.grid.ny * o.grid.nx
        log = lambda key, kind=float: [kind(v) for v in dec[key][:n_exec]]
        res = LevelResult(n_exec, log("max_value"), log("argmax", int), log("data_energy"), n_vox, log("smoothing_energy"))
        res.iteration_limit_reached = n_exec >= self.maximum_iteration_count
        self.level_results.append(res)
        self.last_gradient = o.gradient
        if not self.collect_reports:
            return
        # per-level ConvergenceReport (cpp get_per_level_convergence_reports, run_hierarchical_optimizer3d.py:104):
        # statistics of the last iteration's update field and of |canonical - resampled live| at this level
        from .convergence_report import (ConvergenceReport, tsdf_difference_statistics_from_raw,
                                         warp_delta_statistics_from_raw)
        g_final = o.gradient if o.gradient is not None else torch.zeros_like(o.warp)
        if L is None:
            shape = tuple(o.canonical.shape)
            resampled = dev.warp_field(o.packed[..., 0].contiguous(), o.warp, 1.0)
            raw_warp = dev.warp_statistics(g_final, o.canonical, resampled, thr).cpu().numpy()
            raw_tsdf = dev.tsdf_difference_statistics(o.canonical, resampled).cpu().numpy()
        else:
            # z-slab: the same statistics over the OWNED slices (global voxel indices through z_global_offset), then
            # combined over the ranks -- counts and sums add, minima / maxima compare, the arg-max of the larger
            # maximum wins (smallest index on a tie, as np.argmax over the whole volume)
            shape = (L.nz_global,) + tuple(o.canonical.shape[1:])
            resampled = self._slab_resampled(o, L)
            raw = torch.stack([dev.warp_statistics(g_final, o.canonical, resampled, thr, o.grid),
                               dev.tsdf_difference_statistics(o.canonical, resampled, o.grid)])
            rows = o.comm.gather_rows(raw)
            raw_warp = _combine_statistics([r[0] for r in rows], has_min=False)
            raw_tsdf = _combine_statistics([r[1] for r in rows], has_min=True)
        res.report = ConvergenceReport(n_exec, res.iteration_limit_reached,
                                       warp_delta_statistics_from_raw(raw_warp, shape, thr, float("inf")),
                                       tsdf_difference_statistics_from_raw(raw_tsdf, shape))

    @staticmethod
    def _slab_resampled(o, L):
        """the live field of a slab level under its warp, on every local slice"""
        if o.packed_global is None:
            whole = dev.make_grid(o.canonical.shape, 0, L.nz_local, L.z_global_offset)
            return dev.warp_field(o.packed[..., 0].contiguous(), o.warp, 1.0, whole)
        # the warp reaches past the halo: resample the replicated live field under the whole level's warp (every
        # rank the same work; reports are an opt-in) and keep the owned slices
        warp_g = torch.stack([o.comm.all_gather_owned(o.warp[c]) for c in range(o.warp.shape[0])])
        whole_level = dev.warp_field(o.packed_global[..., 0].contiguous(), warp_g, 1.0)
        resampled = torch.zeros_like(o.canonical)
        resampled[L.owned_local()] = whole_level[L.z0:L.z1]
        return resampled

    OPEN_RECORD = 0x7F800000FFFFFFFF  # packed max = +inf: "previous iteration has not converged" for the gate

    def optimize_level(self, canonical, packed, warp, comm=None):
        """one level by the driver that fits it; the level's warp is advanced in place, returns the _LevelOutcome"""
        comm = comm if comm is not None and comm.active else None
        max_it = self.maximum_iteration_count
        watched = self.iteration_hook is not None or self.collect_iteration_data  # every iteration is looked at
        if (self.blocked_levels and canonical.dim() == 2 and comm is None and not watched
                and not self.compute_energy and max_it >= 1
                and (not self.gradient_kernel_enabled or len(self.gradient_kernel) in dev.XYZ_TAP_COUNTS)):
            return self._optimize_level_blocked(canonical, packed, warp)
        if (self.use_graphs and comm is None and not watched and max_it >= 4
                and self.check_interval >= 2 and canonical.numel() <= self.graph_max_voxels
                and (self.allow_graph_capture or self._graph_key(canonical) in self._graphs)):
            return self._optimize_level_graph(canonical, packed, warp)
        if comm is not None:
            return self._optimize_level_slab(canonical, packed, warp, comm)
        grid = dev.make_grid(canonical.shape)
        return self._optimize_level_eager(self._make_level(canonical, packed, warp, grid, grid, max(max_it, 1)))

    def _optimize_level_slab(self, canonical, packed, warp, comm):
        """a z-slab's level.  The gather follows the cumulative warp: it must stay inside the halo of the static packed
        field.  When it does not, the reference does not stop either (hierarchical_optimizer2d.py:169-171 tests the update
        threshold only): every rank sees the same reduced maximum, so all of them together discard this level's
        iterations, replicate the level's packed field (5 x 512 MiB at 512^3 against 288 GB) and run the
        level again from the warp it started with -- the gather then never leaves the device"""
        L = comm.layout
        grid = dev.make_grid(canonical.shape, L.z_begin, L.z_end, L.z_global_offset)
        full_grid = dev.make_grid(canonical.shape, 0, L.nz_local, L.z_global_offset)
        reach = len(self.gradient_kernel) // 2 if self.gradient_kernel_enabled else 0
        if L.halo < max(reach, 2):
            raise ValueError("slab halo of %d slices is too narrow: this configuration needs >= %d"
                             % (L.halo, max(reach, 2)))
        def run(packed_global):
            return self._optimize_level_eager(self._make_level(canonical, packed, warp, grid, full_grid,
                                                               max(self.maximum_iteration_count, 1), packed_global, comm))
        if self.replicated_levels == 0:
            warp_at_start = warp.clone()
            outcome = run(None)
            if outcome is not None:
                return outcome
            warp.copy_(warp_at_start)
            self.replicated_levels = 1
        self.replicated_levels += 1
        return run(comm.all_gather_owned(packed))

    def _optimize_level_eager(self, lv):
        """one foreign call per launch, check_interval iterations (one, under a hook) per host synchronisation.  Returns
        the outcome -- or None: the warp of a slab level left the halo of its local packed field"""
        max_it, hook, comm = self.maximum_iteration_count, self.iteration_hook, lv.comm
        log, snapshots, it, n_exec = [], [], 0, 0
        while it < max_it:
            batch = 1 if hook is not None else min(self.check_interval, max_it - it)
            for i in range(it, it + batch):
                if self.collect_iteration_data:
                    snapshots.append(self._term_snapshots(lv, i))
                self._enqueue(lv, i, i - 1 if i > 0 else None, i % 2, defer_max=lv.defer_max and i + 1 < it + batch,
                              prev_deferred=lv.defer_max and i > it)
                if self.collect_iteration_data:
                    snapshots[-1][0] = lv.warp.clone()
                if comm is not None:
                    if self.tikhonov_term_enabled:  # the next Laplacian reads one slice of this gradient on either side
                        comm.exchange_halos([lv.F[(i + 1) % 2]], width=1)
                    if i + 1 < max_it:
                        comm.reduce_max(lv.records, i)  # the next iteration's gate tests the GLOBAL max
            if comm is not None:
                comm.reduce_records(lv.records, it, it + batch)
            k_exec, ended = self._read_batch(lv.records[it:it + batch], log)
            it, n_exec = it + batch, n_exec + k_exec
            if comm is not None and lv.packed_global is None:
                wz = lv.warp[2][comm.layout.owned_local()].abs().max().reshape(1)
                comm.reduce_scalar_max(wz)
                if not (float(wz.item()) < comm.layout.halo - 1):
                    return None
            if hook is not None and k_exec == batch:  # iteration it - 1 ran: its gradient is in the buffer the next reads
                g_now = lv.F[it % 2] if lv.F else lv.report_g
                own = (slice(None), comm.layout.owned_local()) if comm is not None else (slice(None),)
                # (a watched level is never deferred: level_results holds every coarser level)
                hook(len(self.level_results), it - 1, dev.interleave(lv.warp[own].contiguous()),
                     dev.interleave(g_now[own].contiguous()), float(log[-1]["max_value"][-1]))
            if ended:
                break
        if self.collect_iteration_data:
            self.iteration_data.append(snapshots[:n_exec])  # snapshots of gated (not executed) launches are dropped
        # iteration n_exec - 1 wrote F[((n_exec - 1) + 1) % 2]
        return _LevelOutcome(lv.canonical, lv.packed, lv.warp, lv.grid, lv.F[n_exec % 2] if lv.F and n_exec else lv.report_g,
                             self._merged(log), n_exec, packed_global=lv.packed_global, comm=comm)

    def _term_snapshots(self, lv, i):
        """telemetry (cpp LoggingParameters.collect_per_level_iteration_data): the two gradient terms the reference hands
        to its visualiser (hierarchical_optimizer2d.py:196,202,242-245) are produced by two extra launches of the same
        kernel on the pre-update warp: [the warp after the iteration (the caller's to fill in), data term, Tikhonov term]"""
        gate = lv.launcher.gates[i - 1] if i > 0 else None
        gathered = lv.packed if lv.packed_global is None else lv.packed_global
        wide = (0, 0, 0, 0) if lv.packed_global is None else (0, 0, int(lv.packed_global.shape[0]), 0)
        terms = [(None, _lib.HierParams(1.0, 0.0, 0.0, 0, 0, 0, *wide))]
        if self.tikhonov_term_enabled:  # laplace(previous gradient) = 0*gd - (-1)*lap
            terms.append((lv.F[i % 2], _lib.HierParams(0.0, -1.0, 0.0, 1, 0, 0, *wide)))
        snapshots = [None, None, None]
        for k, (g_prev, params) in enumerate(terms, 1):
            snapshots[k] = torch.zeros_like(lv.warp)
            dev.hier_iteration(gathered, lv.canonical, lv.warp, g_prev, snapshots[k], lv.grid, params, gate, lv.records, i)
        return snapshots

    # ------------------------------------------------------------------------------------------------
    BLOCKED_ITERATIONS_PER_LAUNCH = 8

    def _optimize_level_blocked(self, canonical, packed, warp):
        """2-D levels, no energy printouts: the whole level in ONE foreign call, K = 8 iterations
        per launch advanced inside LDS tile by tile (lsf_hier_level_run_2d: temporal blocking -- a 512^2 level is
        launch-bound, 7.5 us per iteration from a HIP graph against ~1 us of work).  With the gradient kernel (the
        reference's default constructor) the launch also runs the filter's two passes and the update behind them -- one
        launch instead of four per iteration -- and an iteration consumes taps / 2 + 1 rings of a tile's surroundings: K = 2
        for seven taps.  Same arithmetic on the same inputs:
        warp, gradient and every iteration's maximum equal the per-iteration path's (tests/test_gpu_blocked_levels.py).
        A stop test that can fire (threshold > 0, hierarchical_optimizer2d.py:169-171) is looked at launch by launch on
        the card; the launch in which the level converged is then repeated from its untouched inputs with the reference's
        number of iterations, so the level ends exactly where the reference's ends."""
        max_it = self.maximum_iteration_count
        grid = dev.make_grid(canonical.shape)
        n = dev.n_voxels(grid)
        K = self.BLOCKED_ITERATIONS_PER_LAUNCH
        taps, n_taps = None, 0
        if self.gradient_kernel_enabled:
            kernel = np.ascontiguousarray(np.asarray(self.gradient_kernel, dtype=np.float64))
            n_taps = int(kernel.size)
            if min(canonical.shape) < n_taps:  # (the reference cannot do this either: np.convolve's 'same' mode)
                raise ValueError("cannot convolve a field of extent %d with a %d-tap kernel" % (min(canonical.shape), n_taps))
            taps = kernel.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        # rings of a tile's surroundings an iteration consumes: one for the Tikhonov term's Laplacian, taps / 2 for the filter
        rings = int(bool(self.tikhonov_term_enabled)) + n_taps // 2
        if rings:
            K = max(1, K // rings)
        thr = np.float32(self.maximum_warp_update_threshold)
        gated = bool(thr > 0.0)
        warps = [warp, torch.empty_like(warp)]
        F = [torch.zeros_like(warp), torch.empty_like(warp)]
        records = dev.new_records(max_it, canonical.device)
        params = _lib.HierParams(float(self.data_term_amplifier), float(self.tikhonov_strength), float(self.rate),
                                 int(bool(self.tikhonov_term_enabled)), int(n_taps == 0), 0)
        ptr = dev.checked_pointer
        p_packed, p_canonical = ptr(packed, 4 * n, "packed live"), ptr(canonical, n, "canonical")
        p_warp, p_g = [ptr(w, 2 * n, "warp") for w in warps], [ptr(g, 2 * n, "gradient") for g in F]

        def run(first, record_ptr, iterations, threshold):  # launches reading pair `first` first
            _lib.check(_lib.lib.lsf_hier_level_run_2d(
                p_packed, p_canonical, p_warp[first], p_warp[1 - first], p_g[first], p_g[1 - first], ctypes.byref(grid),
                ctypes.byref(params), taps, n_taps, record_ptr, iterations, K, threshold, dev.stream_ptr()),
                "lsf_hier_level_run_2d")

        run(0, ctypes.c_void_p(records.data_ptr()), max_it, float(thr) if gated else 0.0)
        launches = (max_it + K - 1) // K
        dec = n_exec = None
        if gated:
            dec = dev.decode_records(dev.records_to_host(records[:max_it]))
            ran = int(dec["executed"].sum())  # whole launches: a multiple of K, or every iteration
            below = np.nonzero(dec["max_value"][:ran] < thr)[0]
            n_exec = int(below[0]) + 1 if below.size else ran
            last = (n_exec - 1) // K  # the launch the level ended in; the ones behind it were no-ops
            if n_exec < min((last + 1) * K, max_it):
                # ... in the middle of it: once more from its inputs, as many iterations as the reference runs
                run(last % 2, ctypes.c_void_p(dev.new_records(K, canonical.device).data_ptr()), n_exec - last * K, 0.0)
            launches = last + 1
        if launches % 2:
            warp.copy_(warps[1])
        self.last_call.blocked_levels += 1
        # (what the per-iteration drivers leave: with neither term there are no F buffers, and a gradient only for reports)
        keep = self.tikhonov_term_enabled or self.gradient_kernel_enabled or self.collect_reports
        # deferred: results and reports are made at the end of optimize().  Nothing on the host depends on the records of a
        # fixed count: they are read with the other levels' -- ONE synchronisation per call, not one per level
        return _LevelOutcome(canonical, packed, warp, grid, F[launches % 2] if keep else None, dec, n_exec,
                             records=records, deferred=True)

    def _optimize_level_graph(self, canonical, packed, warp):
        """launch-bound levels: K iterations (K even) are captured once per level shape as a HIP graph over persistent
        buffers and replayed; a replay costs one launch instead of K x (1..5).  Record slots 0..K-1 form a ring that the
        graph itself re-zeroes, slot K keeps the previous batch's last record for the first gate of the next batch, so
        iteration counts and results are exactly those of the eager path (tests demand equality)."""
        max_it = self.maximum_iteration_count
        key = self._graph_key(canonical)
        K = key[2]
        entry = self._graphs.get(key)
        if entry is None:
            grid = dev.make_grid(canonical.shape)
            lv = self._make_level(torch.empty_like(canonical), torch.empty_like(packed), torch.empty_like(warp), grid,
                                  grid, K + 1)
            side = torch.cuda.Stream(device=canonical.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up launch outside capture (first-use initialisation of the kernels)
                lv.warp.zero_()
                lv.canonical.zero_()
                lv.packed.zero_()
                self._enqueue(lv, 0, None, 0)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # thread_local: another optimizer working in another host thread on another stream (experiment/multipair.py:
            # pairs in flight) must not invalidate this capture; two captures at once are kept apart by the lock
            with _CAPTURE_LOCK:
                del _RETIRED_GRAPHS[:]  # graphs of engines that are gone die here, with no capture in progress
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    lv.records[K].copy_(lv.records[K - 1])
                    lv.records[:K].zero_()
                    for j in range(K):
                        # (a stop test that cannot fire: an iteration's maximum is left to the next one's first kernel,
                        # the batch's last keeps its own pass -- see _make_level)
                        self._enqueue(lv, j, K if j == 0 else j - 1, j % 2, defer_max=lv.defer_max and j + 1 < K,
                                      prev_deferred=lv.defer_max and j > 0)
            entry = self._graphs[key] = (lv, graph)
        lv, graph = entry
        lv.canonical.copy_(canonical)
        lv.packed.copy_(packed)
        lv.warp.copy_(warp)
        for t in lv.F + lv.S:
            t.zero_()
        lv.records.zero_()
        dev.set_record_max(lv.records, K - 1, HierarchicalEngine.OPEN_RECORD)
        log, done, n_exec, ended = [], 0, 0, False
        while done + K <= max_it and not ended:
            graph.replay()
            k_exec, ended = self._read_batch(lv.records[:K], log)  # host sync once per K iterations
            done, n_exec = done + K, n_exec + k_exec
        rest = max_it - done
        if not ended and rest > 0:
            # the remainder of a limit that is not a multiple of K (rest < K): eagerly on the captured level, its record
            # ring started afresh -- slot 0 the last record, iteration t in slot t + 1
            lv.records[0].copy_(lv.records[K - 1])
            lv.records[1:rest + 1].zero_()
            for t in range(rest):
                self._enqueue(lv, t + 1, t, (done + t) % 2)
            n_exec += self._read_batch(lv.records[1:rest + 1], log)[0]
        warp.copy_(lv.warp)
        # (the level's buffers are persistent: the caller's fields and a copy of the gradient, which the next call cannot alias)
        final = lv.F[n_exec % 2] if lv.F and n_exec else lv.report_g
        return _LevelOutcome(canonical, packed, warp, lv.grid, None if final is None else final.clone(),
                             self._merged(log), n_exec)


class _Level:
    """What the per-iteration drivers (eager, graph) enqueue a level's iterations from; _make_level makes it.  The fields
    (packed_global: the whole level's packed live field when a slab level runs on a replicated one), the launch grid and
    the level's SlabComm or None; the parameter block; the gradient buffers F ([] with neither Tikhonov term nor gradient
    kernel), the filter's scratch buffers S ([] without a kernel), report_g for the gradient when there is no F and
    reports are collected; the records and their launcher (dev.IterationLauncher); the filter plan (_filter_plan); the
    checked device pointers; the deferred maximum (_make_level): whether, and its kernel's parameters and open gates."""
    __slots__ = ("canonical", "packed", "packed_global", "warp", "grid", "comm", "params", "params_ref", "F", "S",
                 "report_g", "records", "launcher", "steps", "moves_warp", "p_packed", "p_canon", "p_warp", "p_F", "p_S",
                 "p_report", "defer_max", "prevmax", "prevmax_ref", "open_gates", "open_gate_refs")

    def __init__(self, **fields):
        for name in self.__slots__:  # every field, every time
            setattr(self, name, fields.pop(name))
        assert not fields, fields


@dataclass(eq=False)
class _LevelOutcome:
    """what a driver leaves of a level, and all that _finish_level looks at"""
    canonical: torch.Tensor
    packed: torch.Tensor
    warp: torch.Tensor
    grid: object
    gradient: object       # the last executed iteration's (filtered) gradient, or None
    decoded: object        # dev.decode_records of the level's records; None: still on the card, in `records`
    n_exec: object         # executed iterations; None until the records are read
    records: object = None
    packed_global: object = None
    comm: object = None    # the level's SlabComm (z-slab runs)
    deferred: bool = False  # results are made at the end of optimize() (blocked levels), not when the level ends
