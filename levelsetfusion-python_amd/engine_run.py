"""Whole optimize() calls enqueued by the LIBRARY (csrc/lsf_slavcheva_run.hip): the loop of
slavcheva_optimizer2d.py:354-388 without a Python iteration -- two foreign calls that run without the interpreter lock.
_RunCall is what the whole-volume call (here) and the z-slab call (engine_slab.py) set up and leave behind alike."""
import ctypes

import numpy as np
import torch

from . import _lib, device as dev
from .engine_common import _Fast, _Lazy
from .engine_outcome import _RunLog, _RunOutcome, recompute_gradient


class _SparseStateExceeded(Exception):
    """a call whose ping-pong states were initialised near the band only (dev.StatePrepare(sparse_reach=...)) met a warp
    update that can read beyond that; nothing of the caller's has been modified (SlavchevaEngine.optimize repeats the
    call on fully initialised states and keeps doing so for this optimizer)"""


class _RunCall:
    """One library-enqueued call: what lsf_state_run_* (a whole volume) and lsf_slab_run_* (a z-slab rank) are handed and
    leave behind alike, made in the order both need it -- the target, the states, the prepare scratch, the totals and the
    lsf_state_run base block in front of the begin call; behind it the records, their used words and the result arrays;
    and, BEFORE the blocking finish call, everything about the call's aftermath that does not depend on its results
    (behind it the card idles until the next call's first launch: tools/host_tail.py)."""

    def __init__(self, engine, live, canonical, grid, finalize, sparse, base, totals_name, n_totals, restore=False):
        live_out = finalize[0]
        self.engine, self.canonical, self.grid = engine, canonical, grid
        device = self.device = live.device
        n = self.n = dev.n_voxels(grid)
        whole = self.whole = dev.full_range(grid)  # (a slab: the local array, owned slices + halos; z_global_offset stays)
        engine.last_call.sparse_states = sparse
        engine.last_call.library_run = True
        usable = (live_out is not None and live_out.is_cuda and live_out.dtype == torch.float32
                  and live_out.is_contiguous() and tuple(live_out.shape) == tuple(live.shape))
        target = self.target = live_out if usable else torch.empty_like(live)
        if target is not live:
            target.copy_(live)  # the finalize pass writes listed voxels only
        elif usable and restore:
            # the pass writes the caller's tensor before every rank's records have said whether the call stands: what it
            # overwrites is kept (optimize() puts it back before a wider re-run)
            engine._slab_restore = (live_out, live_out.clone())
        states = self.states = [torch.empty(tuple(live.shape) + (4,), dtype=torch.float32, device=device)
                                for _ in range(2)]
        self.scratch = torch.empty(int(_lib.lib.lsf_state_prepare_scratch_elements(ctypes.byref(whole))),
                                   dtype=torch.int32, device=device)
        self.totals = torch.empty(n_totals, dtype=torch.int64, device=device)
        self.totals_host = dev.pinned_scratch(totals_name, n_totals, torch.int64)
        base.live, base.canonical = dev._ptr(live, n, "live"), dev._ptr(canonical, n, "canonical")
        base.state[0], base.state[1] = states[0].data_ptr(), states[1].data_ptr()
        base.prepare_scratch, base.totals_device, base.totals_host = self.scratch.data_ptr(), self.totals.data_ptr(), \
            self.totals_host.data_ptr()
        base.grid = whole
        base.sparse_reach = engine.sparse_reach if sparse else 0
        base.second_state_late = int(not sparse and n <= dev.StatePrepare.SPLIT_MAX_VOXELS)

    def results(self, lists, n_interior, n_boundary, iterations, device_words, host_name, host_words):
        """the records, their used words on the device and on the host and the arrays the finish call decodes them into;
        then what does not depend on the call's results: the two band lists cut from `lists` (sized from the totals the
        begin call waited for), what the call leaves in engine._fast, its outcome"""
        self.lists = lists
        records = self.records = dev.new_records(iterations, self.device)
        self.words = torch.empty(device_words, dtype=torch.int64, device=self.device)
        self.words_host = dev.pinned_scratch(host_name, host_words, torch.int64)
        self.max_value, self.argmax = np.empty(iterations, np.float32), np.empty(iterations, np.int64)
        self.energies, self.executed = np.empty((iterations, 3), np.float64), np.empty(iterations, np.bool_)
        self.result = _lib.StateRunResult(self.max_value.ctypes.data, self.argmax.ctypes.data, self.energies.ctypes.data,
                                          self.executed.ctypes.data)
        bands = self.bands = []
        if n_interior:
            bands.append(dev.BandList(lists[:n_interior], n_interior, _lib.BAND_INTERIOR))
        if n_boundary or not bands:
            bands.append(dev.BandList(lists[n_interior:] if n_boundary else lists[:1], n_boundary, _lib.BAND_BOUNDARY))
        fast = self.fast = _Fast(self.grid, records, bands=bands)
        self.outcome = _RunOutcome(self.grid, self.canonical, None, self.target, bands, None)
        self.weights = tuple(self.engine.weights)
        return fast

    def leave(self, gradient_grid, gradient=None, n_exec=None):
        """the call stands: the engine's count, log and gradient source, the outcome's final state"""
        e = self.engine
        if n_exec is None:
            n_exec = len(self.executed) if self.executed.all() else int(self.executed.sum())
        e._fast = self.fast
        e.iteration_count = n_exec
        e.log = _RunLog(self.max_value[:n_exec], self.argmax[:n_exec], self.energies[:n_exec], self.weights)
        if gradient is None:
            # gradient_field() recomputes the last iteration's gradient on demand from its INPUT state, at the listed voxels
            params, state_in, canonical, bands = e.params, self.states[(n_exec - 1) % 2], self.canonical, self.bands
            gradient = _Lazy(lambda: recompute_gradient(params, state_in, canonical, gradient_grid, bands))
        e._gradient_state = gradient
        self.outcome.state = self.states[n_exec % 2]
        return self.outcome


class RunMixin:
    """SlavchevaEngine's library-enqueued calls on whole volumes"""

    def _optimize_run(self, live, canonical, grid, finalize, sobolev=False):
        """_optimize for the case the library enqueues in one piece (lsf_state_run_begin / _finish): prepare pass, (sparse)
        states, band lists, all iterations -- a fixed count, or the reference's threshold-terminated loop in batches of
        check_interval gated launches --, the listed finalize pass and the read-backs: the same launches in the same order
        as the general path makes one by one, hence the same results, in two foreign calls that run without the interpreter
        lock.  sobolev: the SobolevFusion iteration on whole 3-D volumes of whole boxes (lsf_sobolev_run_finish: gradient + x
        pass over the list of all band voxels, then y pass, z pass, update and re-warp box by box)."""
        live_out, lower_threshold, statistics = finalize
        # the number of records; with min < max the stop test can fire (the reference's default: slavcheva_optimizer2d.py:
        # 360-362) and the library enqueues check_interval gated iterations at a time, reading the records in between
        iterations = max(self.min_iterations, self.max_iterations)
        loop = None
        if self.min_iterations < iterations:
            loop = _lib.RunLoop(self.min_iterations, self.max_iterations, self.lo, self.hi, self.check_interval, 0)
        run = _lib.StateRun()
        c = _RunCall(self, live, canonical, grid, finalize, self._sparse_states(grid), run, "run totals", 5)
        device, n, whole = c.device, c.n, c.whole
        count_boxes = sobolev or (dev.boxes_ok(whole) and (self.box_walk is True or
                                                           (self.box_walk is None and n >= self.box_walk_min_voxels)))
        run.box_all = int(sobolev)
        box_scratch = None
        if count_boxes:
            box_scratch = torch.empty(int(_lib.lib.lsf_band_boxes_scratch_elements(ctypes.byref(whole))),
                                      dtype=torch.int32, device=device)
            run.box_scratch = box_scratch.data_ptr()
        stream = dev.stream_ptr()
        _lib.check(_lib.lib.lsf_state_run_begin(ctypes.byref(run), stream), "lsf_state_run_begin")
        # (the card is writing the states now; the lists are sized from the totals the call waited for)
        n_interior, n_boundary, opposite, first_opposite, n_boxes = c.totals_host.tolist()
        lists = torch.empty(max(n_interior + n_boundary, 1), dtype=torch.int32, device=device)
        boxes = box_canonical = None
        if sobolev:
            boxes = torch.empty((max(n_boxes, 1), 2), dtype=torch.int64, device=device)
            list_all = torch.empty(max(n_interior + n_boundary, 1), dtype=torch.int32, device=device) \
                if n_interior and n_boundary else None
            g4 = self._sobolev_gradient_buffers(live, whole, lists, n_interior + n_boundary)
            taps = np.ascontiguousarray(np.asarray(self.sobolev_kernel, dtype=np.float64))
            self.last_call.sobolev_boxes = True
        elif n_boxes and (self.box_walk is True or 32 * n_interior > self.box_walk_min_band_bytes):
            boxes = torch.empty((n_boxes, 2), dtype=torch.int64, device=device)
            box_canonical = torch.empty(n_boxes * dev.BOX_EDGE ** 3, dtype=torch.float32, device=device)
        self.last_call.box_walk = boxes is not None and not sobolev
        record_rows = None
        if loop is None and not sobolev and self.record_rows:
            # a fixed count reads no record before its end: one row per wave of every launch, combined once per call
            n_launches = int(n_interior > 0) + int(n_boundary > 0 or n_interior == 0)
            record_rows = torch.empty(int(_lib.lib.lsf_state_run_rows_elements(ctypes.byref(whole), iterations, n_launches)),
                                      dtype=torch.int64, device=device)
        n_words = iterations * _lib.RECORD_SLOTS * dev.USED_SLOT_WORDS
        # (the records' used words, then the statistics)
        f = c.results(lists, n_interior, n_boundary, iterations, n_words + 16, "run records", n_words + 16)
        records, words, words_host, result = c.records, c.words, c.words_host, c.result
        stats = stats_scratch = None
        if statistics:
            stats = torch.empty(16, dtype=torch.float64, device=device)
            stats_scratch = torch.empty(2 * int(_lib.lib.lsf_state_finalize_scratch_elements(ctypes.byref(whole))),
                                        dtype=torch.float64, device=device)
        none = ctypes.c_void_p(0)
        p_lists = lists.data_ptr()
        f.boxes = (boxes, box_canonical)
        if sobolev:
            f.keep = (g4, list_all, taps)
            self._sobolev_band = f  # what bench.py prices this path over
            _lib.check(_lib.lib.lsf_sobolev_run_finish(
                ctypes.byref(run), ctypes.byref(self.params), taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                int(taps.size), ctypes.c_void_p(p_lists), ctypes.c_void_p(p_lists + 4 * n_interior),
                ctypes.c_void_p(list_all.data_ptr() if list_all is not None else 0), ctypes.c_void_p(boxes.data_ptr()),
                ctypes.c_void_p(g4[0].data_ptr()), ctypes.c_void_p(g4[1].data_ptr()), ctypes.c_void_p(records.data_ptr()),
                iterations, ctypes.byref(loop) if loop is not None else None, dev._ptr(c.target, n, "live_out"),
                float(lower_threshold), ctypes.c_void_p(stats.data_ptr()) if statistics else none,
                ctypes.c_void_p(stats_scratch.data_ptr()) if statistics else none, ctypes.c_void_p(words.data_ptr()),
                ctypes.c_void_p(words_host.data_ptr()), ctypes.byref(result), stream), "lsf_sobolev_run_finish")
        else:
            self._run_finish(run, p_lists, n_interior, boxes, box_canonical, records, iterations, loop, c.target, n,
                             lower_threshold, stats, stats_scratch, statistics, words, words_host, result, stream, record_rows)
        if result.reach_exceeded:
            raise _SparseStateExceeded()  # the pass has left the caller's array alone (its guard); optimize() repeats
        # SobolevFusion: the filtered gradient of the last executed iteration (float4, made planar when read)
        outcome = c.leave(grid, _Lazy(lambda: g4[1][..., :grid.dims].movedim(-1, 0).contiguous()) if sobolev else None)
        if statistics:
            outcome._raw = words_host[n_words:].numpy().view(np.float64).copy()
        return outcome

    def _sobolev_gradient_buffers(self, live, whole, lists, n_listed):
        """the two float4 gradient buffers of a library-enqueued SobolevFusion call, all zero: the previous call's buffers with
        zeros written back at ITS listed voxels (every other voxel was never written: lsf_zero_listed4, 2 x 26 MB at 256^3) or,
        for another shape, fresh zero fills (2 x 268 MB).  The optimizer keeps them between calls (the reference allocates its
        gradient per call, slavcheva_optimizer2d.py:343-346)."""
        key = (tuple(live.shape), live.device)
        cache = self._g4_cache
        if cache is not None and cache[0] == key:
            _, g4, old_lists, old_n = cache
            for t, bricks in ((g4[0], 1), (g4[1], 0)):
                _lib.check(_lib.lib.lsf_zero_listed4(ctypes.c_void_p(t.data_ptr()), ctypes.byref(whole),
                                                     ctypes.c_void_p(old_lists.data_ptr()), old_n, bricks, dev.stream_ptr()),
                           "lsf_zero_listed4")
        else:
            self._g4_cache = None  # (let go of another shape's buffers first)
            g4 = [torch.zeros(tuple(live.shape) + (4,), dtype=torch.float32, device=live.device) for _ in range(2)]
        # recorded BEFORE the call runs: whatever happens in it, these are the voxels it may have written
        self._g4_cache = (key, g4, lists, int(n_listed))
        return g4

    def _run_finish(self, run, p_lists, n_interior, boxes, box_canonical, records, iterations, loop, target, n,
                    lower_threshold, stats, stats_scratch, statistics, words, words_host, result, stream, record_rows=None):
        none = ctypes.c_void_p(0)
        rows_taken = ctypes.c_int32(0)
        _lib.check(_lib.lib.lsf_state_run_finish_rows(
            ctypes.byref(run), ctypes.byref(self.params), ctypes.c_void_p(p_lists),
            ctypes.c_void_p(p_lists + 4 * n_interior), ctypes.c_void_p(boxes.data_ptr() if boxes is not None else 0),
            ctypes.c_void_p(box_canonical.data_ptr() if boxes is not None else 0),
            ctypes.c_void_p(records.data_ptr()), iterations, ctypes.byref(loop) if loop is not None else None,
            dev._ptr(target, n, "live_out"), float(lower_threshold),
            ctypes.c_void_p(stats.data_ptr()) if statistics else none,
            ctypes.c_void_p(stats_scratch.data_ptr()) if statistics else none, ctypes.c_void_p(words.data_ptr()),
            ctypes.c_void_p(words_host.data_ptr()), ctypes.byref(result),
            ctypes.c_void_p(record_rows.data_ptr()) if record_rows is not None else none,
            record_rows.numel() if record_rows is not None else 0, ctypes.byref(rows_taken), stream),
            "lsf_state_run_finish_rows")
        self.last_call.record_rows = bool(rows_taken.value)

