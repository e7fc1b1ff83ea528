"""What a SlavchevaEngine.optimize() call leaves behind: the final fields on the device (handed out on demand), the
per-iteration log, how gradient_field() recomputes its field (the engine keeps it as an engine_common._Lazy: made when
first read, then kept, and what it was made from let go of), and what the launch-by-launch iterations on
the float4 ping-pong states share."""
import torch

from . import _lib, device as dev


def unpack_state(state, grid):
    """a float4 state as fresh planar (live, warp) tensors"""
    live = torch.empty(tuple(state.shape[:-1]), dtype=torch.float32, device=state.device)
    warp = torch.empty((grid.dims,) + tuple(live.shape), dtype=torch.float32, device=state.device)
    dev.state_unpack(state, grid, live, warp, None)
    return live, warp


def without_energies(params):
    """a copy of the parameter block for launches whose records nobody reads"""
    params = _lib.SlavchevaParams.from_buffer_copy(params)
    params.energy_mode = _lib.ENERGY_NONE
    return params


def recompute_gradient(params, state_in, canonical, grid, bands=None, complete=None):
    """The fused kernel does not store the gradient (12 B/voxel/iteration saved); it is recomputed here from the inputs
    of the last iteration, which the ping-pong buffers still hold, by the unfused kernels -- same code path, same bits.
    bands: the unfused kernels at the voxels of the call's band lists (the gradient is zero everywhere else): of the
    input state only the listed voxels' neighbourhoods and re-warp cells are read, so a state that was initialised
    near the band only (lsf_state_pack_needed) serves as it stands, and nothing of the caller's is touched.
    complete = (dev.StatePrepare, live): the state was initialised near the band only and is read whole: complete it from
    the call's live array, which still holds the input wherever no list entry points (the finalize pass writes listed
    voxels only)."""
    if complete is not None:
        complete[0].complete(state_in, complete[1])
    live_in, warp_in = unpack_state(state_in, grid)
    g = torch.empty_like(warp_in) if bands is None else torch.zeros_like(warp_in)
    scratch_records = dev.new_records(1, live_in.device)
    params = without_energies(params)
    warp_out, live_scratch = torch.empty_like(warp_in), torch.empty_like(live_in)
    bands = [None] if bands is None else [band for band in bands if band.count]
    for band in bands:
        dev.slavcheva_gradient(live_in, canonical, warp_in, g, grid, params, None, scratch_records, 0, band)
    for band in bands:
        dev.slavcheva_update_rewarp(live_in, canonical, g, warp_out, live_scratch, grid, params, None, scratch_records, 0,
                                    band)
    return g


class SlavchevaOutcome:
    """final fields of one SlavchevaEngine.optimize() call, left on the device in the layout the iteration kernels use
    (the float4 state of the fused path, or planar live / warp of the Sobolev path) and handed out on demand"""

    def __init__(self, grid, canonical, state=None, live=None, warp_planar=None, listed=None, sparse=None,
                 warp_zeroed=None):
        self.grid, self.canonical, self.state = grid, canonical, state
        self._live, self._warp_planar = live, warp_planar
        # (input live field, band lists, state_prepare's unlisted counts): finalize then visits the band voxels only
        self._listed = listed
        # dev.StatePrepare whose states were initialised near the band only: readers of the WHOLE state complete it first
        self._sparse = sparse
        self._guard = None
        self._warp_zeroed = warp_zeroed  # a zero-filled API-layout warp tensor made while the card was idle (or None)
        self._early = None  # enqueue_finalize(): (its arguments, target, warp, raw statistics on their way to the host)

    def guard(self, records, count, limit):
        """a sparse run: the listed finalize pass leaves the caller's fields alone when one of records[0..count) holds a
        maximum update of `limit` voxels or more (it looks at the records itself, on the device)"""
        self._guard = (records, int(count), float(limit))

    def _whole_state(self):
        if self._sparse is not None:
            self._sparse.complete(self.state, self._listed[0])
            self._sparse = None
        return self.state

    def _shape(self):
        g = self.grid
        return (g.nz, g.ny, g.nx) if g.dims == 3 else (g.ny, g.nx)

    def _device(self):
        return (self.state if self.state is not None else self._live).device

    def live(self):
        if self._live is None:
            self._live = torch.empty(self._shape(), dtype=torch.float32, device=self._device())
            dev.state_unpack(self._whole_state(), self.grid, self._live, None, None)
        return self._live

    def warp_planar(self):
        if self._warp_planar is None:
            self._warp_planar = torch.empty((self.grid.dims,) + self._shape(), dtype=torch.float32,
                                            device=self._device())
            dev.state_unpack(self._whole_state(), self.grid, None, self._warp_planar, None)
        return self._warp_planar

    def finalize(self, live_out=None, lower_threshold=0.0, statistics=False):
        """ONE pass for the end of optimize(): writes the final live field into `live_out` (a contiguous float32
        device tensor, or None for a new one), builds the interleaved warp [z,]y,x,c and -- with `statistics` -- the raw
        convergence statistics (float64 [16] on the HOST: warp [0:8], |canonical - live| [8:16]).
        Returns (live, warp_interleaved, raw statistics or None)."""
        early = self._early
        if early is not None and early[0][0] is live_out and \
                early[0][1:] == (float(lower_threshold), bool(statistics)):
            # already enqueued by optimize() behind the last iteration (fixed iteration counts): nothing left to launch
            _, target, warp, raw = early
            self._early = None
            if live_out is not None and target is not live_out:
                live_out.copy_(target)
            if raw is not None:
                host, done = raw
                done.synchronize()
                raw = host.numpy().copy()  # the pinned buffer is reused by the next call
            return target, warp, raw
        return self._finalize_now(live_out, lower_threshold, statistics, to_host=True)

    def enqueue_finalize(self, live_out, lower_threshold, statistics):
        """launch the finalize pass now (no host synchronisation); finalize() with the same arguments collects it"""
        target, warp, raw = self._finalize_now(live_out, lower_threshold, statistics, to_host=False)
        if raw is not None:  # on its way to the host behind the pass: the caller's next synchronising read covers it
            host = dev.pinned_scratch("finalize statistics", raw.numel(), raw.dtype)
            host.copy_(raw, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            raw = (host, done)
        self._early = ((live_out, float(lower_threshold), bool(statistics)), target, warp, raw)

    def _finalize_now(self, live_out, lower_threshold, statistics, to_host):
        g = self.grid
        full = dev.full_range(g)
        if live_out is None or not (live_out.is_cuda and live_out.dtype == torch.float32 and live_out.is_contiguous()):
            target = torch.empty(self._shape(), dtype=torch.float32, device=self._device())
        else:
            target = live_out
        if self.state is not None and self._listed is not None and not (statistics and self._listed[2] is None):
            # outside the band lists nothing ever moves: the input live field and a zero warp are already final there
            live0, bands, unlisted = self._listed
            unlisted = unlisted or (0, -1)
            if target is not live0:
                target.copy_(live0)
            warp, self._warp_zeroed = self._warp_zeroed, None
            if warp is None:
                warp = torch.zeros(self._shape() + (g.dims,), dtype=torch.float32, device=self._device())
            raw = dev.state_finalize_listed(self.state, self.canonical, full, bands, unlisted, target, warp,
                                            lower_threshold, statistics, guard=self._guard)
            self._live = target
        elif self.state is not None:
            warp = torch.empty(self._shape() + (g.dims,), dtype=torch.float32, device=self._device())
            raw = dev.state_finalize(self._whole_state(), self.canonical, full, target, None, warp, lower_threshold,
                                     statistics)
            self._live = target
        else:
            # planar final fields (SobolevFusion path): one pass as well (lsf_planar_finalize)
            warp = torch.empty(self._shape() + (g.dims,), dtype=torch.float32, device=self._device())
            raw = dev.planar_finalize(self._live, self._warp_planar, self.canonical, full,
                                      None if target is self._live else target, warp, lower_threshold, statistics)
        if not to_host:
            return target, warp, raw
        if live_out is not None and target is not live_out:
            live_out.copy_(target)
        return target, warp, (raw.cpu().numpy() if raw is not None else None)


class _RunLog(dict):
    """the per-iteration log of a call as the lists the callers read -- max_warps, max_warp_indices, data_energies,
    smoothing_energies, level_set_energies --, converted from the decoded records when a key is first read: the lists of a
    50-iteration call cost ~10 us of host time behind the call's last synchronisation, where the card waits for the next
    call's first launch"""

    def __init__(self, max_value, argmax, energies, weights):
        super().__init__()
        self._pending = {"max_warps": lambda: max_value.tolist(), "max_warp_indices": lambda: argmax.tolist(),
                         "data_energies": lambda: (weights[0] * energies[:, 0]).tolist(),
                         "smoothing_energies": lambda: (weights[1] * energies[:, 1]).tolist(),
                         "level_set_energies": lambda: (weights[2] * energies[:, 2]).tolist()}

    def __missing__(self, key):
        value = self[key] = self._pending.pop(key)()
        return value

    def _all(self):
        for key in list(self._pending):
            self[key]
        return self

    def keys(self):
        return dict.keys(self._all())

    def items(self):
        return dict.items(self._all())

    def values(self):
        return dict.values(self._all())

    def __iter__(self):
        return dict.__iter__(self._all())

    def __len__(self):
        return dict.__len__(self._all())

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._pending

    def __eq__(self, other):
        return dict.__eq__(self._all(), other._all() if isinstance(other, _RunLog) else other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None


class _RunOutcome(SlavchevaOutcome):
    """the final fields of a call the LIBRARY enqueued in one piece (SlavchevaEngine._optimize_run): the live field is
    already in the caller's array and the statistics are on the host; the dense API-layout warp is only built when somebody
    asks for it (the reference's optimize() does not hand its warp field out at all, slavcheva_optimizer2d.py:332-408) --
    from the final state's LISTED voxels, so that states initialised near the band only need no completion and nothing here
    depends on the caller's tensor staying as the call left it"""

    def __init__(self, grid, canonical, state, target, bands, raw):
        super().__init__(grid, canonical, state=state)
        self._live, self._bands, self._raw, self._warp = target, bands, raw, None

    def live(self):
        return self._live

    def warp_interleaved(self):
        if self._warp is None:
            warp = torch.zeros(self._shape() + (self.grid.dims,), dtype=torch.float32, device=self._device())
            dev.state_finalize_listed(self.state, self.canonical, dev.full_range(self.grid), self._bands, (0, -1), None,
                                      warp, 0.0, False)
            self._warp = warp
        return self._warp

    def warp_planar(self):
        if self._warp_planar is None:
            self._warp_planar = dev.deinterleave(self.warp_interleaved(), self.grid.dims)
        return self._warp_planar

    def finalize(self, live_out=None, lower_threshold=0.0, statistics=False):
        """(live, a callable that builds the interleaved warp, raw statistics): everything was produced by the call"""
        if live_out is not None and live_out is not self._live:
            live_out.copy_(self._live)
        return self._live, self.warp_interleaved, (self._raw if statistics else None)


class _StateIteration:
    """what the launch-by-launch iterations on the float4 ping-pong states share (the fused kernel: engine_slavcheva.py's
    _FusedIteration, SobolevFusion on lists / boxes: engine_sobolev.py's _SobolevStatePlan): iteration i reads
    states[i % 2] and writes the other.  listed, sparse, warp_zeroed: SlavchevaOutcome's; live_at_entry: a copy of what an
    early finalize pass of a slab call overwrites."""

    restore = None  # (the caller's tensor an early finalize pass has written, its contents before), slab calls

    def hold(self, states, canonical, grid, records, listed=None, sparse=None, warp_zeroed=None, live_at_entry=None):
        self.states, self.canonical, self.grid, self.records = states, canonical, grid, records
        self._outcome_args = dict(listed=listed, sparse=sparse, warp_zeroed=warp_zeroed)
        self._live_at_entry, self._early = live_at_entry, None

    def inputs(self, i):
        """planar (live, warp) iteration i started from"""
        return unpack_state(self.states[i % 2], dev.full_range(self.grid))

    def finalize_early(self, finalize, records, limit, sparse_reach):
        """every launch runs ungated, so the final state is states[limit % 2]: finalize before looking.  A slab run
        may still have to be discarded (see optimize()), and the pass writes the caller's tensor: optimize() puts
        the copy taken at entry back before it runs the call again"""
        early = self._early = SlavchevaOutcome(self.grid, self.canonical, state=self.states[limit % 2],
                                               **self._outcome_args)
        if self._outcome_args["sparse"] is not None:
            # the pass must not touch the caller's fields when an update outran the initialised region
            early.guard(records, limit, float(sparse_reach))
        if self._live_at_entry is not None:
            self.restore = (finalize[0], self._live_at_entry)
        early.enqueue_finalize(*finalize)

    def outcome(self, n_exec, limit):
        if self._early is not None and n_exec == limit:
            return self._early
        return SlavchevaOutcome(self.grid, self.canonical, state=self.states[n_exec % 2], **self._outcome_args)
