"""The canonical / live pyramids of a hierarchical call, whole volumes and z-slabs
(nonrigid_opt/hierarchical/hierarchical_optimizer2d.py:126-131, pyramid.py)."""
import torch

from . import device as dev
from .engine_common import pyramid_level_count
from .slab import SlabComm, SlabLayout


def build_pyramids(canonical, live, maximum_chunk_size, linear_resampling, comm=None):
    """canonical / live pyramids, coarsest first; live is packed with its full-resolution np.gradient
    BEFORE restriction (gradients are averaged, not recomputed: hierarchical_optimizer2d.py:126-131).
    comm: the finest level's SlabComm of a z-slab run.  Returns (canonical levels, packed levels, per-level SlabComm
    or None)."""
    if comm is None or not comm.active:
        n_levels = pyramid_level_count(live.shape, maximum_chunk_size)
        canon_levels = [canonical]
        packed_levels = [dev.pack_live_gradient(live)]
        restrict = dev.downsample2x_linear if linear_resampling else dev.restrict_mean
        for _ in range(1, n_levels):
            canon_levels.append(restrict(canon_levels[-1], 1))
            packed_levels.append(restrict(packed_levels[-1], 4))
        return canon_levels[::-1], packed_levels[::-1], [None] * n_levels
    # z-slab: every level keeps `halo` neighbour slices; a level's owned slices are the restriction of the finer
    # level's owned slices (slab boundaries are multiples of 2^levels), its halos come from one exchange per level
    L0 = comm.layout
    if live.dim() != 3 or live.shape[0] != L0.nz_local:
        raise ValueError("slab runs need 3-D local fields with %d slices, got %r" % (L0.nz_local, tuple(live.shape)))
    global_shape = (L0.nz_global,) + tuple(live.shape[1:])
    n_levels = pyramid_level_count(global_shape, maximum_chunk_size)
    per = L0.z1 - L0.z0
    if per % (1 << (n_levels - 1)) != 0 or (per >> (n_levels - 1)) < max(L0.halo, 1):
        raise ValueError("a slab of %d slices cannot carry %d pyramid levels with a %d-slice halo"
                         % (per, n_levels, L0.halo))
    comms = [comm]
    packed = dev.pack_live_gradient(live)
    # the outermost halo slice got a one-sided z difference: refresh the halos from their owners
    comms[0].exchange_halos([packed.view(packed.shape[0], packed.shape[1], -1)])
    canon_levels, packed_levels = [canonical], [packed]
    for k in range(1, n_levels):
        fine_comm = comms[-1]
        Lf = fine_comm.layout
        Lc = SlabLayout(Lf.nz_global // 2, Lf.rank, Lf.world, Lf.halo)
        cc = SlabComm(Lc, fine_comm.group)
        own_f = Lf.owned_local()
        if linear_resampling:
            c_own = _restrict_linear_owned(canon_levels[-1], Lf, 1)
            p_own = _restrict_linear_owned(packed_levels[-1], Lf, 4)
        else:
            c_own = dev.restrict_mean(canon_levels[-1][own_f].contiguous(), 1)
            p_own = dev.restrict_mean(packed_levels[-1][own_f].contiguous(), 4)
        c_loc = torch.zeros((Lc.nz_local,) + tuple(c_own.shape[1:]), dtype=torch.float32, device=live.device)
        p_loc = torch.zeros((Lc.nz_local,) + tuple(p_own.shape[1:]), dtype=torch.float32, device=live.device)
        c_loc[Lc.owned_local()] = c_own
        p_loc[Lc.owned_local()] = p_own
        cc.exchange_halos([c_loc])
        cc.exchange_halos([p_loc.view(p_loc.shape[0], p_loc.shape[1], -1)])
        canon_levels.append(c_loc)
        packed_levels.append(p_loc)
        comms.append(cc)
    return canon_levels[::-1], packed_levels[::-1], comms[::-1]


def _restrict_linear_owned(fine, layout, channels):
    """LINEAR restriction (4x4x4 windows, math_utils/resampling.py:90-109) of a slab's owned slices: the window of a
    coarse slice reaches one fine slice past the owned range -- the neighbour's slice from the halo, or the edge
    slice again where the volume ends (the kernel's clamp).  Two slices are put on either side so that the window
    origin stays even; the outer one and the two extra coarse slices it produces are never looked at."""
    own = layout.owned_local()
    below = fine[own.start - 1:own.start] if layout.halo_lo >= 1 else fine[own.start:own.start + 1]
    above = fine[own.stop:own.stop + 1] if layout.halo_hi >= 1 else fine[own.stop - 1:own.stop]
    padded = torch.cat([below, below, fine[own], above, above], 0).contiguous()
    return dev.downsample2x_linear(padded, channels)[1:-1].contiguous()
