"""The cumulative warp of a KillingFusion call, restated in numpy ("Cumulative warp").

Every iteration of the Slavcheva-style optimizer re-warps the live field by its own update u_k,
live_{k+1}(v) = live_k(v + u_k(v)) (slavcheva_optimizer2d.py:324-328), so the call's total displacement PSI with
live_0(v + PSI(v)) ~ canonical(v) is the composition
    PSI_0 = 0,   PSI_{k+1}(v) = u_k(v) + PSI_k(v + u_k(v)).
The rule, D = 2 and 3: after iteration k, with u the update the oracle holds (the post-snap one: warp_field_advanced has
zeroed it where the re-warped live value snapped to +-1), for every voxel and component c
    PSI'_c(v) = float32( u_c(v) + sample_linear(PSI_c, _grid_positions(u), oob = 0) )
with the oracle's own _grid_positions and sample_linear.  An iteration that does not run composes nothing; zero iterations
leave PSI = 0.  The plain sum of the updates is kept next to it, for comparison.  numpy only: importable without a GPU."""
import types

import numpy as np

from oracle import lsf_oracle as O

F32 = np.float32

# the KillingFusion configuration (DIRECT terms, Killing regulariser) with a fixed iteration count; oracle keywords
KILLING = dict(compute_method=O.DIRECT, level_set_term_enabled=True, sobolev_smoothing_enabled=False,
               data_term_method=O.BASIC, smoothing_term_method=O.KILLING, gradient_descent_rate=0.1, data_term_weight=1.0,
               smoothing_term_weight=0.2, isomorphic_enforcement_factor=0.1, level_set_term_weight=0.2,
               maximum_warp_length_lower_threshold=0.0, maximum_warp_length_upper_threshold=10000, max_iterations=30,
               min_iterations=30, sobolev_kernel=None)


def fixed(iterations, **changes):
    """KILLING with `iterations` fixed iterations and further keywords changed"""
    return dict(KILLING, max_iterations=iterations, min_iterations=iterations, **changes)


def compose(psi, update):
    """one step: PSI' = update + PSI(id + update), per component, out-of-array taps read 0"""
    pos = O._grid_positions(update)
    out = np.empty_like(psi)
    for c in range(psi.shape[-1]):
        sampled = O.sample_linear(np.ascontiguousarray(psi[..., c]), pos, F32(0.0))
        out[..., c] = (update[..., c] + sampled).astype(F32)
    return out


def run(canonical, live0, cfg):
    """the oracle's call with the composition behind every executed iteration: live (the final live field), warp (the last
    update), gradient, psi (composed), summed (the plain sum of the updates), iteration_count, log, update_maxima"""
    oracle = O.SlavchevaOracle(**cfg)
    d = live0.ndim
    acc = types.SimpleNamespace(psi=np.zeros(live0.shape + (d,), F32), summed=np.zeros(live0.shape + (d,), F32))

    def hook(it, live, warp, gradient, energies, max_warp, at):
        acc.psi = compose(acc.psi, warp)  # `warp` is the post-snap update: warp_field_advanced zeroed it in place
        acc.summed = (acc.summed + warp).astype(F32)

    oracle.iteration_hook = hook
    live = live0.copy()
    oracle.optimize(live, canonical)
    out = types.SimpleNamespace(live=live, warp=oracle.warp_field, gradient=oracle.gradient_field, psi=acc.psi,
                                summed=acc.summed, iteration_count=oracle.iteration_count, log=oracle.log)
    for a in (out.live, out.warp, out.psi, out.summed):
        a.setflags(write=False)
    return out


def pull_back(field, psi):
    """field o (id + psi): the D-linear resampling the optimizer re-warps with, out-of-array taps read 1"""
    return O.warp_field(field, np.ascontiguousarray(psi, dtype=F32))


def band(canonical, live):
    """the narrow-band union (tsdf_set_routines.py:19-52)"""
    return ~(O.is_truncated(live) & O.is_truncated(canonical))


def consistency(canonical, live0, result):
    """band means of |live_0 o (id + PSI) - live_K| for the composed PSI and for the summed updates, and of
    |live_0 - live_K|: how well each field explains what the call did to the live field"""
    at = band(canonical, live0)
    final = result.live.astype(np.float64)
    return tuple(float(np.abs(x.astype(np.float64) - final)[at].mean())
                 for x in (pull_back(live0, result.psi), pull_back(live0, result.summed), live0))


def ortho64():
    """BASELINE config 1's 64 x 64 input: the crop [30:94, 30:94] of the reference generator's 128 x 128 pair;
    (canonical, live)"""
    live, canonical = O.orthographic_pair(field_size=128)
    return canonical[30:94, 30:94].copy(), live[30:94, 30:94].copy()


def smooth_pair(shape, amplitude=0.6, shift=(0.75, -0.5, 1.0)):
    """(canonical, live) with EVERY voxel inside the band: amplitude * tanh of a scaled distance to an ellipsoid, and the
    same body shifted -- no value reaches +-1"""
    shape = tuple(int(s) for s in shape)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")[::-1]  # (x, y[, z])
    extents = shape[::-1]

    def field(offset):
        sq = 0.0
        for q, n, o in zip(grids, extents, offset):
            sq = sq + ((q - ((n - 1) / 2.0 + 0.3 + o)) / (0.3 * n)) ** 2
        return (amplitude * np.tanh((np.sqrt(sq) - 1.0) * 2.0)).astype(F32)

    canonical, live = field((0.0,) * len(shape)), field(tuple(shift)[:len(shape)])
    assert np.abs(canonical).max() < 1 and np.abs(live).max() < 1
    return canonical, live


def deforming_chain(cfg):
    """tests/deforming_scene.py's chain with the KillingFusion oracle: frame 0 fused, the live volume of frame 1, the
    oracle's call from it to the model with PSI composed, frame 1 fused through PSI: (model tsdf and weight after frame 0,
    psi, tsdf, weight and record after frame 1, tsdf after a rigid frame 1, the call's result)"""
    import deforming_scene as D
    import fusion_weighted_restatement as FW
    import rigid3d_restatement as R3
    import warped_fusion_restatement as WR
    d0, d1 = D.frames()
    shape = (D.N,) * 3
    gen = (D.K, 1.0, D.OFFSET, D.TWIST, D.BAND, D.VOXEL)
    t0, W0, _ = FW.fuse_depth_weighted(np.ones(shape, F32), np.zeros(shape, F32), d0, *gen)
    live = R3.live_volume(d1, D.K, 1.0, shape, D.OFFSET, D.TWIST, D.BAND, D.VOXEL)
    result = run(t0, live, cfg)
    psi = result.psi
    assert psi.dtype == F32 and psi.shape == shape + (3,) and np.isfinite(psi).all()
    t1, W1, _, rec = WR.fuse_depth_warped(t0, W0, d1, D.K, 1.0, D.OFFSET, D.TWIST, psi, D.BAND, D.VOXEL)
    rigid = FW.fuse_depth_weighted(t0, W0, d1, *gen)[0]
    return t0, W0, psi, t1, W1, rec, rigid, result
