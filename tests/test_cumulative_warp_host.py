"""CPU checks of the cumulative warp ("Cumulative warp"): the numpy restatement
(tests/cumulative_warp_restatement.py) on its degenerate cases, what composing buys over summing the updates on the
sphere pairs, the restated chain on tests/deforming_scene.py with the KillingFusion oracle, what
tests/test_gpu_cumulative_warp.py assumes about its inputs, the new symbol of the built library and its own refusals with
no GPU present, the constructor's refusals, and the combinations SequenceFusion3d accepts."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cumulative_warp_restatement as CW
import deforming_scene as D
import fusion_scene as S
import ragged_scene
from oracle import lsf_oracle as O

F32 = np.float32


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _sphere(d):
    canonical, live = O.sphere_pair(32 if d == 3 else 64, d=d)
    for a in (canonical, live):
        a.setflags(write=False)
    return canonical, live


# --------------------------------------------------------------------------------------------------- degenerate cases
def test_zero_iterations_leave_zeros():
    canonical, live = _sphere(3)
    result = CW.run(canonical, live, dict(CW.KILLING, min_iterations=0, max_iterations=5))
    assert result.iteration_count == 0 and result.psi.shape == live.shape + (3,)
    assert _bits_equal(result.psi, np.zeros_like(result.psi)) and _bits_equal(result.live, live)


@pytest.mark.parametrize("d", [2, 3])
def test_one_iteration_is_the_post_snap_update(d):
    """PSI_1 = u_0 + 0 in float32: the oracle's warp bit for bit, except that -0.0 + 0.0 is +0.0 (the update is
    (-0.0) * rate = -0.0 wherever the gradient is zero, outside the band for one), so the bits are those of warp + 0"""
    canonical, live = _sphere(d)
    result = CW.run(canonical, live, CW.fixed(1))
    assert result.iteration_count == 1
    assert np.array_equal(result.psi, result.warp) and _bits_equal(result.psi, result.warp + F32(0.0))
    assert np.count_nonzero(result.psi) > 100 and not np.signbit(result.psi[result.psi == 0]).any()
    assert _bits_equal(result.summed, result.psi)


def test_a_voxel_that_snapped_contributes_no_update():
    """where iteration k's re-warped live value snapped to +-1 the state holds u = 0 (field_warping.py:138-141): the
    gather sits on the voxel itself with ratio 0, so PSI_{k+1} = PSI_k there, bit for bit.  tests/ragged_scene.py's `odd`
    moves 3.7 to 5 voxels per iteration: values from inside the band reach +-1 (128, 117 and 43 voxels)"""
    canonical, live0 = ragged_scene.scene("odd")
    oracle = O.SlavchevaOracle(**CW.fixed(3))
    trace = []
    oracle.iteration_hook = lambda it, live, warp, *rest: trace.append((live.copy(), warp.copy()))
    live = live0.copy()
    oracle.optimize(live, canonical)
    psi = np.zeros(live0.shape + (3,), F32)
    before = live0
    snapped_total = 0
    for after, update in trace:
        band = CW.band(canonical, before)
        snapped = band & (np.abs(after) == 1) & (np.abs(before) != 1) & ~update.any(axis=-1)
        nxt = CW.compose(psi, update)
        assert _bits_equal(nxt[snapped], psi[snapped] + F32(0.0))
        snapped_total += int(np.count_nonzero(snapped))
        psi, before = nxt, after
    assert snapped_total > 100
    assert _bits_equal(psi, CW.run(canonical, live0, CW.fixed(3)).psi)


# ----------------------------------------------------------------------------------- composing against summing the updates
@pytest.mark.parametrize("d", [2, 3])
def test_the_composed_warp_explains_the_call_better_than_the_summed_updates(d):
    """band means of |live_0 o (id + PSI) - live_30|: composed below summed, both below |live_0 - live_30|.  Measured:
    32^3 0.0086 / 0.0147 / 0.0566, 64^2 0.00016 / 0.00048 / 0.0264"""
    canonical, live = _sphere(d)
    result = CW.run(canonical, live, CW.fixed(30))
    composed, summed, untouched = CW.consistency(canonical, live, result)
    print("sphere pair %s, 30 iterations: band mean |live_0 o (id + PSI) - live_30| = %.6f composed, %.6f summed; "
          "|live_0 - live_30| = %.6f" % (live.shape, composed, summed, untouched))
    assert result.iteration_count == 30
    assert composed < summed < untouched


# --------------------------------------------------------------------------------------------- the restated chain
@functools.lru_cache(maxsize=None)
def chain():
    """tests/deforming_scene.py fused through the KillingFusion oracle's cumulative warp.  The level-set term is OFF: the
    voxels behind the model's band were never observed and keep +1 where the live volume has -1; across that step the
    term produces updates of 14 voxels per iteration (the reference's behaviour on such a field) and the chain changes the
    model by 0.17 per voxel instead of 0.070"""
    return CW.deforming_chain(CW.fixed(30, level_set_term_enabled=False))


def test_the_restated_chain_fuses_the_growing_sphere_through_the_cumulative_warp():
    """test_gpu_warped_fusion's condition: through PSI frame 1 changes the model near its surface by less than half of what
    it changes it by when fused rigidly (0.070 against 0.212 here; HierarchicalOptimizer3d gives 0.024)"""
    t0, W0, psi, t1, W1, rec, rigid, result = chain()
    through, rigidly = D.model_change(t0, t1), D.model_change(t0, rigid)
    print("mean |change| near the surface: %.6f through the cumulative warp, %.6f rigidly; longest update %.3f voxels"
          % (through, rigidly, max(result.log["max_warps"])))
    assert through < 0.5 * rigidly
    assert rec["warp_rejected"] == 0 and rec["fused"] > 1000
    assert result.iteration_count == 30 and np.count_nonzero(psi.any(axis=-1)) > 1000


# ------------------------------------------------------------------------- what the GPU tests assume about their inputs
def test_the_orthographic_pair_moves_by_more_than_a_cell_and_out_of_the_array():
    canonical, live = CW.ortho64()
    assert canonical.shape == live.shape == (64, 64)
    result = CW.run(canonical, live, CW.fixed(10))
    maxima = np.float32(result.log["max_warps"])
    print("orthographic 64^2, KillingFusion, 10 iterations: longest updates %s" % np.round(maxima, 2))
    assert result.iteration_count == 10 and maxima.min() > 2 and np.isfinite(result.psi).all()
    pos = O._grid_positions(np.ascontiguousarray(result.warp))
    assert any(((p < 0) | (p > 63)).any() for p in pos)  # the last update alone gathers outside the array


def test_the_smooth_pair_lists_every_voxel_and_stays_finite():
    canonical, live = CW.smooth_pair((81, 81, 81))
    assert CW.band(canonical, live).all()
    result = CW.run(canonical, live, CW.fixed(2))
    assert result.iteration_count == 2 and np.isfinite(result.psi).all() and np.isfinite(result.live).all()
    assert 0.01 < max(result.log["max_warps"]) < 2 and np.count_nonzero(result.psi.any(axis=-1)) > 500000


# ------------------------------------------------------------------------------------------- the library and the host
NAME = "lsf_cumulative_warp_compose"


def test_the_built_library_exports_the_entry_point():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, NAME) and NAME in L.PROTOTYPES and getattr(L.lib, NAME).restype is ctypes.c_int
    args = L.PROTOTYPES[NAME][1]
    assert len(args) == 8 and args[3]._type_ is L.Grid and args[4]._type_ is L.Gate and args[6] is ctypes.c_int64
    assert L.ABI_VERSION == 4
    grid = lsf.device.make_grid((4, 5, 6))
    assert getattr(L.lib, NAME)(None, None, None, ctypes.byref(grid), None, None, 0, None) == -1
    assert getattr(L.lib, NAME)(None, None, None, None, None, None, 0, None) == -1


# a child without torch and with every GPU hidden: the entry point's own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
fn = lib.lsf_cumulative_warp_compose
fn.restype = ctypes.c_int
fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_void_p]
out = []
for case in json.load(sys.stdin):
    if case["passes"] and not hidden:  # never launch on made-up pointers
        out.append(None)
        continue
    grid = ctypes.create_string_buffer(bytes.fromhex(case["grid"])) if case["grid"] else None
    gate = ctypes.create_string_buffer(bytes.fromhex(case["gate"])) if case["gate"] else None
    state, psi_in, psi_out, band = case["pointers"]
    out.append(fn(state, psi_in, psi_out, grid, gate, band, case["count"], None))
print(json.dumps(out))
"""


def test_the_entry_point_refuses_on_its_own():
    """NULL buffers, a base off 16-byte alignment, psi_in == psi_out, every pairwise overlap among state, psi_in and psi_out
    at the last record of the earlier buffer, bad dims and extents, a negative count, a list without a count and a count
    without a list.  Made-up addresses: every case must return before a launch"""
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    shape = (6, 7, 9)
    size = 6 * 7 * 9 * 16
    base = dict(state=0x10000000, psi_in=0x10100000, psi_out=0x10200000, band=0x10300000)

    def grid(shape_=shape, **fields):
        g = lsf.device.make_grid(shape_)
        for k, v in fields.items():
            setattr(g, k, v)
        return bytes(g).hex()

    def case(passes=False, grid_=None, gate=None, count=0, no_grid=False, **moved):
        at = dict(base, band=None)
        at.update(moved)
        return dict(passes=passes, grid=None if no_grid else (grid_ or grid()), gate=gate, count=count,
                    pointers=[at[k] for k in ("state", "psi_in", "psi_out", "band")])

    refused = {"no grid": case(no_grid=True), "dims 4": case(grid_=grid(dims=4)), "dims 1": case(grid_=grid(dims=1)),
               "two dimensions with slices": case(grid_=grid(dims=2)), "nx 0": case(grid_=grid(nx=0)),
               "ny negative": case(grid_=grid(ny=-3)), "nz 0": case(grid_=grid(nz=0)),
               "z range past the array": case(grid_=grid(z_end=7)), "z range reversed": case(grid_=grid(z_begin=4, z_end=2)),
               "too many voxels": case(grid_=grid(nz=2048, ny=2048, nx=2048, z_end=2048)),
               "cut along y": case(grid_=grid(y_global_offset=2, ny_global=12)),
               "psi_in == psi_out": case(psi_out=base["psi_in"]),
               "a negative count": case(band=base["band"], count=-1),
               "a negative count without a list": case(count=-5),
               "a count past int32": case(band=base["band"], count=1 << 31),
               "a list without a count": case(band=base["band"], count=0),
               "a count without a list": case(count=12)}
    for name in ("state", "psi_in", "psi_out"):
        refused["no %s" % name] = case(**{name: None})
        for off in (4, 8, 12):
            refused["%s %d bytes off alignment" % (name, off)] = case(**{name: base[name] + off})
    order = ("state", "psi_in", "psi_out")
    for i, first in enumerate(order):  # the later buffer begins on the earlier one's last record, or ends on its first
        for second in order[i + 1:]:
            refused["%s overlaps the end of %s" % (second, first)] = case(**{second: base[first] + size - 16})
            refused["%s overlaps the start of %s" % (second, first)] = case(**{second: base[first] - size + 16})
    gate = bytes(L.Gate(0, L.GATE_SLAVCHEVA, 0.1, 10000.0)).hex()  # no previous record: always open
    passing = {"the dense walk": case(passes=True), "a list": case(passes=True, band=base["band"], count=12),
               "an open gate": case(passes=True, gate=gate, band=base["band"], count=1),
               "two dimensions": case(passes=True, grid_=grid((7, 9))),
               "psi_out right behind psi_in": case(passes=True, psi_out=base["psi_in"] + size),
               "psi_in right behind state": case(passes=True, psi_in=base["state"] + size),
               "a z range": case(passes=True, grid_=grid(z_begin=2, z_end=5))}
    cases = dict(refused, **passing)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", _CHILD, L.LIB_PATH], input=json.dumps(list(cases.values())),
                          capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stderr
    status = dict(zip(cases, json.loads(done.stdout)))
    for name in refused:
        assert status[name] == -1, (name, status[name])
    for name in passing:  # past every check: without a device the launch itself fails; None where a device was visible
        assert status[name] is None or status[name] not in (0, -1), (name, status[name])


# ------------------------------------------------------------------------------------------------------ constructors
class _ActiveComm:
    active = True


def test_the_keyword_is_refused_with_sobolev_smoothing_and_with_a_slab_comm():
    import levelsetfusion_python_amd as lsf
    kernel = O.generate_1d_sobolev_kernel(7, 0.1)
    for cls, n in ((lsf.SlavchevaOptimizer2d, 64), (lsf.SlavchevaOptimizer3d, 32)):
        with pytest.raises(ValueError, match="sobolev_smoothing_enabled"):
            cls(out_path=None, field_size=n, sobolev_smoothing_enabled=True, sobolev_kernel=kernel, cumulative_warp=True)
        with pytest.raises(ValueError, match="comm"):
            cls(out_path=None, field_size=n, comm=_ActiveComm(), cumulative_warp=True)
        # each of them is fine without the keyword, and the keyword is fine without them
        cls(out_path=None, field_size=n, sobolev_smoothing_enabled=True, sobolev_kernel=kernel)
        opt = cls(out_path=None, field_size=n, cumulative_warp=True)
        assert opt.cumulative_warp and opt.engine.cumulative_warp and opt.cumulative_warp_field is None
        off = cls(out_path=None, field_size=n)
        assert not off.cumulative_warp and not off.engine.cumulative_warp and off.cumulative_warp_field is None


def test_the_sequence_accepts_the_depth_mode_options_with_the_keyword_only(monkeypatch):
    """the constructor's refusals come before it asks for a GPU: with every GPU hidden, a combination it accepts gets as
    far as that question and a combination it refuses does not"""
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_core
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(device_core, "_gpu_seen", False)
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    killing = dict(out_path=None, field_size=32, smoothing_term_method=lsf.SmoothingTermMethod.KILLING)
    composed = lsf.SlavchevaOptimizer3d(cumulative_warp=True, **killing)
    plain = lsf.SlavchevaOptimizer3d(**killing)
    flat = lsf.SlavchevaOptimizer2d(out_path=None, field_size=32, cumulative_warp=True)
    options = (dict(carve=True), dict(confidence=lsf.DepthConfidence()), dict(colour=True),
               dict(carve=True, confidence=lsf.DepthConfidence(), colour=True), dict())
    for kw in options:
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=composed, **kw)
    for other in (plain, flat):
        for kw in options[:-1]:
            with pytest.raises(ValueError, match="nonrigid_optimizer"):
                lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=other, **kw)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=other)
