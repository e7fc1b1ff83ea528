"""CPU checks of fusion into a canonical TSDF volume: the numpy restatement of the rule (tests/fusion_restatement.py)
against INTEGRATION.md section 3, the analytic scene (tests/fusion_scene.py) against the generator and the tracker, the
ctypes layout of lsf_fusion_params, host argument checks, the exports and the no-CPU-path error."""
import ctypes
import math
import os

import numpy as np
import pytest

import fusion_restatement as F
import fusion_scene as S
import rigid3d_restatement as R3
from conftest import ROOT

# the tracker of one scene pair (frame 0's TSDF, frame 1 under STEP), 64^3, 60 iterations from zero, measured on the
# restatement: |twist - truth| = 1.5e-3 m in translation and 3.1e-3 rad in rotation at most.  The SDF-2-SDF minimum of
# two projective TSDFs of this scene is not exactly at the true pose (the energy there is 149, at the minimum 123);
# the tolerances keep a margin of about 4x.
PAIR_ATOL_T, PAIR_ATOL_R = 6e-3, 1.2e-2


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_first_observation_copies_the_live_value():
    rng = np.random.default_rng(1)
    live = rng.uniform(-0.999, 0.999, (7, 9, 5)).astype(np.float32)
    t, w = F.empty_model(live.shape)
    t1, w1, rec = F.fuse(t, w, live)
    assert np.array_equal(_bits(t1), _bits(live)) and np.all(w1 == 1)
    assert rec["fused"] == rec["first_seen"] == live.size
    assert rec["max_abs_change"] == float(np.max(np.abs(live - np.float32(1))))


def test_the_rule_in_float32_and_the_cap():
    t = np.array([0.5, -0.25, 0.75, 0.1], np.float32)
    W = np.array([3, 2, 5, 0], np.float32)
    l = np.array([0.1, 0.3, -0.5, 0.2], np.float32)
    t1, w1, rec = F.fuse(t, W, l, w=2.0, max_weight=4.0)
    W1 = W + np.float32(2)
    want = (W * t + np.float32(2) * l) / W1  # the uncapped W1 in the average
    assert np.array_equal(_bits(t1), _bits(want))
    assert w1.tolist() == [4, 4, 4, 2]
    assert t1[0] == np.float32((np.float32(1.5) + np.float32(0.2)) / np.float32(5))
    assert rec["first_seen"] == 1 and rec["fused"] == 4
    assert rec["sum_abs_change"] == float(np.sum(np.abs(want - t).astype(np.float64)))


def test_unobserved_voxels_are_untouched():
    t = np.array([0.3, -0.7, np.float32(0.2), 0.9, 0.4, 1.0], np.float32)
    W = np.array([2, 1, 0, 7, 3, 0], np.float32)
    l = np.array([1.0, -1.0, np.nan, np.inf, -np.inf, 0.5], np.float32)
    t1, w1, rec = F.fuse(t, W, l)
    assert np.array_equal(_bits(t1[:5]), _bits(t[:5])) and np.array_equal(w1[:5], W[:5])
    assert t1[5] == np.float32(0.5) and w1[5] == 1
    assert rec == {"fused": 1, "first_seen": 1, "sum_abs_change": 0.5, "max_abs_change": 0.5}
    _, _, none = F.fuse(t, W, np.ones_like(t))
    assert none == {"fused": 0, "first_seen": 0, "sum_abs_change": 0.0, "max_abs_change": 0.0}


def test_record_counts():
    rng = np.random.default_rng(2)
    live = rng.uniform(-1.5, 1.5, 4000).astype(np.float32)
    W = rng.choice(np.array([0, 1, 4], np.float32), 4000)
    t = rng.uniform(-1, 1, 4000).astype(np.float32)
    _, _, rec = F.fuse(t, W, live)
    obs = (live > -1) & (live < 1)
    assert rec["fused"] == int(obs.sum()) and rec["first_seen"] == int((obs & (W == 0)).sum())


def test_the_scene_agrees_with_the_generator():
    """frame k's TSDF under its true twist matches frame 0's near the surface within a voxel (0.1 in TSDF units at a
    20-voxel band); measured at 64^3: mean 0.007 / 0.010, 99th percentile 0.042 / 0.058 for frames 1 / 2"""
    n = 64
    off = S.offset(n)
    frames = S.frames(3)
    t0 = R3.live_volume(frames[0], S.K, 1.0, (n,) * 3, off, np.zeros(6))
    near = np.abs(t0) < 0.5
    assert near.sum() > 10000
    for k in (1, 2):
        tk = R3.live_volume(frames[k], S.K, 1.0, (n,) * 3, off, S.true_twist(k))
        d = np.abs(tk - t0)[near]
        assert d.mean() < 0.025 and np.percentile(d, 99) < 0.1, (k, d.mean(), np.percentile(d, 99))


def test_the_restated_tracker_recovers_a_scene_pair():
    n = 64
    off = S.offset(n)
    f0, f1 = S.frames(2)
    canonical = R3.tsdf_nearest(f0, S.K, 1.0, (n,) * 3, off)
    records, twist = R3.optimize(canonical, f1, S.K, 1.0, off, 60, 20)
    assert not any(r["skipped"] for r in records)
    err = np.abs(twist - S.true_twist(1))
    assert np.all(err[:3] <= PAIR_ATOL_T) and np.all(err[3:] <= PAIR_ATOL_R), err


def test_restated_sequence():
    """48^3, four frames, 60 rigid iterations: the restated SequenceFusion3d without a non-rigid step.  Measured: frame
    0 fuses 32916 voxels, all first seen; later frames 7703-8217.  Tracking against the fused model does NOT recover the
    true twists on this scene (errors up to 0.21 m and 0.49 rad): the rule leaves the voxels behind the band, where a
    frame's TSDF is -1, at the model's initial +1, and the layer of voxels just past the back edge of each live band then
    carries a residual of 2 with a non-zero twist gradient.  The numbers are pinned here so that a change of the rule
    or of the tracker shows."""
    n = 48
    off = S.offset(n)
    tsdf, weight, twists, records = F.sequence(S.frames(4), S.K, 1.0, (n,) * 3, off, 60)
    assert [r["fused"] for r in records] == [32916, 8217, 7705, 7703]
    assert [r["first_seen"] for r in records] == [32916, 2205, 80, 32]
    assert np.array_equal(twists[0], np.zeros(6))
    assert np.all(weight <= 4) and np.all(weight[tsdf == 1] == 0) and int((weight > 0).sum()) > 32916
    err = np.abs(np.array(twists) - np.array([S.true_twist(k) for k in range(4)]))
    assert err[1:, :3].max() > 0.05  # the documented failure of tracking against the model


def test_params_layout():
    import levelsetfusion_python_amd._lib as lib
    p = lib.FusionParams
    assert [f[0] for f in p._fields_] == ["tsdf", "twist", "array_offset", "depth", "height", "width", "weight",
                                          "max_weight", "depth_dtype"]
    assert ctypes.sizeof(p) == ctypes.sizeof(lib.TsdfParams) + 8 * 6 + 8 * 3 + 4 * 6
    assert p.twist.offset == ctypes.sizeof(lib.TsdfParams) and p.weight.offset == p.width.offset + 4
    assert lib.FUSION_RECORD_DOUBLES == 8 and lib.FUSION_MAX_BLOCKS == 2048
    assert lib.FUSION_SCRATCH_BYTES == 2048 * 4 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for macro, value in (("LSF_FUSION_RECORD_DOUBLES", "8"), ("LSF_FUSION_MAX_BLOCKS", "2048"),
                         ("LSF_FUSION_SCRATCH_BYTES", "(LSF_FUSION_MAX_BLOCKS * 4 * 8)")):
        assert "#define %s %s" % (macro, value) in header
    for name in ("lsf_fusion_integrate_volume", "lsf_fusion_integrate_depth"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None


def test_the_c_abi_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    p = lib.FusionParams()
    p.depth, p.height, p.width, p.weight, p.max_weight = 4, 4, 4, 1.0, math.inf
    p.tsdf.image_width, p.tsdf.image_height, p.tsdf.narrow_band_half_width = 8, 8, 0.04
    a, b, c, d, e = (ctypes.c_void_p(16 * k) for k in (1, 2, 3, 4, 5))  # never dereferenced: every call is refused
    for field, value in (("depth", 0), ("width", -1), ("weight", 0.0), ("weight", math.inf), ("weight", math.nan),
                         ("max_weight", 0.0), ("max_weight", math.nan), ("depth_dtype", 7)):
        q = lib.FusionParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.lib.lsf_fusion_integrate_depth(a, b, c, d, e, ctypes.byref(q), None) == -1, field
        if field != "depth_dtype":
            assert lib.lib.lsf_fusion_integrate_volume(a, b, c, d, e, ctypes.byref(q), None) == -1, field
    for f in (lib.lib.lsf_fusion_integrate_volume, lib.lib.lsf_fusion_integrate_depth):
        assert f(a, a, c, d, e, ctypes.byref(p), None) == -1  # tsdf is weight
        assert f(a, b, a, d, e, ctypes.byref(p), None) == -1  # the source aliases the model
        assert f(None, b, c, d, e, ctypes.byref(p), None) == -1
        assert f(a, b, c, None, e, ctypes.byref(p), None) == -1
        assert f(a, b, c, d, None, ctypes.byref(p), None) == -1
        assert f(a, b, c, d, e, None, None) == -1
    q = lib.FusionParams.from_buffer_copy(p)
    q.tsdf.narrow_band_half_width = 0.0
    assert lib.lib.lsf_fusion_integrate_depth(a, b, c, d, e, ctypes.byref(q), None) == -1


def test_host_argument_checks():
    from levelsetfusion_python_amd import device_fusion
    assert device_fusion.fusion_weights(2, math.inf) == (2.0, math.inf)
    for w, cap in ((0, 1), (-1, 1), (math.inf, 1), (math.nan, 1), (1e39, 1), (1, 0), (1, -1), (1, math.nan)):
        with pytest.raises(ValueError):
            device_fusion.fusion_weights(w, cap)
    r = device_fusion.unpack_record(np.array([5, 2, 0.25, 0.125, 0, 0, 0, 0]))
    assert r == {"fused": 5, "first_seen": 2, "sum_abs_change": 0.25, "max_abs_change": 0.125}
    assert device_fusion.RECORD_FIELDS == tuple(r)


def test_package_exports_fusion():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import fusion
    assert lsf.fusion is fusion and lsf.SequenceFusion3d is fusion.SequenceFusion3d
    assert lsf.CanonicalVolume is fusion.CanonicalVolume
    for name in ("fusion", "SequenceFusion3d", "CanonicalVolume"):
        assert name in lsf.__all__
    for name in ("integrate_volume", "integrate_depth", "reset"):
        assert callable(getattr(fusion.CanonicalVolume, name))
    assert callable(fusion.SequenceFusion3d.integrate)
    assert "synchronisation" in fusion.__doc__


def test_no_cpu_path():
    import torch
    from levelsetfusion_python_amd import device_fusion, fusion
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        fusion.CanonicalVolume((4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        fusion.SequenceFusion3d(cam, 8, [0, 0, 100])
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        device_fusion.integrate_volume(z, z.clone(), z.clone())
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        device_fusion.integrate_depth(z, z.clone(), z, 1, cam, [0, 0, 0], np.zeros(6))
