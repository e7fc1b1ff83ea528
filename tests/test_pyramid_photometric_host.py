"""CPU checks of the intensity pyramids and of the joint geometric and photometric ICP over the depth pyramid: the
restatement's own properties (tests/pyramid_photometric_restatement.py), the accuracy bounds the GPU tests import, the
ctypes layout of the two parameter structs, the header's macros, the exports, and the refusal of bad arguments by both C
entry points and by the Python interfaces."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_pyramid_restatement as DP
import fusion_scene as S
import photometric_restatement as PR
import pyramid_photometric_restatement as PP
import textured_wall_scene as W
from conftest import ROOT
from test_photometric_host import SEQUENCE_COLOUR_BAND, SEQUENCE_FRAMES, SEQUENCE_N, sequence_frames, wall_inputs

LAMBDA = 0.1
LEVELS, RUN_ITERATIONS = 3, (4, 4, 6)
# the trackers of the accuracy tests gate the geometric pairs at 20 degrees, DepthPyramid's tuned value
GATE_ANGLE = math.radians(20.0)

# The accuracy bounds of the GPU tests: twice the restatement's own error on the same inputs, measured here on the CPU
# (test_restated_run_meets_its_bound and test_restated_sequence_meets_its_bound pin the measurements to 2 %); the device
# run differs from the restatement by the order of its sums and the last bit of the filter's exp only.
# The whole run on the 152 x 120 wall (analytic prediction at 0, live frame at textured_wall_scene.MOTION, lambda 0.1,
# the default DepthPyramid of three levels, iterations (4, 4, 6), the 20 degree gate): the final twist errs by
# 7.3923e-6 m and 1.5468e-5 rad.  (The strided run of tests/test_photometric_host.py ends nearer, 2.1e-6 m, with 19
# iterations against these 14.)
RUN_ERROR_T, RUN_ERROR_R = 7.3923e-6, 1.5468e-5
RUN_ATOL_T, RUN_ATOL_R = 2 * RUN_ERROR_T, 2 * RUN_ERROR_R
# The restated three-frame sequence of the wall (test_photometric_host.sequence_frames: fusion_scene's K, 640 x 480
# and STEP; 64^3, colour_band 0.25, lambda 0.1, the same pyramid, schedule and gate): the worst frame errs by
# 2.2155e-5 m and 5.7769e-5 rad -- the strided sequence's figures, both ending on every pixel of the full image.
SEQUENCE_ERROR_T, SEQUENCE_ERROR_R = 2.2155e-5, 5.7769e-5
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 2 * SEQUENCE_ERROR_T, 2 * SEQUENCE_ERROR_R
# against a vacuous pass: the least share of the geometric pairs that must carry a photometric term, on every record
PHOTOMETRIC_SHARE = 0.75


def restated_pyramids(level0=None, levels=LEVELS):
    """(depth pyramid, live intensity pyramid, prediction intensity pyramid) of the wall inputs with the default
    settings; level0: the depth pyramid's level 0 to start from (the device's own, whose exp may differ in the last
    bit), None for the restated filter"""
    pd, pn, pc, depth, image = wall_inputs()
    if level0 is None:
        level0 = DP.bilateral(depth, 1.0)
    return (DP.pyramid_from_level0(level0, W.K_SMALL, levels), PP.live_pyramid(image, levels),
            PP.prediction_pyramid(pc, levels))


def restated_run_from(level0=None):
    pd, pn, _, _, _ = wall_inputs()
    lv, il, ip = restated_pyramids(level0)
    return PP.icp(lv, il, ip, pd, pn, W.K_SMALL, np.zeros(6), LAMBDA, None, RUN_ITERATIONS,
                  cos_max=DP.cos_of(GATE_ANGLE))


@functools.lru_cache(maxsize=None)
def restated_run():
    """(records, final twist, residuals, intensity residuals) of the whole joint pyramid run on the wall"""
    return restated_run_from()


@functools.lru_cache(maxsize=None)
def restated_sequence():
    """pyramid_photometric_restatement.sequence of the wall's three frames; nothing modifies it"""
    frames = sequence_frames()
    n = SEQUENCE_N
    return PP.sequence([f[0] for f in frames], [f[1] for f in frames], S.K, 1.0, (n,) * 3, S.offset(n), LAMBDA,
                       RUN_ITERATIONS, cos_max=DP.cos_of(GATE_ANGLE), colour_band=SEQUENCE_COLOUR_BAND)


def holed_prediction(pc):
    """the wall's colour prediction with a rectangle of NaN (three payloads) and a lone NaN"""
    out = np.array(pc)
    y = out[..., 3].view(np.uint32)
    y[40:70, 50:100] = 0x7fc00000
    y[41, 51], y[42, 52] = 0x7fc01234, 0xffc00001
    y[100, 20] = 0x7fc00000
    return out


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_level0_of_both_sources():
    _, _, pc, _, image = wall_inputs()
    holed = holed_prediction(pc)
    level0 = PP.prediction_level0(holed)
    assert level0.dtype == np.float32 and np.array_equal(_bits(level0), _bits(holed[..., 3]))  # payloads included
    assert _bits(level0)[41, 51] == 0x7fc01234 and _bits(level0)[42, 52] == 0xffc00001
    assert not np.shares_memory(level0, holed)
    live = PP.live_level0(image)
    assert live.dtype == np.float32 and np.array_equal(live, W.luminance(image).astype(np.float32))
    with pytest.raises(ValueError):
        PP.live_level0(image.astype(np.float32))
    with pytest.raises(ValueError):
        PP.prediction_level0(pc[..., :3])


def test_one_nan_in_a_block_makes_one_nan_in_the_next_level():
    rng = np.random.default_rng(5)
    level = rng.random((53, 75)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        holed = level.copy()
        holed[21, 30] = bad  # block (10, 15), its second row
        down = PP.downsample(holed)
        assert down.shape == (26, 37) and np.isnan(down).sum() == 1 and np.isnan(down[10, 15])
        clean = PP.downsample(level)
        assert np.isfinite(clean).all()
        keep = np.ones(down.shape, bool)
        keep[10, 15] = False
        assert np.array_equal(_bits(down[keep]), _bits(clean[keep]))
    # the last row and column of an odd level are never read
    holed = level.copy()
    holed[52, :] = np.nan
    holed[:, 74] = np.nan
    assert np.array_equal(_bits(PP.downsample(holed)), _bits(PP.downsample(level)))
    d = level.astype(np.float64)
    want = (((d[0, 0] + d[0, 1]) + (d[1, 0] + d[1, 1])) / 4.0).astype(np.float32)
    assert PP.downsample(level)[0, 0] == want


def test_a_constant_image_stays_constant_at_every_level():
    for value in (np.float32(0.3), np.float32(1.0), np.float32(1e-30)):
        levels = PP.pyramid_from_level0(np.full((53, 75), value, np.float32), 4)
        assert [l.shape for l in levels] == [(53, 75), (26, 37), (13, 18), (6, 9)]
        assert all(np.all(l == value) for l in levels)  # (c + c) + (c + c) = 4 c exactly, and 4 c / 4 = c
    with pytest.raises(ValueError):
        PP.pyramid_from_level0(np.zeros((4, 9), np.float32), 4)


def test_one_level_without_filter_or_gate_is_the_strided_iteration():
    """a one-level pyramid with radius 0 and no gate against photometric_restatement.iteration at stride 1.  The pairs,
    r, J and J_I are the same doubles, so the counts are equal and A is equal bit for bit.  r_I differs in I_l alone:
    the pyramid holds float32(I_l), and I_l < 1, so |dI_l| <= 2^-25 and |d b_i| <= 2^-25 lambda^2 sum |J_I,i| over the
    photometric pairs (plus the two sums' own rounding, 1e-12 of b_abs).  Against b_abs >= lambda^2 sum |J_I,i| |r_I|
    that is at most 2^-25 / <|r_I|>, the |J_I|-weighted mean of |r_I|, which on these inputs is about 0.1: 3.1e-7 of
    b_abs at the most, inside the 1e-6 the test allows (the measured difference, whose roundings carry both signs, is
    2e-9).  The test asserts the derived bound, that it lies inside 1e-6, and 1e-6 itself."""
    pd, pn, pc, depth, image = wall_inputs()
    start, zero = np.array([0.0004, -0.0003, 0.0002, 0.001, -0.002, 0.0015]), np.zeros(6)
    lv = DP.pyramid(depth, 1.0, W.K_SMALL, levels=1, radius=0)
    il, ip = PP.live_pyramid(image, 1)[0], PP.prediction_pyramid(pc, 1)[0]
    got, res, ires, _ = PP.iteration(lv[0][0], lv[1][0], il, ip, lv[2][0], pd, pn, W.K_SMALL, start, zero, LAMBDA)
    want, want_res, want_ires, _ = PR.iteration(depth, image, pd, pn, pc, W.K_SMALL, 1.0, start, zero, LAMBDA)
    assert (got["count"], got["photometric_count"]) == (want["count"], want["photometric_count"])
    assert got["count"] > 10000 and got["photometric_count"] > PHOTOMETRIC_SHARE * got["count"]
    assert np.array_equal(got["A"], want["A"]) and np.array_equal(_bits(res), _bits(want_res))
    rows, cols, valid, _, g, _, _ = PR.I.associate(depth, pd, pn, W.K_SMALL, 1.0, start, zero)
    has, rI, JI = PR.photometric_terms(image, pc, W.K_SMALL, zero, rows, cols, valid, g)
    derived = np.array([2.0 ** -25 * LAMBDA * LAMBDA * np.abs(j[has]).sum() for j in JI]) + 1e-12 * want["b_abs"]
    assert np.all(derived <= 1e-6 * want["b_abs"]), derived / want["b_abs"]
    assert np.all(np.abs(got["b"] - want["b"]) <= derived)
    assert np.all(np.abs(got["b"] - want["b"]) <= 1e-6 * want["b_abs"])
    assert np.nanmax(np.abs(ires.astype(np.float64) - want_ires)) <= 2.0 ** -24


def test_geometry_alone_skips_every_iteration_on_the_wall():
    """the geometric pyramid run (lsf_icp_run_pyramid's restatement) on the same inputs: A is singular on a flat wall,
    every iteration is skipped and the twist stays -- what the joint run gains, the photometric term gives"""
    pd, pn, _, _, _ = wall_inputs()
    lv, _, _ = restated_pyramids()
    for cos_max in (None, DP.cos_of(GATE_ANGLE)):
        records, twist, _ = DP.icp(lv, pd, pn, W.K_SMALL, np.zeros(6), None, RUN_ITERATIONS, cos_max=cos_max)
        assert len(records) == 14 and all(r["skipped"] == 1 and r["count"] > 1000 for r in records)
        assert np.array_equal(twist, np.zeros(6))


def test_restated_run_meets_its_bound():
    """the joint pyramid run updates in every iteration, at least PHOTOMETRIC_SHARE of the geometric pairs carry a
    photometric term on every record (about 3 pixels of shift and one row and column of the bilinear border leave 0.94
    at 38 x 30), the gate rejects pairs, and the final twist's error is the recorded one"""
    records, twist, res, ires = restated_run()
    assert [r["level"] for r in records] == [0] * 4 + [1] * 4 + [2] * 6
    assert all(r["skipped"] == 0 for r in records)
    for r in records:
        assert r["count"] > 1000 and r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"], r
    print("photometric share per record:", [round(r["photometric_count"] / r["count"], 3) for r in records])
    assert records[0]["angle_rejected"] > 0
    assert res.shape == ires.shape == W.SHAPE_SMALL and np.isfinite(ires).sum() == records[-1]["photometric_count"]
    err = np.abs(twist - W.MOTION)
    print("restated joint pyramid run, |twist - truth|:", err)
    np.testing.assert_allclose([err[:3].max(), err[3:].max()], [RUN_ERROR_T, RUN_ERROR_R], rtol=0.02)
    assert err[:3].max() <= RUN_ATOL_T and err[3:].max() <= RUN_ATOL_R


def test_restated_sequence_meets_its_bound():
    _, _, _, twists, hits, icp = restated_sequence()
    truth = np.array([S.true_twist(k) for k in range(SEQUENCE_FRAMES)])
    err = np.abs(np.array(twists) - truth)
    assert hits[0] is None and min(hits[1:]) > 40000 and icp[0] == []
    for recs in icp[1:]:
        assert len(recs) == 14
        for r in recs:
            assert r["skipped"] == 0 and r["count"] > 1000
            assert r["photometric_count"] >= PHOTOMETRIC_SHARE * r["count"], r
    print("restated joint pyramid sequence, |twist - truth| per frame:\n", err)
    np.testing.assert_allclose([err[1:, :3].max(), err[1:, 3:].max()], [SEQUENCE_ERROR_T, SEQUENCE_ERROR_R], rtol=0.02)
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    p = lib.IcpPyramidPhotometricParams
    assert [f[0] for f in p._fields_] == ["fx", "fy", "cx", "cy", "max_distance", "cos_max_angle",
                                          "photometric_weight", "max_intensity_difference", "twist_p", "height",
                                          "width", "pyramid_levels", "levels", "angle_gate", "reserved", "iterations"]
    assert ctypes.sizeof(p) == 14 * 8 + 6 * 4 + 4 * 4 and p.twist_p.offset == 64 and p.height.offset == 112
    assert p.iterations.offset == 136
    q = lib.IntensityPyramidParams
    assert [f[0] for f in q._fields_] == ["height", "width", "levels", "source"] and ctypes.sizeof(q) == 16
    assert (lib.INTENSITY_SOURCE_COLOUR, lib.INTENSITY_SOURCE_PREDICTION) == (0, 1)
    assert lib.ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES == 2 * 256 * 32 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    assert "#define LSF_ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 32 * 8)" in header
    assert "#define LSF_INTENSITY_SOURCE_COLOUR 0" in header and "#define LSF_INTENSITY_SOURCE_PREDICTION 1" in header
    assert "#define LSF_ABI_VERSION 4" in header and lib.ABI_VERSION == 4 and lib.lib.lsf_abi_version() == 4
    for name in ("lsf_intensity_pyramid", "lsf_icp_run_pyramid_photometric"):
        assert name in lib.PROTOTYPES and getattr(lib.lib, name) is not None and name + "(" in header
    assert len(lib.PROTOTYPES["lsf_intensity_pyramid"][1]) == 4
    assert len(lib.PROTOTYPES["lsf_icp_run_pyramid_photometric"][1]) == 13


# a child without torch and with every GPU hidden: the entry points' refusals are host code, and a call that a refusal
# should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
out = []
for case in json.load(sys.stdin):
    if case["passes"] and not hidden:  # never launch on made-up pointers
        out.append(None)
        continue
    fn = getattr(lib, case["entry"])
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * (len(case["pointers"]) + 2)
    params = ctypes.create_string_buffer(bytes.fromhex(case["params"])) if case["params"] else None
    out.append(fn(*case["pointers"], params, None))
print(json.dumps(out))
"""


def _refusals(cases):
    import levelsetfusion_python_amd._lib as L
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    done = subprocess.run([sys.executable, "-c", _CHILD, L.LIB_PATH], input=json.dumps(list(cases.values())),
                          capture_output=True, text=True, env=env, timeout=120)
    assert done.returncode == 0, done.stderr
    return dict(zip(cases, json.loads(done.stdout)))


def _check(cases):
    status = _refusals(cases)
    for name, case in cases.items():
        if case["want"] is not None:
            assert status[name] == case["want"], (name, status[name])
        else:  # past every check: without a device the launch itself fails; None where a device was visible
            assert status[name] is None or status[name] not in (0, -1), (name, status[name])


def test_the_intensity_pyramid_entry_point_refuses_bad_arguments_before_launching():
    import levelsetfusion_python_amd._lib as lib
    h, w, levels = 48, 64, 3
    pixels = sum((h >> l) * (w >> l) for l in range(levels))
    image, out = 0x10000000, 0x10100000

    def case(want=-1, pointers=(image, out), no_params=False, **fields):
        p = lib.IntensityPyramidParams()
        p.height, p.width, p.levels, p.source = h, w, levels, lib.INTENSITY_SOURCE_PREDICTION
        for k, v in fields.items():
            setattr(p, k, v)
        return dict(entry="lsf_intensity_pyramid", passes=want is None, want=want, pointers=list(pointers),
                    params=None if no_params else bytes(p).hex())

    cases = {"no image": case(pointers=(None, out)), "no output": case(pointers=(image, None)),
             "no params": case(no_params=True)}
    for field, value in (("height", 0), ("width", -1), ("levels", 0), ("levels", 5), ("source", 2), ("source", -1)):
        cases["%s %r" % (field, value)] = case(**{field: value})
    cases["no 4-level pyramid of 48 x 7"] = case(width=7, levels=4)
    cases["too many pixels"] = case(height=1 << 16, width=1 << 15)
    # the prediction image is 16 bytes a pixel, the colour image 3: the output begins on the input's last byte, or
    # ends on its first
    cases["output in the prediction's last byte"] = case(pointers=(image, image + 16 * h * w - 1))
    cases["output over the prediction's first byte"] = case(pointers=(image, image - 4 * pixels + 1))
    cases["output in the colour image's last byte"] = case(pointers=(image, image + 3 * h * w - 1),
                                                           source=lib.INTENSITY_SOURCE_COLOUR)
    cases["the plain call"] = case(want=None)
    cases["output right behind the colour image"] = case(want=None, pointers=(image, image + 3 * h * w),
                                                         source=lib.INTENSITY_SOURCE_COLOUR)
    cases["output right before the prediction"] = case(want=None, pointers=(image, image - 4 * pixels))
    cases["one level of 1 x 1"] = case(want=None, height=1, width=1, levels=1)
    _check(cases)


def test_the_joint_pyramid_entry_point_refuses_bad_arguments_before_launching():
    """lsf_icp_run_pyramid's refusals, lsf_icp_run_photometric's, and the aliasing check over the two intensity
    pyramids and the intensity residual image"""
    import levelsetfusion_python_amd._lib as lib
    h, w, levels = 48, 64, 3
    pyramid = sum((h >> l) * (w >> l) for l in range(levels))
    names = ("live_depth", "live_normals", "live_intensity", "pred_depth", "pred_normals", "pred_intensity", "twist",
             "records", "scratch", "residuals", "intensity_residuals")
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}  # 1 MiB apart: nothing aliases
    sizes = dict(live_depth=4 * pyramid, live_normals=12 * pyramid, live_intensity=4 * pyramid, pred_depth=4 * h * w,
                 pred_normals=12 * h * w, pred_intensity=4 * pyramid)

    def params(iterations=(2, 0, 3), **fields):
        p = lib.IcpPyramidPhotometricParams()
        p.fx, p.fy, p.cx, p.cy, p.max_distance, p.cos_max_angle = 70.0, 70.0, 32.0, 24.0, 0.02, 0.9
        p.photometric_weight, p.max_intensity_difference = 0.1, math.inf
        p.height, p.width, p.pyramid_levels, p.levels, p.angle_gate = h, w, levels, len(iterations), 1
        p.iterations[:len(iterations)] = list(iterations)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def case(want=-1, p=None, no_params=False, **moved):
        at = dict(base, residuals=None, intensity_residuals=None)
        at.update(moved)
        return dict(entry="lsf_icp_run_pyramid_photometric", passes=want is None, want=want,
                    pointers=[at[name] for name in names], params=None if no_params else bytes(p or params()).hex())

    cases = {"no params": case(no_params=True)}
    for name in names[:7] + ("records", "scratch"):  # every required pointer (records: there are iterations)
        cases["no %s" % name] = case(**{name: None})
    for field, value in (("photometric_weight", 0.0), ("photometric_weight", -0.1), ("photometric_weight", math.nan),
                         ("photometric_weight", math.inf), ("max_intensity_difference", 0.0),
                         ("max_intensity_difference", -1.0), ("max_intensity_difference", math.nan),
                         ("height", 0), ("width", -1), ("fx", 0.0), ("fy", math.nan), ("cx", math.inf),
                         ("max_distance", 0.0), ("max_distance", math.nan), ("cos_max_angle", 1.5),
                         ("cos_max_angle", math.nan), ("pyramid_levels", 0), ("pyramid_levels", 5), ("levels", 0),
                         ("levels", 4)):
        cases["%s %r" % (field, value)] = case(p=params(**{field: value}))
    cases["a negative iteration count"] = case(p=params(iterations=(2, -1, 3)))
    bad = params()
    bad.twist_p[4] = math.nan
    cases["twist_p not finite"] = case(p=bad)
    cases["no 4-level pyramid of 48 x 7"] = case(p=params(width=7, pyramid_levels=4))
    # the last iteration runs on level 0 (entry 2): the residual images are 48 x 64
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES, residuals=4 * h * w,
                intensity_residuals=4 * h * w)
    for out, n in outs.items():
        for name, size in sizes.items():
            cases["%s in the last byte of %s" % (out, name)] = case(**{out: base[name] + size - 1})
            cases["%s over the first byte of %s" % (out, name)] = case(**{out: base[name] - n + 1})
    cases["the two residual images alias"] = case(residuals=base["residuals"], intensity_residuals=base["residuals"])
    cases["the intensity residuals alias the scratch"] = case(intensity_residuals=base["scratch"])
    cases["the records alias the twist"] = case(records=base["twist"] + 40)
    # with the last iteration on level 2 the residual images are 12 x 16: one right behind or right before an input
    # passes, one float into it is refused
    coarse = params(iterations=(2, 0, 0))
    cases["coarse residuals right behind an input"] = case(want=None, p=coarse,
                                                           intensity_residuals=base["pred_intensity"] + 4 * pyramid)
    cases["coarse residuals right before an input"] = case(
        want=None, p=coarse, intensity_residuals=base["pred_intensity"] - 4 * (h >> 2) * (w >> 2))
    cases["coarse residuals one float early"] = case(p=coarse,
                                                     intensity_residuals=base["pred_intensity"] + 4 * pyramid - 4)
    cases["the plain call"] = case(want=None)
    cases["both residual images"] = case(want=None, residuals=base["residuals"],
                                         intensity_residuals=base["intensity_residuals"])
    cases["no gate"] = case(want=None, p=params(angle_gate=0))
    cases["nothing to launch"] = case(want=0, p=params(iterations=(0, 0, 0)), records=None,
                                      residuals=base["residuals"], intensity_residuals=base["intensity_residuals"])
    _check(cases)


def test_python_argument_checks():
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_icp, device_intensity_pyramid, fusion, rigid_opt
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, ProjectiveIcp3d
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    assert "IntensityPyramid" in dir(rigid_opt) and IntensityPyramid().levels == 3 and IntensityPyramid(4).levels == 4
    for bad in (0, 5):
        with pytest.raises(ValueError, match="levels"):
            IntensityPyramid(bad)
    p = device_intensity_pyramid.params((480, 640), 3, "colour")
    assert (p.height, p.width, p.levels, p.source) == (480, 640, 3, 0)
    assert device_intensity_pyramid.params((5, 9), 3, "prediction").source == 1
    for shape, levels, source in (((4, 9), 4, "colour"), ((480, 640), 0, "colour"), ((480, 640), 3, "grey"),
                                  ((0, 640), 1, "colour")):
        with pytest.raises(ValueError):
            device_intensity_pyramid.params(shape, levels, source)
    p = device_icp.pyramid_photometric_params(cam, (480, 640), 3, np.arange(6) * 0.01, 0.25, 0.125, (2, 5), 0.03, 0.3)
    assert (p.height, p.width, p.pyramid_levels, p.levels, list(p.iterations), p.angle_gate) == \
        (480, 640, 3, 2, [2, 5, 0, 0], 1)
    assert (p.fx, p.max_distance, p.photometric_weight, p.max_intensity_difference, p.twist_p[5], p.cos_max_angle) == \
        (700.0, 0.03, 0.25, 0.125, 0.05, math.cos(0.3))
    q = device_icp.pyramid_photometric_params(cam, (48, 64), 3, np.zeros(6), 1.0)
    assert (q.max_intensity_difference, q.angle_gate, q.cos_max_angle, list(q.iterations)) == \
        (math.inf, 0, -1.0, [4, 4, 6, 0])
    for weight, gate in ((0.0, 1.0), (-1.0, 1.0), (math.nan, 1.0), (math.inf, 1.0), (0.1, 0.0), (0.1, math.nan)):
        with pytest.raises(ValueError):
            device_icp.pyramid_photometric_params(cam, (48, 64), 3, np.zeros(6), weight, gate)
    with pytest.raises(ValueError):
        device_icp.pyramid_photometric_params(cam, (48, 64), 3, np.zeros(6), 0.1, iterations=(1, 1, 1, 1))

    t = ProjectiveIcp3d(cam, (2, 5), pyramid=DepthPyramid(levels=2), intensity_pyramid=IntensityPyramid(2),
                        photometric_weight=0.1, max_normal_angle=0.3, max_intensity_difference=0.5)
    assert (t.intensity_pyramid.levels, t.photometric_weight, t.max_normal_angle, t.max_intensity_difference,
            t.iterations, t.strides, t.last_intensity_pyramids, t.last_pyramid) == (2, 0.1, 0.3, 0.5, (2, 5), None,
                                                                                    None, None)
    assert ProjectiveIcp3d(cam).intensity_pyramid is None
    with pytest.raises(ValueError, match="levels"):
        ProjectiveIcp3d(cam, pyramid=DepthPyramid(levels=3), intensity_pyramid=IntensityPyramid(2),
                        photometric_weight=0.1)
    with pytest.raises(ValueError, match="needs both a pyramid and a photometric_weight"):
        ProjectiveIcp3d(cam, intensity_pyramid=IntensityPyramid(), photometric_weight=0.1)
    with pytest.raises(ValueError, match="needs both a pyramid and a photometric_weight"):
        ProjectiveIcp3d(cam, pyramid=DepthPyramid(), intensity_pyramid=IntensityPyramid())
    with pytest.raises(ValueError, match="IntensityPyramid"):
        ProjectiveIcp3d(cam, pyramid=DepthPyramid(), intensity_pyramid=3, photometric_weight=0.1)
    with pytest.raises(ValueError, match="there is no intensity pyramid"):  # today's text, kept
        ProjectiveIcp3d(cam, pyramid=DepthPyramid(), photometric_weight=0.1)
    with pytest.raises(ValueError, match="colour_image and prediction_colour"):
        t.track(None, 0, None, None, np.zeros(6), np.zeros(6))

    kw = dict(camera=cam, field_shape=8, array_offset=[0, 0, 100], colour=True, tracking_reference="icp")
    for bad, match in ((dict(photometric_weight=0.1, icp_pyramid=DepthPyramid()), "there is no intensity pyramid"),
                       (dict(photometric_weight=0.1, icp_pyramid=DepthPyramid(levels=2),
                             icp_intensity_pyramid=IntensityPyramid(3), icp_iterations=(1, 1)), "levels"),
                       (dict(photometric_weight=0.1, icp_intensity_pyramid=IntensityPyramid()), "needs both"),
                       (dict(icp_pyramid=DepthPyramid(), icp_intensity_pyramid=IntensityPyramid()), "needs both"),
                       (dict(photometric_weight=0.1, icp_pyramid=DepthPyramid(), icp_intensity_pyramid="yes"),
                        "IntensityPyramid")):
        with pytest.raises(ValueError, match=match):
            fusion.SequenceFusion3d(**kw, **bad)
    for other in (dict(colour=False), dict(tracking_reference="raycast")):
        with pytest.raises(ValueError, match="photometric_weight needs"):
            fusion.SequenceFusion3d(**dict(kw, **other), photometric_weight=0.1, icp_pyramid=DepthPyramid(),
                                    icp_intensity_pyramid=IntensityPyramid())
    assert "icp_intensity_pyramid" in fusion.__doc__ and "an intensity pyramid" in fusion.__doc__
    not_covered = fusion.__doc__[fusion.__doc__.index("Not covered:"):]
    assert "intensity pyramid" not in not_covered
    assert "prediction depth and normal pyramid" in not_covered and "robust ICP weights" in not_covered
    assert callable(device_icp.icp_run_pyramid_photometric) and callable(device_intensity_pyramid.intensity_pyramid)
    assert lsf.rigid_opt.IntensityPyramid is IntensityPyramid
