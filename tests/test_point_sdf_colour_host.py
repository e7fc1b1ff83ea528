"""CPU checks of point-to-SDF tracking with the colour term and on the depth pyramid: the restatement's own properties
(tests/point_sdf_colour_restatement.py) on tests/textured_wall_scene.py seen by tests/fusion_scene.py's camera -- its
colour Jacobian against finite differences, geometry alone skipping every iteration, the joint runs and sequences whose
errors the GPU tests are bound by --, the ctypes layouts of the two new structs, the header's macros, the exports, and
the refusal of bad arguments by the two C entry points and by the Python interfaces."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import colour_restatement as C
import depth_pyramid_restatement as DP
import fusion_restatement as F
import fusion_scene as S
import icp_restatement as I
import point_sdf_colour_restatement as PC
import pyramid_photometric_restatement as PP
import test_pyramid_photometric_host as PH
import textured_wall_scene as W
from conftest import ROOT

N, LAMBDA, COLOUR_BAND, IMAGE = 64, 0.1, 0.25, (480, 640)
NON_CUBIC = ((40, 36, 52), (-26.25, -18.0, 112.5))  # test_gpu_icp.NON_CUBIC's shape and offset
# the restated joint run of frame 1 against the 64^3 model of frame 0, started from frame 0's twist, iterations
# (4, 4, 6), measured (largest |t error| m, largest |r error| rad): strided 1.0139e-5, 3.6094e-5; on the default
# 3-level pyramid 1.0139e-5, 3.6094e-5.  The three-frame sequences: strided 1.0139e-5, 4.8313e-5; pyramid 1.0139e-5,
# 4.8313e-5.  The GPU bounds are twice these.  Geometry alone leaves frame 1 at its start (3 mm, 1.2e-2 rad) and ends
# frame 2 at 1.3065e-2 m (t_y) and 1.6393e-2 rad (r_z).
RUN_ERROR_T, RUN_ERROR_R = 1.0139e-5, 3.6094e-5
# the same pyramid run against test_gpu_icp.NON_CUBIC's 40 x 36 x 52 model, which holds a third of the coloured voxels
NON_CUBIC_ERROR_T, NON_CUBIC_ERROR_R = 2.0982e-5, 1.1195e-4
SEQUENCE_ERROR_T, SEQUENCE_ERROR_R = 1.0139e-5, 4.8313e-5
RUN_ATOL_T, RUN_ATOL_R = 2 * RUN_ERROR_T, 2 * RUN_ERROR_R
NON_CUBIC_ATOL_T, NON_CUBIC_ATOL_R = 2 * NON_CUBIC_ERROR_T, 2 * NON_CUBIC_ERROR_R
SEQUENCE_ATOL_T, SEQUENCE_ATOL_R = 2 * SEQUENCE_ERROR_T, 2 * SEQUENCE_ERROR_R


@functools.lru_cache(maxsize=None)
def wall_frames(count=3):
    """(depth float32 metres, colour uint8) of the wall's first frames, read only"""
    out = []
    for k in range(count):
        depth, image, _ = W.render(S.true_twist(k), S.K, IMAGE)
        depth.setflags(write=False)
        image.setflags(write=False)
        out.append((depth, image))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wall_model(shape=(N, N, N), offset=None):
    """frame 0 fused with its colour at its true twist (restated): (tsdf, weight, colour, offset), read only"""
    off = S.offset(shape[0]) if offset is None else np.array(offset)
    t, w = F.empty_model(shape)
    depth, image = wall_frames()[0]
    t, w, c, _ = C.fuse_depth_colour(t, w, np.zeros(tuple(shape) + (4,), np.float32), depth, image, S.K, 1.0, off,
                                     S.true_twist(0), colour_band=COLOUR_BAND)
    for a in (t, w, c, off):
        a.setflags(write=False)
    return t, w, c, off


@functools.lru_cache(maxsize=None)
def restated_run(pyramid=False, non_cubic=False):
    """frame 1 against the model from frame 0's twist, joint: (records, twist, residuals, intensity residuals)"""
    t, w, c, off = wall_model(*NON_CUBIC) if non_cubic else wall_model()
    depth, image = wall_frames()[1]
    if not pyramid:
        return PC.track(t, w, depth, S.K, 1.0, S.true_twist(0), off, colour=c, live_colour=image, lam=LAMBDA)[:4]
    depths, _, intr = DP.pyramid(depth, 1.0, S.K)
    return PC.track_pyramid(t, w, depths, intr, S.true_twist(0), off, colour=c,
                            intensities=PP.live_pyramid(image, len(depths)), lam=LAMBDA)[:4]


@functools.lru_cache(maxsize=None)
def restated_sequence(kind):
    """point_sdf_colour_restatement.sequence of the three wall frames at 64^3: kind "strided", "pyramid" (both joint) or
    "geometry" (the plain tracker).  Nothing modifies it"""
    frames = wall_frames()
    kw = dict(strided=dict(lam=LAMBDA), pyramid=dict(lam=LAMBDA, pyramid={}), geometry={})[kind]
    return PC.sequence([f[0] for f in frames], [f[1] for f in frames], S.K, 1.0, (N,) * 3, S.offset(N),
                       colour_band=COLOUR_BAND, **kw)


def twist_errors(twists):
    """(frames, 6) |twist - truth|"""
    return np.abs(np.array(twists) - np.array([S.true_twist(k) for k in range(len(twists))]))


def test_restated_colour_jacobian_against_finite_differences():
    """J_I against central differences of r_I under the left perturbation g <- g + tau + omega x g
    (icp_restatement.compose), step h = 1e-6 per component, at the pairs with a colour term whose voxel coordinates stay
    in one cell for both steps, where Y is one trilinear polynomial.  The bound is computed from the inputs.  With D the
    largest difference of two corner luminances of a cell in use, the trilinear Y has first derivatives <= D, mixed
    second ones <= 2 D, the mixed third one <= 4 D and no pure second or third ones; with L = max |g| / voxel_size the
    point's path p(h) has |p'|, |p''|, |p'''| <= L voxels (a translation is a line of slope 1 / voxel_size <= L, a
    rotation a circle of radius <= |g|).  Truncation: h^2 / 6 times |r'''| <= 6 * 4 D L^3 + 3 * 6 * 2 D L^2 + 3 D L.
    Rounding: g takes about 12 operations on values below max |g| and p = g / voxel_size - offset is rounded at its
    own size P, so p is off by dp = 12 eps max |g| / voxel_size + eps P voxels, r_I by 3 D dp plus 16 eps for Y's own
    operations, and the difference quotient by twice that over 2 h.  The bound is their sum; the test also requires it
    to be below 1e-6 of the largest Jacobian entry it checks, so that it decides something"""
    h, vs, eps = 1e-6, 0.004, 2.0 ** -53
    t, w, c, off = wall_model()
    depth, image = wall_frames()[1]
    src = PC.strided_source(depth, S.K, 1.0, 1, image)
    twist = S.true_twist(0) + np.array([4e-4, -3e-4, 2e-4, 1e-3, -2e-3, 1.5e-3])

    def terms(tw):
        q = PC.terms(t, w, src, tw, off, colour=c)
        return q, [np.floor(x) for x in q["p"]]

    q, cell = terms(twist)
    has = q["has"]
    assert has.sum() > 10000
    y = PC.luminance(c)
    z0, y0, x0 = (cell[2][has].astype(int), cell[1][has].astype(int), cell[0][has].astype(int))
    corners = np.stack([y[z0 + dz, y0 + dy, x0 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    D = float((corners.max(axis=0) - corners.min(axis=0)).max())
    gmax = float(max(np.abs(q["g"][j][has]).max() for j in range(3))) * math.sqrt(3.0)
    L, P = gmax / vs, float(max(np.abs(q["p"][j][has]).max() for j in range(3)))
    truncation = h * h / 6.0 * (24.0 * D * L ** 3 + 36.0 * D * L ** 2 + 3.0 * D * L)
    dp = 12.0 * eps * gmax / vs + eps * P
    rounding = (3.0 * D * dp + 16.0 * eps) / h
    bound = truncation + rounding
    checked, largest = 0, 0.0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        qp, cp = terms(I.compose(twist, d))
        qm, cm = terms(I.compose(twist, -d))
        same = has & qp["has"] & qm["has"]
        for j in range(3):
            same &= (cp[j] == cell[j]) & (cm[j] == cell[j])
        assert same.sum() > 0.9 * has.sum()
        fd = (qp["rI"][same] - qm["rI"][same]) / (2 * h)
        worst = np.abs(fd - q["JI"][k][same]).max()
        print("component %d: |fd - J_I| max %.3e, bound %.3e, |J_I| max %.3e" % (k, worst, bound,
                                                                                np.abs(q["JI"][k][same]).max()))
        assert worst <= bound, (k, worst, bound)
        largest = max(largest, float(np.abs(q["JI"][k][same]).max()))
        checked += int(same.sum())
    assert checked > 10000 and largest > 1.0 and bound < 1e-6 * largest, (checked, largest, bound)


def test_geometry_alone_skips_every_iteration_on_the_wall():
    t, w, _, off = wall_model()
    records, twist = PC.track(t, w, wall_frames()[1][0], S.K, 1.0, S.true_twist(0), off)[:2]
    assert len(records) == 14 and all(r["skipped"] == 1 and r["count"] > 1000 for r in records)
    assert np.array_equal(twist, S.true_twist(0))


@pytest.mark.parametrize("pyramid", [False, True])
def test_restated_joint_run_meets_its_bound(pyramid):
    records, twist, res, ires = restated_run(pyramid)
    assert [r["level"] for r in records] == [0] * 4 + [1] * 4 + [2] * 6
    assert all(r["skipped"] == 0 and 2 * r["photometric_count"] > r["count"] > 1000 for r in records)
    err = np.abs(twist - S.true_twist(1))
    print("restated joint run, pyramid %s: |twist - truth|" % pyramid, err)
    np.testing.assert_allclose([err[:3].max(), err[3:].max()], [RUN_ERROR_T, RUN_ERROR_R], rtol=0.02)
    assert res.shape == ires.shape == IMAGE and np.isfinite(ires).sum() == records[-1]["photometric_count"]
    assert not np.any(np.isfinite(ires) & np.isnan(res))  # only a pixel with a pair has a colour term


def test_restated_joint_run_on_the_non_cubic_volume():
    records, twist, _, _ = restated_run(True, True)
    assert all(r["skipped"] == 0 and 2 * r["photometric_count"] > r["count"] > 1000 for r in records)
    err = np.abs(twist - S.true_twist(1))
    np.testing.assert_allclose([err[:3].max(), err[3:].max()], [NON_CUBIC_ERROR_T, NON_CUBIC_ERROR_R], rtol=0.02)


@pytest.mark.parametrize("kind", ["strided", "pyramid"])
def test_restated_joint_sequence_meets_its_bound(kind):
    _, _, colour, twists, records = restated_sequence(kind)
    assert records[0] == [] and all(len(r) == 14 for r in records[1:])
    for frame in records[1:]:
        assert all(r["skipped"] == 0 and 2 * r["photometric_count"] > r["count"] for r in frame)
    err = twist_errors(twists)
    print("restated joint %s sequence, |twist - truth| per frame:\n" % kind, err)
    np.testing.assert_allclose([err[1:, :3].max(), err[1:, 3:].max()], [SEQUENCE_ERROR_T, SEQUENCE_ERROR_R], rtol=0.02)
    assert err[1:, :3].max() <= SEQUENCE_ATOL_T and err[1:, 3:].max() <= SEQUENCE_ATOL_R
    assert (colour[..., 3] > 0).sum() > 10000


def test_the_geometry_only_sequence_drifts_in_the_plane():
    """the plain tracker on the same frames: every iteration of frame 1 is skipped, and frame 2 ends outside the joint
    sequences' bounds in t_y and r_z, the wall's free directions"""
    _, _, _, twists, records = restated_sequence("geometry")
    assert all(r["skipped"] == 1 for r in records[1])
    err = twist_errors(twists)
    assert err[2, 1] > 100 * SEQUENCE_ATOL_T and err[2, 5] > 100 * SEQUENCE_ATOL_R, err
    np.testing.assert_allclose([err[2, 1], err[2, 5]], [1.3065e-2, 1.6393e-2], rtol=0.02)


def test_params_layout_and_macros():
    import levelsetfusion_python_amd._lib as lib
    old = lib.PointSdfParams
    p, q = lib.PointSdfPhotometricParams, lib.PointSdfPyramidParams
    colour = ["photometric_weight", "max_intensity_difference", "intensity_scale"]
    assert [f[0] for f in p._fields_] == [f[0] for f in old._fields_] + colour
    assert [f[0] for f in q._fields_] == [f[0] for f in p._fields_] + ["pyramid_levels", "reserved"]
    for s in (p, q):
        for name, _ in old._fields_:  # the old members first, where they were
            assert getattr(s, name).offset == getattr(old, name).offset, name
        assert (s.loss.offset, s.photometric_weight.offset, s.max_intensity_difference.offset,
                s.intensity_scale.offset) == (156, 160, 168, 176)
    assert ctypes.sizeof(old) == 160 and ctypes.sizeof(p) == 184 and ctypes.sizeof(q) == 192
    assert (q.pyramid_levels.offset, q.reserved.offset) == (184, 188)
    assert lib.POINT_SDF_COLOUR_SCRATCH_BYTES == 2 * 256 * 35 * 8 and lib.POINT_SDF_SCRATCH_BYTES == 2 * 256 * 33 * 8
    header = open(os.path.join(ROOT, "include", "lsf_hip.h")).read()
    for text in ("#define LSF_POINT_SDF_COLOUR_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 35 * 8)",
                 "#define LSF_POINT_SDF_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 33 * 8)", "#define LSF_ABI_VERSION 4",
                 "} lsf_point_sdf_photometric_params;", "} lsf_point_sdf_pyramid_params;",
                 "lsf_point_sdf_run_photometric(", "lsf_point_sdf_run_pyramid("):
        assert text in header, text
    assert lib.ABI_VERSION == 4 and lib.lib.lsf_abi_version() == 4
    for name in ("lsf_point_sdf_run_photometric", "lsf_point_sdf_run_pyramid"):
        assert len(lib.PROTOTYPES[name][1]) == 13 and getattr(lib.lib, name) is not None
    assert len(lib.PROTOTYPES["lsf_point_sdf_run"][1]) == 10


H, WID, VOLUME, LEVELS = 48, 64, (8, 10, 12), 3
_VOXELS = 4 * VOLUME[0] * VOLUME[1] * VOLUME[2]
_PIXELS = sum((H >> l) * (WID >> l) for l in range(LEVELS))


def _fill(p, iterations, strides, fields):
    p.fx, p.fy, p.cx, p.cy, p.depth_unit_ratio, p.max_distance = 70.0, 70.0, 32.0, 24.0, 0.001, 0.02
    p.voxel_size, p.narrow_band_width_voxels, p.scale = 0.004, 20.0, 0.003
    p.offset_x, p.offset_y, p.offset_z = -6.0, -5.0, 100.0
    p.depth, p.height, p.width = VOLUME
    p.image_height, p.image_width, p.depth_dtype, p.levels = H, WID, 0, len(iterations)
    p.iterations[:len(iterations)] = list(iterations)
    p.strides[:len(strides)] = list(strides)
    p.loss, p.photometric_weight, p.max_intensity_difference, p.intensity_scale = 2, 0.1, 0.2, 0.05
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _cases(entry, make, names, sizes, outs, last_image):
    """the refusals the two entry points share; make(**fields) is the parameter struct, names the pointer arguments in
    order, sizes the inputs' bytes, outs the outputs' bytes, last_image the bytes of a residual image"""
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}  # 1 MiB apart: nothing aliases
    optional = ("residuals", "intensity", "weights")

    def case(want=-1, p=None, no_params=False, **moved):
        at = dict(base, **{name: None for name in optional})
        at.update(moved)
        return dict(entry=entry, passes=want is None, want=want, pointers=[at[name] for name in names],
                    params=None if no_params else bytes(p or make()).hex())

    live = names[4]  # the live colour input
    no_colour = {"colour": None, live: None}
    cases = {"no params": case(no_params=True), "tsdf is weight": case(weight=base["tsdf"])}
    for name in ("tsdf", "weight", names[3], "twist", "records", "scratch"):
        cases["no %s" % name] = case(**{name: None})
    for field, value in (("image_height", 0), ("image_width", -1), ("depth", 1), ("height", 1), ("width", 1),
                         ("fx", 0.0), ("fy", math.nan), ("cx", math.inf), ("max_distance", 0.0),
                         ("max_distance", math.nan), ("voxel_size", 0.0), ("voxel_size", math.nan),
                         ("voxel_size", math.inf), ("narrow_band_width_voxels", 0.0),
                         ("narrow_band_width_voxels", math.nan), ("offset_x", math.nan), ("offset_z", math.inf),
                         ("levels", 0), ("levels", 5), ("loss", 3), ("loss", -1), ("scale", 0.0), ("scale", math.nan),
                         ("photometric_weight", -0.1), ("photometric_weight", math.nan),
                         ("photometric_weight", math.inf), ("photometric_weight", 0.0),
                         ("max_intensity_difference", 0.0), ("max_intensity_difference", -1.0),
                         ("max_intensity_difference", math.nan), ("intensity_scale", 0.0),
                         ("intensity_scale", -0.05), ("intensity_scale", math.nan)):
        cases["%s %r" % (field, value)] = case(p=make(**{field: value}))
    cases["a negative iteration count"] = case(p=make(iterations=(2, -1, 3)))
    cases["too many pixels"] = case(p=make(image_height=1 << 16, image_width=1 << 15))
    cases["a weight image without a loss"] = case(p=make(loss=0), weights=base["weights"])
    cases["a colour volume without a live colour"] = case(**{live: None})
    cases["a live colour without a colour volume"] = case(colour=None)
    cases["a weight without the colour inputs"] = case(**no_colour)
    cases["an intensity image without the colour inputs"] = case(p=make(photometric_weight=0.0),
                                                                 intensity=base["intensity"], **no_colour)
    cases["a bad gate without the colour inputs"] = case(p=make(photometric_weight=0.0, max_intensity_difference=0.0),
                                                         **no_colour)
    cases["a bad intensity scale without the colour inputs"] = case(p=make(photometric_weight=0.0,
                                                                           intensity_scale=math.nan), **no_colour)
    for shift in (4, 8, 12):
        cases["a colour volume %d bytes off alignment" % shift] = case(colour=base["colour"] + shift)
    for out, size in outs.items():
        for name, bytes_ in sizes.items():
            cases["%s in the last byte of %s" % (out, name)] = case(**{out: base[name] + bytes_ - 1})
            cases["%s over the first byte of %s" % (out, name)] = case(**{out: base[name] - size + 1})
    cases["the weights alias the residuals"] = case(residuals=base["residuals"], weights=base["residuals"])
    cases["the intensity image aliases the residuals"] = case(residuals=base["residuals"],
                                                              intensity=base["residuals"] + last_image - 1)
    cases["the intensity image aliases the weights"] = case(intensity=base["weights"], weights=base["weights"])
    cases["the residuals alias the scratch"] = case(residuals=base["scratch"])
    cases["the intensity image aliases the twist"] = case(intensity=base["twist"])
    cases["the plain call"] = case(want=None)
    cases["all three images"] = case(want=None, residuals=base["residuals"], intensity=base["intensity"],
                                     weights=base["weights"])
    cases["no loss"] = case(want=None, p=make(loss=0, scale=math.nan, intensity_scale=math.nan),
                            residuals=base["residuals"], intensity=base["intensity"])
    cases["geometry alone"] = case(want=None, p=make(photometric_weight=0.0), residuals=base["residuals"],
                                   weights=base["weights"], **no_colour)
    cases["geometry alone without a loss"] = case(want=None, p=make(photometric_weight=0.0, loss=0), **no_colour)
    cases["infinite scales and gate"] = case(want=None, p=make(scale=math.inf, intensity_scale=math.inf,
                                                               max_intensity_difference=math.inf))
    cases["the smallest volume"] = case(want=None, p=make(depth=2, height=2, width=2))
    cases["an intensity image right behind the residuals"] = case(want=None, residuals=base["residuals"],
                                                                  intensity=base["residuals"] + last_image)
    cases["nothing to launch"] = case(want=0, p=make(iterations=(0, 0, 0)), records=None,
                                      residuals=base["residuals"], intensity=base["intensity"])
    return cases, case, base


def test_the_strided_entry_point_refuses_bad_arguments_before_launching():
    """lsf_point_sdf_run's refusals, the colour term's, and the aliasing check over the colour volume, the colour image
    and the intensity residual image"""
    import levelsetfusion_python_amd._lib as lib

    def make(iterations=(2, 0, 3), strides=(4, 2, 1), **fields):
        return _fill(lib.PointSdfPhotometricParams(), iterations, strides, fields)

    names = ("tsdf", "weight", "colour", "live_depth", "live_colour", "twist", "records", "scratch", "residuals",
             "intensity", "weights")
    sizes = dict(tsdf=_VOXELS, weight=_VOXELS, colour=4 * _VOXELS, live_depth=2 * H * WID, live_colour=3 * H * WID)
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.POINT_SDF_COLOUR_SCRATCH_BYTES, residuals=4 * H * WID,
                intensity=4 * H * WID, weights=4 * H * WID)
    cases, case, base = _cases("lsf_point_sdf_run_photometric", make, names, sizes, outs, 4 * H * WID)
    cases["depth_unit_ratio nan"] = case(p=make(depth_unit_ratio=math.nan))
    cases["depth_dtype 9"] = case(p=make(depth_dtype=9))
    cases["a stride of 0"] = case(p=make(strides=(4, 0, 1)))
    PH._check(cases)


def test_the_pyramid_entry_point_refuses_bad_arguments_before_launching():
    """the same, and the pyramid's own: its levels and their extents; the images have the last iteration's level's"""
    import levelsetfusion_python_amd._lib as lib

    def make(iterations=(2, 0, 3), **fields):
        return _fill(lib.PointSdfPyramidParams(), iterations, (), dict(dict(pyramid_levels=LEVELS), **fields))

    names = ("tsdf", "weight", "colour", "pyramid_depth", "pyramid_intensity", "twist", "records", "scratch",
             "residuals", "intensity", "weights")
    sizes = dict(tsdf=_VOXELS, weight=_VOXELS, colour=4 * _VOXELS, pyramid_depth=4 * _PIXELS,
                 pyramid_intensity=4 * _PIXELS)
    outs = dict(twist=48, records=5 * 64 * 8, scratch=lib.POINT_SDF_COLOUR_SCRATCH_BYTES, residuals=4 * H * WID,
                intensity=4 * H * WID, weights=4 * H * WID)
    cases, case, base = _cases("lsf_point_sdf_run_pyramid", make, names, sizes, outs, 4 * H * WID)
    for levels in (0, -1, 5):
        cases["pyramid_levels %d" % levels] = case(p=make(pyramid_levels=levels))
    cases["more tracked levels than the pyramid has"] = case(p=make(pyramid_levels=2))
    cases["a level without pixels"] = case(p=make(image_height=3, iterations=(1,)))
    cases["the ratio, the depth type and the strides are not read"] = case(
        want=None, p=make(depth_unit_ratio=math.nan, depth_dtype=9))
    # the last iteration runs on level 1: images of 24 x 32 fit where full-size ones would alias
    quarter = 4 * (H >> 1) * (WID >> 1)
    cases["a level-1 image right behind the residuals"] = case(want=None, p=make(iterations=(2, 3, 0)),
                                                               residuals=base["residuals"],
                                                               intensity=base["residuals"] + quarter)
    cases["a level-1 image in the residuals' last byte"] = case(p=make(iterations=(2, 3, 0)),
                                                                residuals=base["residuals"],
                                                                intensity=base["residuals"] + quarter - 1)
    cases["one level of 1 x 1"] = case(want=None, p=make(image_height=1, image_width=1, pyramid_levels=1,
                                                         iterations=(1,)))
    PH._check(cases)


def test_python_argument_checks():
    import inspect

    from levelsetfusion_python_amd import device_point_sdf, fusion
    from levelsetfusion_python_amd.rigid_opt import DepthPyramid, IntensityPyramid, PointToSdf3d, RobustLoss
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    loss = RobustLoss("tukey", 0.003, 0.05)
    args = dict(shape=(40, 36, 52), camera=cam, image_shape=(480, 640), array_offset=[-26.25, -18.0, 112.5])
    p = device_point_sdf.photometric_params(depth_code=0, robust=loss, photometric_weight=0.1,
                                            max_intensity_difference=0.2, **args)
    assert (p.photometric_weight, p.max_intensity_difference, p.intensity_scale, p.loss, p.scale) == \
        (0.1, 0.2, 0.05, 2, 0.003)
    assert (p.depth, p.height, p.width, p.image_height, p.image_width, p.levels) == (40, 36, 52, 480, 640, 3)
    p = device_point_sdf.photometric_params(depth_code=1, **args)
    assert (p.photometric_weight, p.max_intensity_difference, p.intensity_scale, p.loss) == (0.0, math.inf, math.inf, 0)
    p = device_point_sdf.pyramid_params(pyramid_levels=3, iterations=(2, 5), photometric_weight=0.25, **args)
    assert (p.pyramid_levels, p.levels, list(p.iterations), p.depth_unit_ratio, p.photometric_weight) == \
        (3, 2, [2, 5, 0, 0], 1.0, 0.25)
    for bad in (dict(photometric_weight=0.0), dict(photometric_weight=-1.0), dict(photometric_weight=math.inf),
                dict(photometric_weight=math.nan), dict(max_intensity_difference=0.0),
                dict(max_intensity_difference=math.nan), dict(robust="tukey"), dict(voxel_size=0.0)):
        with pytest.raises(ValueError):
            device_point_sdf.photometric_params(depth_code=0, **args, **bad)
        with pytest.raises(ValueError):
            device_point_sdf.pyramid_params(pyramid_levels=3, **args, **bad)
    for bad in (dict(pyramid_levels=0), dict(pyramid_levels=5), dict(pyramid_levels=2),
                dict(pyramid_levels=3, iterations=(1, -1, 1)), dict(pyramid_levels=4, image_shape=(7, 640),
                                                                    iterations=(1,))):
        with pytest.raises(ValueError):
            device_point_sdf.pyramid_params(**dict(args, **bad))

    # the positional order and the defaults of the first five arguments; the new keywords behind them
    sig = inspect.signature(PointToSdf3d.__init__)
    assert list(sig.parameters)[1:] == ["camera", "iterations", "strides", "max_distance", "robust", "pyramid",
                                        "photometric_weight", "max_intensity_difference", "intensity_pyramid"]
    assert [sig.parameters[n].default for n in ("iterations", "strides", "max_distance", "robust", "pyramid",
                                                "photometric_weight", "max_intensity_difference",
                                                "intensity_pyramid")] == \
        [(4, 4, 6), (4, 2, 1), 0.02, None, None, None, math.inf, None]
    t = PointToSdf3d(cam)
    assert (t.pyramid, t.photometric_weight, t.max_intensity_difference, t.intensity_pyramid) == \
        (None, None, math.inf, None)
    assert t.last_intensity_residuals is None and t.last_pyramid is None and t.last_intensity_pyramid is None
    t = PointToSdf3d(cam, (2, 3), pyramid=DepthPyramid(), photometric_weight=0.1, intensity_pyramid=IntensityPyramid(),
                     max_intensity_difference=0.2, robust=loss)
    assert (t.iterations, t.strides, t.photometric_weight, t.max_intensity_difference) == ((2, 3), None, 0.1, 0.2)
    assert PointToSdf3d(cam, photometric_weight=0.1).strides == (4, 2, 1)
    for bad in (dict(pyramid="pyramid"), dict(pyramid=DepthPyramid(), photometric_weight=0.1),
                dict(intensity_pyramid=IntensityPyramid()), dict(intensity_pyramid=IntensityPyramid(),
                                                                 photometric_weight=0.1),
                dict(pyramid=DepthPyramid(), intensity_pyramid=IntensityPyramid()),
                dict(pyramid=DepthPyramid(), intensity_pyramid=IntensityPyramid(2), photometric_weight=0.1),
                dict(pyramid=DepthPyramid(), intensity_pyramid="pyramid", photometric_weight=0.1),
                dict(pyramid=DepthPyramid(levels=2), iterations=(1, 1, 1)), dict(photometric_weight=0.0),
                dict(photometric_weight=math.nan), dict(max_intensity_difference=0.0)):
        with pytest.raises(ValueError):
            PointToSdf3d(cam, **bad)
    # colour and colour_image go with a photometric_weight, and only with one: checked before the device is touched
    with pytest.raises(ValueError, match="colour and colour_image"):
        PointToSdf3d(cam, photometric_weight=0.1).track(None, 0, None, None, [0, 0, 0], np.zeros(6))
    with pytest.raises(ValueError, match="colour and colour_image"):
        PointToSdf3d(cam).track(None, 0, None, None, [0, 0, 0], np.zeros(6), colour=object(), colour_image=object())
    with pytest.raises(ValueError, match="colour and colour_image"):
        PointToSdf3d(cam, photometric_weight=0.1).track(None, 0, None, None, [0, 0, 0], np.zeros(6), colour=object())

    kw = dict(camera=cam, field_shape=8, array_offset=[0, 0, 100], tracking_reference="sdf")
    joint = PointToSdf3d(cam, photometric_weight=0.1)
    with pytest.raises(ValueError, match="needs colour=True"):
        fusion.SequenceFusion3d(**kw, sdf_tracker=joint)
    for name, value in (("photometric_weight", 0.1), ("icp_robust", loss), ("icp_pyramid", DepthPyramid()),
                        ("icp_max_normal_angle", 0.3), ("icp_intensity_pyramid", IntensityPyramid())):
        with pytest.raises(ValueError, match="%s belongs to the \"icp\" tracker" % name):
            fusion.SequenceFusion3d(**kw, colour=True, sdf_tracker=joint, **{name: value})
    doc = " ".join(fusion.__doc__.split())
    not_covered = doc[doc.index("Not covered:"):]
    assert "intensity pyramid" not in not_covered and "settings of the `sdf_tracker`" in not_covered
    assert "PointToSdf3d(photometric_weight=)" in doc and "PointToSdf3d(pyramid=)" in doc
    assert "intensity_scale is not used" not in " ".join(inspect.getmodule(PointToSdf3d).__doc__.split())
