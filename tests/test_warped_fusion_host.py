"""CPU checks of warped depth fusion ("Warped depth fusion"): the numpy restatement
(tests/warped_fusion_restatement.py) against the weighted and colour restatements where a warp field reduces to them -- a
zero field, a field of signed zeros, a constant integer shift --, its handling of displacements that are not finite, the
new symbol of the built library, its struct mirror, the entry point's own refusals with no GPU present, the wrapper's
argument checks, and the combinations SequenceFusion3d's constructor accepts."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import colour_restatement as C
import colour_scene as CS
import fusion_scene as S
import fusion_weighted_restatement as FW
import warped_fusion_restatement as WR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsf_hip.h")
SHAPE = (12, 10, 14)
OFF = np.array([-7.5, -5.25, 116.0])  # the middle sphere's front runs through the volume
SHIFT = (2, -1, -3)  # x, y, z: three distinct components


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _case():
    """a painted frame at a non-zero twist, a random model and colour volume, a weight image with unusable pixels"""
    rng = np.random.default_rng(3)
    depth, image, _ = CS.frames()[1]
    t = rng.uniform(-1, 1, SHAPE).astype(F32)
    W = rng.choice(np.array([0, 1, 2.5, 4], F32), SHAPE)
    c = rng.uniform(0, 255, SHAPE + (4,)).astype(F32)
    c[..., 3] = rng.choice(np.array([0, 0, 1, 4], F32), SHAPE)
    pw = rng.uniform(0.1, 2, depth.shape).astype(F32)
    pw[::3, ::2] = 0
    pw[1::7, 1::5] = np.nan
    for a in (t, W, c, pw):
        a.setflags(write=False)
    return depth, image, t, W, c, pw


def _args(off, pw, carve):
    return (S.K, 1.0, off, S.true_twist(1), 20, 0.004, 0.5, 4.0, pw, carve)


def _warped(warp, off=OFF, pw=None, carve=False, colour=False, band=0.25):
    depth, image, t, W, c, _ = _case()
    K, ratio, off, twist, nb, vs, w, cap, pw, carve = _args(off, pw, carve)
    return WR.fuse_depth_warped(t, W, depth, K, ratio, off, twist, warp, nb, vs, w, cap, pw, carve,
                                c if colour else None, image if colour else None, band)


def _assert_equals_the_unwarped_calls(warp, off_unwarped, weighted, carve):
    depth, image, t, W, c, pw = _case()
    pw = pw if weighted else None
    want_t, want_w, want = FW.fuse_depth_weighted(t, W, depth, *_args(off_unwarped, pw, carve))
    got_t, got_w, got_c, rec = _warped(warp, pw=pw, carve=carve)
    assert got_c is None and _bits_equal(got_t, want_t) and _bits_equal(got_w, want_w)
    assert rec == dict(want, coloured=0, first_coloured=0, warp_rejected=0) and tuple(rec) == WR.WARPED_RECORD_FIELDS
    assert want["fused"] > 100 and (want["carved"] > 100) == carve and (want["weight_rejected"] > 20) == weighted
    K, ratio, off, twist, nb, vs, w, cap, _, _ = _args(off_unwarped, pw, carve)
    want_t, want_w, want_c, want = C.fuse_depth_colour(t, W, c, depth, image, K, ratio, off, twist, nb, vs, w, cap, pw,
                                                       carve, 0.25)
    got_t, got_w, got_c, rec = _warped(warp, pw=pw, carve=carve, colour=True)
    assert _bits_equal(got_t, want_t) and _bits_equal(got_w, want_w) and _bits_equal(got_c, want_c)
    assert rec == dict(want, warp_rejected=0) and 0 < want["coloured"] < want["fused"]


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("weighted,carve", [(False, False), (True, True), (True, False), (False, True)])
def test_a_zero_warp_is_the_weighted_and_the_colour_restatement(weighted, carve):
    _assert_equals_the_unwarped_calls(np.zeros(SHAPE + (3,), F32), OFF, weighted, carve)
    signs = np.where(np.random.default_rng(5).integers(0, 2, SHAPE + (3,)) == 1, F32(-0.0), F32(0.0)).astype(F32)
    assert np.signbit(signs).any() and not np.signbit(signs).all()
    _assert_equals_the_unwarped_calls(signs, OFF, weighted, carve)


@pytest.mark.parametrize("weighted,carve", [(False, False), (True, True)])
def test_a_constant_integer_warp_is_a_shifted_array_offset(weighted, carve):
    """channel 0 moves x, 1 y, 2 z: with three distinct components any other order reads another frustum.  The sums
    (index + psi) + offset and index + (offset + psi) are exact in float64 for these values"""
    warp = np.broadcast_to(np.array(SHIFT, F32), SHAPE + (3,)).copy()
    _assert_equals_the_unwarped_calls(warp, OFF + np.array(SHIFT, np.float64), weighted, carve)
    depth, _, t, W, _, _ = _case()
    for other in ((SHIFT[1], SHIFT[0], SHIFT[2]), (SHIFT[2], SHIFT[1], SHIFT[0])):  # the test can tell the orders apart
        swapped = FW.fuse_depth_weighted(t, W, depth, *_args(OFF + np.array(other, np.float64), None, False))[0]
        assert not _bits_equal(swapped, _warped(warp)[0])


def test_a_displacement_that_is_not_finite_leaves_the_voxel_alone_and_is_counted():
    depth, image, t, W, c, pw = _case()
    rng = np.random.default_rng(7)
    warp = rng.uniform(-2, 2, SHAPE + (3,)).astype(F32)
    clean = _warped(warp, pw=pw, carve=True, colour=True)
    bad = np.zeros(SHAPE, bool).reshape(-1)
    flat = warp.reshape(-1, 3)
    for index, channel, value in [(5, 0, np.nan), (77, 1, np.inf), (300, 2, -np.inf), (301, 0, np.nan), (301, 2, np.inf),
                                  (bad.size - 1, 1, np.nan)]:
        flat[index, channel] = value
        bad[index] = True
    changed = np.flatnonzero((clean[0] != t).reshape(-1) & ~bad)[:50]  # and 50 voxels that the clean field updates
    flat[changed, changed % 3] = np.nan
    bad[changed] = True
    bad = bad.reshape(SHAPE)
    got_t, got_w, got_c, rec = _warped(warp, pw=pw, carve=True, colour=True)
    assert rec["warp_rejected"] == np.count_nonzero(bad) == 55
    assert _bits_equal(got_t[bad], t[bad]) and _bits_equal(got_w[bad], W[bad]) and _bits_equal(got_c[bad], c[bad])
    assert _bits_equal(got_t[~bad], clean[0][~bad]) and _bits_equal(got_w[~bad], clean[1][~bad])
    assert _bits_equal(got_c[~bad], clean[2][~bad])
    # counted in warp_rejected and in nothing else: every other count is that of a field which sends the same voxels
    # behind the camera, where there is no pixel to see, to weigh or to reject
    unseen = np.where(bad[..., None], np.array([0, 0, -1e4], F32), warp).astype(F32)
    want = _warped(unseen, pw=pw, carve=True, colour=True)
    assert _bits_equal(got_t, want[0]) and _bits_equal(got_c, want[2])
    assert rec == dict(want[3], warp_rejected=55) and want[3]["warp_rejected"] == 0
    assert rec["fused"] + rec["carved"] <= clean[3]["fused"] + clean[3]["carved"] - 50 and rec["weight_rejected"] > 0
    # a finite displacement that leaves the image, or goes behind the camera, is no rejection
    far = np.zeros(SHAPE + (3,), F32)
    far[..., 0] = 1e6
    behind = np.zeros(SHAPE + (3,), F32)
    behind[..., 2] = -1e4
    for field in (far, behind):
        got_t, got_w, _, rec = _warped(field, carve=True)
        assert _bits_equal(got_t, t) and _bits_equal(got_w, W)
        assert rec["warp_rejected"] == rec["fused"] == rec["carved"] == rec["weight_rejected"] == 0


# ------------------------------------------------------------------------------------------- the library and the host
def _header_struct(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    return [tuple(" ".join(s.split()).rsplit(" ", 1)) for s in body.split(";") if s.strip()]


def test_the_built_library_exports_the_entry_point_and_the_mirror_matches_the_header():
    import levelsetfusion_python_amd as lsf
    L = lsf._lib
    name = "lsf_fusion_integrate_depth_warped"
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, name) and name in L.PROTOTYPES and getattr(L.lib, name).restype is ctypes.c_int
    assert len(L.PROTOTYPES[name][1]) == 11 and L.PROTOTYPES[name][1][9]._type_ is L.FusionWarpedParams
    text = open(HEADER).read()
    assert re.search(r"#define\s+LSF_FUSION_WARPED_RECORD_DOUBLES\s+9\b", text)
    assert re.search(r"#define\s+LSF_FUSION_WARPED_SCRATCH_BYTES\s+\(LSF_FUSION_MAX_BLOCKS \* 9 \* 8\)", text)
    assert re.search(r"#define\s+LSF_FUSION_RECORD_DOUBLES\s+8\b", text) and L.FUSION_RECORD_DOUBLES == 8
    assert L.FUSION_WARPED_RECORD_DOUBLES == 9 and L.FUSION_WARPED_SCRATCH_BYTES == L.FUSION_MAX_BLOCKS * 9 * 8
    assert _header_struct("lsf_fusion_warped_params") == [("lsf_fusion_colour_params", "colour"),
                                                          ("int32_t", "has_colour")]
    fields = L.FusionWarpedParams._fields_
    assert [f[0] for f in fields] == ["colour", "has_colour"]
    assert fields[0][1] is L.FusionColourParams and fields[1][1] is ctypes.c_int32
    assert L.FusionWarpedParams.has_colour.offset == ctypes.sizeof(L.FusionColourParams)
    assert ctypes.sizeof(L.FusionWarpedParams) == ctypes.sizeof(L.FusionColourParams) + 8  # 8-byte aligned: doubles
    # the host refuses before anything touches a device
    p = L.FusionWarpedParams()
    assert getattr(L.lib, name)(None, None, None, None, None, None, None, None, None, ctypes.byref(p), None) == -1
    assert getattr(L.lib, name)(None, None, None, None, None, None, None, None, None, None, None) == -1


# a child without torch and with every GPU hidden: the entry point's own refusals are host code, and a call that a
# refusal should have stopped must find no device to launch on
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
count = ctypes.c_int(-1)
hidden = lib.hipGetDeviceCount(ctypes.byref(count)) != 0 or count.value == 0
fn = lib.lsf_fusion_integrate_depth_warped
fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 11
out = []
for case in json.load(sys.stdin):
    if case["passes"] and not hidden:  # never launch on made-up pointers
        out.append(None)
        continue
    params = ctypes.create_string_buffer(bytes.fromhex(case["params"]))
    out.append(fn(*case["pointers"], params, None))
print(json.dumps(out))
"""


def test_the_entry_point_refuses_on_its_own():
    """lsf_fusion_integrate_depth_warped's refusals behind the wrapper's: NULL required buffers, a misaligned colour
    volume, a has_* flag that disagrees with its pointer, colour_band outside (0, 1], and every pairwise overlap among
    tsdf, weight, colour, warp, depth, pixel_weight and colour_image at the last byte of the earlier buffer.  Made-up
    addresses: every case must return before a launch"""
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_fusion, device_rigid
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    L = lsf._lib
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=0.001)
    shape, (h, w) = (8, 8, 8), (6, 8)
    model, pixels = 8 * 8 * 8 * 4, h * w
    sizes = dict(tsdf=model, weight=model, colour=4 * model, warp=3 * model, depth=2 * pixels, pixel_weight=4 * pixels,
                 image=3 * pixels)
    names = ("tsdf", "weight", "colour", "warp", "depth", "pixel_weight", "image", "record", "scratch")
    base = {name: 0x10000000 + 0x100000 * i for i, name in enumerate(names)}

    def params(band=1.0, has_pixel_weight=1, has_colour=1):
        p = L.FusionWarpedParams()
        f = p.colour.weighted
        f.fusion = device_fusion._params(shape, 1.0, np.inf)
        f.fusion.tsdf = device_rigid._tsdf3d(np.asarray(S.K), cam, torch.zeros((h, w), dtype=torch.int16), 0.004, 20., 1)
        f.fusion.depth_dtype = L.DEPTH_U16
        f.carve, f.has_pixel_weight, p.colour.colour_band, p.has_colour = 1, has_pixel_weight, band, has_colour
        return bytes(p).hex()

    def case(passes=False, params_=None, **moved):
        at = dict(base, **moved)
        return dict(passes=passes, params=params_ or params(), pointers=[at[name] for name in names])

    no_colour = dict(params_=params(has_colour=0), colour=None, image=None)
    refused = {"colour not 16-byte aligned": case(colour=base["colour"] + 4),
               "no colour volume": case(colour=None), "no colour image": case(image=None),
               "has_colour without either": case(colour=None, image=None),
               "a colour volume without has_colour": case(params_=params(has_colour=0), image=None),
               "a colour image without has_colour": case(params_=params(has_colour=0), colour=None),
               "both without has_colour": case(params_=params(has_colour=0)),
               "pixel_weight without has_pixel_weight": case(params_=params(has_pixel_weight=0)),
               "has_pixel_weight without pixel_weight": case(pixel_weight=None)}
    for name in ("tsdf", "weight", "warp", "depth", "record", "scratch"):
        refused["no %s" % name] = case(**{name: None})
        refused["no %s, no colour" % name] = case(**dict(no_colour, **{name: None}))
    for band in (0.0, -0.25, 1.5, float("nan"), float("inf")):
        refused["colour_band %r" % band] = case(params_=params(band=band))
    order = ("tsdf", "weight", "colour", "warp", "depth", "pixel_weight", "image")
    for i, first in enumerate(order):  # the later buffer begins on the earlier one's last byte (or last record)
        for second in order[i + 1:]:
            step = 16 if second == "colour" else 1
            refused["%s overlaps %s" % (second, first)] = case(**{second: base[first] + sizes[first] - step})
            refused["%s overlaps %s" % (first, second)] = case(**{second: base[first] - sizes[second] + step})
    for second in ("tsdf", "weight", "depth", "pixel_weight"):  # and the warp's without a colour volume
        refused["warp overlaps %s, no colour" % second] = case(**dict(no_colour, warp=base[second] + sizes[second] - 1))
    passing = {"the plain call": case(passes=True),
               "no pixel_weight": case(passes=True, params_=params(has_pixel_weight=0), pixel_weight=None),
               "no colour": case(passes=True, **no_colour),
               "no colour, and a band that is then not read": case(passes=True, **dict(
                   no_colour, params_=params(band=0.0, has_colour=0))),
               "colour_band 0.25": case(passes=True, params_=params(band=0.25)),
               "a warp off 16-byte alignment": case(passes=True, warp=base["warp"] + 4),
               "warp right behind colour": case(passes=True, warp=base["colour"] + sizes["colour"]),
               "warp right before depth": case(passes=True, warp=base["depth"] - sizes["warp"])}
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


def test_the_wrapper_checks_the_warp_field():
    import torch
    from levelsetfusion_python_amd import device_fusion
    tsdf, weight = torch.ones((4, 5, 6)), torch.zeros((4, 5, 6))
    others = [("tsdf", tsdf), ("weight", weight), ("colour", None)]
    good = torch.zeros((4, 5, 6, 3))
    device_fusion.check_warp(good, tsdf, others)
    with pytest.raises(TypeError, match="torch tensor"):
        device_fusion.check_warp(np.zeros((4, 5, 6, 3), F32), tsdf, others)
    with pytest.raises(ValueError, match="float32"):
        device_fusion.check_warp(good.double(), tsdf, others)
    with pytest.raises(ValueError, match="contiguous"):
        device_fusion.check_warp(torch.zeros((3, 4, 5, 6)).permute(1, 2, 3, 0), tsdf, others)
    for bad in ((4, 5, 6), (4, 5, 6, 2), (3, 4, 5, 6), (6, 5, 4, 3)):
        with pytest.raises(ValueError, match=r"\+ \(3,\)"):
            device_fusion.check_warp(torch.zeros(bad), tsdf, others)
    both = torch.zeros(4 * 5 * 6 * 4)
    with pytest.raises(ValueError, match="alias weight"):
        device_fusion.check_warp(both[:360].view(4, 5, 6, 3), tsdf, [("tsdf", tsdf), ("weight", both[359:479])])
    device_fusion.check_warp(both[:360].view(4, 5, 6, 3), tsdf, [("tsdf", tsdf), ("weight", both[360:480])])
    rec = device_fusion.unpack_warped_record(np.array([5, 2, 1.5, 0.75, 7, 3, 4, 1, 9], np.float64))
    assert rec == {"fused": 5, "first_seen": 2, "sum_abs_change": 1.5, "max_abs_change": 0.75, "carved": 7,
                   "weight_rejected": 3, "coloured": 4, "first_coloured": 1, "warp_rejected": 9}
    assert device_fusion.WARPED_RECORD_FIELDS == device_fusion.COLOUR_RECORD_FIELDS + ("warp_rejected",)
    assert tuple(rec) == device_fusion.WARPED_RECORD_FIELDS == WR.WARPED_RECORD_FIELDS
    assert device_fusion.WARPED_RECORD == 9 and device_fusion.RECORD == 8


def test_the_sequence_accepts_the_depth_mode_options_with_the_hierarchical_optimizer_only(monkeypatch):
    """the constructor's refusals come before it asks for a GPU: with every GPU hidden, a combination it accepts gets as
    far as that question and a combination it refuses does not"""
    import torch
    import levelsetfusion_python_amd as lsf
    from levelsetfusion_python_amd import device_core
    from levelsetfusion_python_amd.tsdf.generation import DepthCamera
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(device_core, "_gpu_seen", False)
    cam = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=S.K), depth_unit_ratio=1.0)
    hierarchical = lsf.HierarchicalOptimizer3d(tikhonov_strength=0.05, gradient_kernel_enabled=False)
    options = (dict(carve=True), dict(confidence=lsf.DepthConfidence()), dict(colour=True),
               dict(carve=True, confidence=lsf.DepthConfidence(), colour=True), dict())
    for kw in options:
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=hierarchical, **kw)
    for other in (object(), lsf.HierarchicalOptimizer2d(gradient_kernel_enabled=False)):
        for kw in options[:-1]:
            with pytest.raises(ValueError, match="nonrigid_optimizer"):
                lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=other, **kw)
        with pytest.raises(RuntimeError, match="no CPU execution path"):
            lsf.SequenceFusion3d(cam, 32, S.offset(32), nonrigid_optimizer=other)
    assert lsf.fusion.WARPED_RECORD_FIELDS == lsf.fusion.COLOUR_RECORD_FIELDS + ("warp_rejected",)
    assert lsf.fusion.unpack_warped_record is not None and "warp" in lsf.fusion.CanonicalVolume.integrate_depth.__doc__
