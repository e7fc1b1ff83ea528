"""GPU checks of the one voxel walk of csrc/lsf_fusion.hip (fusion_kernel<RULE>) where every entry point now takes one
code path: a model that is a tail alone, every tail length through the colour and the warped rule, and the choice of
the entry point from the arguments (device_fusion.integrate_depth_by_arguments behind CanonicalVolume.integrate_depth).
tsdf, weight and the colour volume are compared bit for bit with the numpy restatements, the record's counts and maximum
exactly, and its float64 sum to the 1e-12 relative of tests/fusion_restatement.py."""
import functools

import numpy as np
import pytest
import torch

import colour_restatement as C
import fusion_restatement as F
import fusion_weighted_restatement as FW
import warped_fusion_restatement as WR
from test_gpu_colour import CAP, _assert_colour_record, _random_colour
from test_gpu_colour import _call as _colour_call
from test_gpu_fusion import _assert_record as _assert_plain_record
from test_gpu_fusion import _host_record
from test_gpu_fusion_weighted import TWIST, _assert_record, _random_model
from test_gpu_fusion_weighted import _unpack as _unpack_weighted
from test_gpu_rigid3d import _depth
from test_gpu_warped_fusion import _assert_warped_record, _bits_equal, _camera, _device
from test_gpu_warped_fusion import _call as _warped_call
from test_gpu_warped_fusion import _unpack as _unpack_warped
from test_rigid3d_host import K_SYN

pytestmark = pytest.mark.gpu

BAND = 0.1  # the colour band: a part of the voxels in band lie outside it
# under TWIST the synthetic surface crosses the camera's axis near z = 246 voxels: these offsets put it through the volumes
TAIL_ONLY = ((1, 1, 3), np.array([-1.0, 0.25, 245.0]))
# 105, 90 and 75 voxels: 26, 22 and 18 four-voxel steps on one workgroup and a tail of 1, 2 and 3
TAILS = [((3, 5, 7), 1), ((3, 5, 6), 2), ((3, 5, 5), 3)]
TAILS_OFF = np.array([-3.5, -2.25, 244.0])
GEN = (K_SYN, 0.001)
RULE = (20, 0.004, 0.5, CAP)  # band, voxel_size, w, max_weight


@pytest.fixture(scope="module")
def lsf():
    import levelsetfusion_python_amd as m
    return m


@functools.lru_cache(maxsize=None)
def _inputs():
    """the rigid tests' uint16 depth image, a random colour image and a weight image in [0.5, 2) with a few unusable
    pixels; made once, never written"""
    d = _depth(np.uint16)
    rng = np.random.default_rng(53)
    image = rng.integers(0, 256, d.shape + (3,)).astype(np.uint8)
    pw = rng.uniform(0.5, 2, d.shape).astype(np.float32)
    pw.reshape(-1)[::29] = 0
    pw.reshape(-1)[5::31] = np.nan
    for a in (d, image, pw):
        a.setflags(write=False)
    return d, image, pw


def _random_warp(shape, rng):
    """psi in [-1, 1]^3, one voxel's not finite"""
    warp = rng.uniform(-1, 1, shape + (3,)).astype(np.float32)
    warp.reshape(-1, 3)[1, 2] = np.nan
    return warp


def _assert_model(got_t, got_w, want_t, want_w):
    assert _bits_equal(got_t.cpu().numpy(), want_t) and _bits_equal(got_w.cpu().numpy(), want_w)


# -------------------------------------------------------------------------------------- 1. a model that is a tail alone
def test_a_model_of_three_voxels_is_the_tail_alone(lsf):
    """no four-voxel step, one workgroup, lane 0 does everything: all five entry points against their restatements"""
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    shape, off = TAIL_ONLY
    assert int(np.prod(shape)) // 4 == 0 and int(np.prod(shape)) % 4 == 3
    d, image, pw = _inputs()
    dev, code = gen.device_depth(d)
    rng = np.random.default_rng(59)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    cam = _camera(K_SYN)

    live = np.array([0.3, 1.0, -0.5], np.float32).reshape(shape)
    want_t, want_w, want = F.fuse(t, W, live, 0.5, CAP)
    assert want["fused"] == 2
    a_t, a_w, a_l = _device(t, W, live)
    rec = device_fusion.integrate_volume(a_t, a_w, a_l, 0.5, CAP)
    _assert_model(a_t, a_w, want_t, want_w)
    _assert_plain_record(_host_record(rec), want)

    want_t, want_w, want = F.fuse_depth(t, W, d, *GEN, off, TWIST, *RULE)
    assert want["fused"] > 0
    a_t, a_w = _device(t, W)
    rec = device_fusion.integrate_depth(a_t, a_w, dev, code, cam, off, TWIST, w=0.5, max_weight=CAP)
    _assert_model(a_t, a_w, want_t, want_w)
    _assert_plain_record(_host_record(rec), want)

    want_t, want_w, want = FW.fuse_depth_weighted(t, W, d, *GEN, off, TWIST, *RULE, pw, True)
    assert want["fused"] > 0
    a_t, a_w = _device(t, W)
    rec = device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, cam, off, TWIST, w=0.5, max_weight=CAP,
                                                 pixel_weight=_device(pw)[0], carve=True)
    _assert_model(a_t, a_w, want_t, want_w)
    _assert_record(_unpack_weighted(rec), want)

    want_t, want_w, want_c, want = C.fuse_depth_colour(t, W, c, d, image, *GEN, off, TWIST, *RULE, pw, True, BAND)
    assert want["fused"] > 0 and want["coloured"] > 0
    a_t, a_w, a_c, rec = _colour_call(t, W, c, d, image, pw, off, True, BAND)
    _assert_model(a_t, a_w, want_t, want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_colour_record(lsf.fusion.unpack_colour_record(rec.cpu().numpy()), want)

    warp = rng.uniform(-1, 1, shape + (3,)).astype(np.float32)
    want_t, want_w, want_c, want = WR.fuse_depth_warped(t, W, d, *GEN, off, TWIST, warp, *RULE, pw, True, c, image, BAND)
    assert want["fused"] > 0 and want["coloured"] > 0
    a_t, a_w, a_c, rec = _warped_call(t, W, c, warp, d, image, pw, off, True, band=BAND)
    _assert_model(a_t, a_w, want_t, want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_warped_record(_unpack_warped(rec), want)


# -------------------------------------------------------------------- 2. every tail length through the colour and warped rules
@pytest.mark.parametrize("shape,tail", TAILS)
def test_every_tail_length_through_the_colour_rule(lsf, shape, tail):
    assert int(np.prod(shape)) % 4 == tail and int(np.prod(shape)) // 4 <= 256
    d, image, pw = _inputs()
    rng = np.random.default_rng(61)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    want_t, want_w, want_c, want = C.fuse_depth_colour(t, W, c, d, image, *GEN, TAILS_OFF, TWIST, *RULE, pw, True, BAND)
    assert want["fused"] > 0 and want["coloured"] > 0
    assert np.any(want_t.reshape(-1)[-tail:].view(np.uint32) != t.reshape(-1)[-tail:].view(np.uint32))  # in the tail too
    a_t, a_w, a_c, rec = _colour_call(t, W, c, d, image, pw, TAILS_OFF, True, BAND)
    _assert_model(a_t, a_w, want_t, want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_colour_record(lsf.fusion.unpack_colour_record(rec.cpu().numpy()), want)


@pytest.mark.parametrize("shape,tail", TAILS)
def test_every_tail_length_through_the_warped_rule(lsf, shape, tail):
    assert int(np.prod(shape)) % 4 == tail and int(np.prod(shape)) // 4 <= 256
    d, image, pw = _inputs()
    rng = np.random.default_rng(67)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    warp = _random_warp(shape, rng)
    want_t, want_w, want_c, want = WR.fuse_depth_warped(t, W, d, *GEN, TAILS_OFF, TWIST, warp, *RULE, pw, True, c, image,
                                                        BAND)
    assert want["fused"] > 0 and want["coloured"] > 0 and want["warp_rejected"] == 1
    assert np.any(want_t.reshape(-1)[-tail:].view(np.uint32) != t.reshape(-1)[-tail:].view(np.uint32))  # in the tail too
    a_t, a_w, a_c, rec = _warped_call(t, W, c, warp, d, image, pw, TAILS_OFF, True, band=BAND)
    _assert_model(a_t, a_w, want_t, want_w)
    assert _bits_equal(a_c.cpu().numpy(), want_c)
    _assert_warped_record(_unpack_warped(rec), want)


# ------------------------------------------------------------------------------------- 3. the arguments pick the entry point
PICKS = {"plain": {}, "pixel_weight": dict(pixel_weight=True), "carve": dict(carve=True),
         "colour": dict(colour_image=True, pixel_weight=True, carve=True), "warp": dict(warp=True, carve=True),
         "warp and colour": dict(warp=True, colour_image=True, pixel_weight=True)}


@pytest.mark.parametrize("pick", sorted(PICKS))
def test_the_volume_calls_the_entry_point_its_arguments_name(lsf, pick):
    """CanonicalVolume.integrate_depth gives the model bits and the record of the device_fusion call of that name"""
    from levelsetfusion_python_amd import device_fusion
    from levelsetfusion_python_amd.tsdf import generation as gen
    given = PICKS[pick]
    shape, _ = TAILS[0]
    d, image, pw = _inputs()
    dev, code = gen.device_depth(d)
    rng = np.random.default_rng(71)
    t, W = _random_model(shape, rng, CAP)
    c = _random_colour(shape, rng)
    cam = _camera(K_SYN)
    pw_dev = _device(pw)[0] if given.get("pixel_weight") else None
    img = _device(image)[0] if given.get("colour_image") else None
    psi = _device(_random_warp(shape, rng))[0] if given.get("warp") else None
    carve = bool(given.get("carve"))

    a_t, a_w, a_c = _device(t, W, c)
    rule = dict(w=0.5, max_weight=CAP)
    if psi is not None:
        want = device_fusion.integrate_depth_warped(a_t, a_w, dev, code, cam, TAILS_OFF, TWIST, psi, pixel_weight=pw_dev,
                                                    carve=carve, colour=None if img is None else a_c, colour_image=img,
                                                    colour_band=BAND, **rule)
    elif img is not None:
        want = device_fusion.integrate_depth_colour(a_t, a_w, a_c, dev, code, cam, TAILS_OFF, TWIST, img,
                                                    pixel_weight=pw_dev, carve=carve, colour_band=BAND, **rule)
    elif pw_dev is not None or carve:
        want = device_fusion.integrate_depth_weighted(a_t, a_w, dev, code, cam, TAILS_OFF, TWIST, pixel_weight=pw_dev,
                                                      carve=carve, **rule)
    else:
        want = device_fusion.integrate_depth(a_t, a_w, dev, code, cam, TAILS_OFF, TWIST, **rule)
    assert want.cpu().numpy()[0] > 0  # fused

    vol = lsf.fusion.CanonicalVolume(shape, max_weight=CAP, colour=True)
    vol.tsdf.copy_(torch.from_numpy(t)), vol.weight.copy_(torch.from_numpy(W)), vol.colour.copy_(torch.from_numpy(c))
    got = vol.integrate_depth(dev, cam, TWIST, TAILS_OFF, weight=0.5, pixel_weight=pw_dev, carve=carve, colour_image=img,
                              colour_band=BAND, warp=psi)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint64), want.cpu().numpy().view(np.uint64))
    for a, b in ((vol.tsdf, a_t), (vol.weight, a_w), (vol.colour, a_c)):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert (img is not None) == bool(np.any(a_c.cpu().numpy() != c))  # the colour volume changed with an image only
